# Evaluation package (drop-in for the reference's src/evaluation).
