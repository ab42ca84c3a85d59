# Data package (drop-in for the reference's src/data): the datasets and their collation.
