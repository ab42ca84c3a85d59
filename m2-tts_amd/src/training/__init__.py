# Training package (drop-in for the reference's src/training): the loss functions.
