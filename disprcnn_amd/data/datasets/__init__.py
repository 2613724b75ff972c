"""disprcnn/data/datasets: the evaluation package only.  The dataset classes themselves (KITTIObjectDatasetCar, ...) are not provided;
`evaluation.evaluate` recognises them by class name."""
