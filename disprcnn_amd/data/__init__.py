"""Data side of the reference's package tree (disprcnn/data): the transforms (`transforms/`), the collators and the device input path
(`collate_batch.py`, `device_input.py`) and the evaluation entry points (`datasets/evaluation/`).  Dataset classes, samplers and
`make_data_loader` are not part of this implementation."""
