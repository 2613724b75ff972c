"""Data side of the reference's package tree (disprcnn/data).  Only the evaluation entry points live here; dataset classes and loading
are not part of this implementation."""
