"""Scene loading (reference code/datasets/)."""
