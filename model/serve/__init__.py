"""`model.serve`: the serving worker's face (model_worker.py)."""
