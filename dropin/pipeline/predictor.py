from matinvent_amd.pipeline import TrainPredictor  # noqa: F401
