from matinvent_amd.rewards import HeatCapacity, PyMatGen, Surrogate  # noqa: F401
