from matinvent_amd.rewards import Elastic, HeatCapacity, PyMatGen, Surrogate  # noqa: F401
