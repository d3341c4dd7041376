from matinvent_amd.rewards import Elastic, HeatCapacity, PyMatGen, Surrogate, Symmetry  # noqa: F401
