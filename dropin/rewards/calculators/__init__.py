from matinvent_amd.rewards import PyMatGen, Surrogate  # noqa: F401
