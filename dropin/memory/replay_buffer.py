from matinvent_amd.memory import ReplayBuffer  # noqa: F401
