from matinvent_amd.memory import LongTimeMem  # noqa: F401
