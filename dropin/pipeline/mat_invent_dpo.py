from matinvent_amd.pipeline import MatInventDPO  # noqa: F401
