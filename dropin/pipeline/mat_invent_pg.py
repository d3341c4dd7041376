from matinvent_amd.pipeline import MatInventPG  # noqa: F401
