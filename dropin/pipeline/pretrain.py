from matinvent_amd.pipeline import Pretrain  # noqa: F401
