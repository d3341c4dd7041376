"""The uniqueness / novelty filter under the drop-in import path (configs/filter/un.yaml)."""
from matinvent_amd.novelty import FingerprintBank, UNFilter  # noqa: F401
