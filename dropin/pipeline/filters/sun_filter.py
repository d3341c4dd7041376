"""The stability / uniqueness / novelty filter under the drop-in import path (configs/filter/sun.yaml)."""
from matinvent_amd.stability import PhaseBank, SUNFilter, energy_above_hull, stable_mask  # noqa: F401
