"""The relaxation on a learned energy under the drop-in import path (configs/relax/surrogate.yaml): the callable the reference's
sample_cfg.mlip_opt names, built from a predictor directory."""
from matinvent_amd.relax import Relaxer, relax_records, relax_state  # noqa: F401


class SurrogateRelaxer(Relaxer):
    """relax.Relaxer on the predictor saved in `model_path` (predictor.save_predictor; models/final of a pipeline=predictor run)."""

    def __init__(self, model_path=None, task=None, device=None, **kwargs):
        if not model_path or not task:
            raise ValueError("relax=surrogate needs sample_cfg.mlip_opt.model_path (a directory written by save_predictor) and task")
        from matinvent_amd.predictor import load_predictor
        from matinvent_amd.suite import get_device
        super().__init__(load_predictor(str(model_path), device=get_device(device)), str(task), **kwargs)
