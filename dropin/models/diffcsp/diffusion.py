from matinvent_amd.diffcsp import DiffCSPModule, SinusoidalTimeEmbeddings, MAX_ATOMIC_NUM, log_prob_wn, p_wrapped_normal  # noqa: F401
