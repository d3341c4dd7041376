"""memory/: the reference's import paths for the replay buffer and the long-term memory."""
from matinvent_amd.memory import LongTimeMem, ReplayBuffer  # noqa: F401
