from .simple_reacher import SimpleReacherEnv, SimpleReacherMPWrapper, sample_simple_reacher_starts  # noqa: F401
from .hole_reacher import HoleReacherEnv, HoleReacherMPWrapper, sample_hole_reacher_starts  # noqa: F401
