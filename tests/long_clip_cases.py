"""Cases shared by tests/test_long_clip_ref.py (CPU) and tests/test_long_clip_gpu.py: trajectory attention over MORE than 32 key-frames (the
table route, vmg_ltam_fwd_tab / _bwd_tab) and recurrences of more than 64 steps.  Plain module; the case form, the inputs, the fp64 reference
and the per-element bounds are those of tests/traj_cases.py.

Bound beyond 32 key-frames: traj_cases.bound(...) * t / 32.  KAPPA is four times the worst ratio measured with at most 32 key-frames; the rounding
error of a sum of 4t terms (the softmax denominator, P V, the gradients' sums over keys) and of the probabilities that depend on it grows at most in
proportion to the number of terms."""
from tests import traj_cases as TC

LTAM_LONG = [
    TC.Ltam("8x8-c16-t33-frac", 1, 8, 8, 16, 2, 2, 33, "frac"),
    TC.Ltam("16x8-c32-t40-int", 2, 16, 8, 32, 2, 2, 40, "int"),
    TC.Ltam("10x12-c112-t34-frac", 1, 10, 12, 112, 2, 2, 34, "frac"),
    TC.Ltam("8x8-c144-t67-int", 1, 8, 8, 144, 2, 2, 67, "int"),
    TC.Ltam("16x8-c16-w4x2-t35-frac", 1, 16, 8, 16, 4, 2, 35, "frac"),
]
LTAM_LONG_BY_ID = {g.id: g for g in LTAM_LONG}

# the cases of tests/traj_cases.py on which the table route must give the argument route's bits (t <= 32)
ROUTE_EQUALITY = ["8x8-c32-t2-int", "10x12-c112-t7-frac", "16x8-c16-t17-int", "8x8-c16-t32-frac", "18x6-c144-t2-oneframe-out", "16x8-c16-w4x2-t7-frac"]

# step tensors: (n, t) around the 64-step limit of one launch and past two ranges
STEP_SHAPES = [(1, 64), (2, 65), (1, 100), (2, 129)]

# Trajectory_multi_head(32, 2, s, 4, True, 0.1, (2, 2)): (n, T, h, w, s)
MODULE_SHAPES = [(1, 67, 16, 16, 2), (2, 100, 8, 8, 3), (1, 65, 8, 8, 3)]


def factor(g):
    """What traj_cases.bound is multiplied by for a case of g.t key-frames."""
    return max(1.0, g.t / 32.0)


def key_frames(T, s):
    """Key-frames the recurrence has built when its last step attends: steps 0, s, 2s, ... below T."""
    return (T - 1) // s + 1
