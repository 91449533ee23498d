"""dev tool: how many pairs the hull rounds of the contact phase's narrow stage refine side by side (library built with
tools/build_timing.sh), over all workgroups: rounds with 1, 2, 3 and 4 pairs for the two input sets of tests/test_gpu_wide_support.py and
for the default benchmark's rollout (4096 environments, 330 launches, seed 0).
    python tools/round_hist.py [n_envs] [n_steps]
A lone pair is refined by the whole wavefront, two pairs by 32 lanes each (csrc/contact_team.h: contact_collide)."""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "robot-control-stack_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import rcs_amd._lib as lib
lib.LIB_PATH = os.environ.get("RCSH_TIMING_LIB") or os.path.join(ROOT, "robot-control-stack_amd", "rcs_amd", "librcs_hip_timing.so")
import numpy as np
import parity_util as PU
import test_gpu_wide_support as T

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 330
out = (C.c_ulonglong * 4)()


def read():
    lib.load().rcsh_debug_round_hist(out)
    return np.array(out[:], dtype=np.int64)


base = read()
for name, fn in (("quiet rollout (10 environments, 290 launches)", lambda: T._rollout(None)), ("folded arms (24 environments, 40 launches)", lambda: T._folded_arms(None))):
    fn()
    a = read()
    print(f"{name}: rounds with 1 / 2 / 3 / 4 pairs {(a - base).tolist()}")
    base = a
venv = PU.make_vec_env(n, True)
joints, grip = PU.synthetic_actions(n, steps, 0)
venv.reset()
for t in range(steps):
    venv.step({"joints": joints[t], "gripper": grip[t]})
    if (t + 1) % 30 == 0 or t + 1 == steps:
        a = read()
        print(f"benchmark rollout ({n} environments), launches ..{t}: rounds with 1 / 2 / 3 / 4 pairs {(a - base).tolist()}")
        base = a
