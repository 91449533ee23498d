"""Cost of the env layer's collision guard (VecSimEnv.configure_guard, csrc/guard_team.h): 4096 FR3 environments in JOINTS mode,
relative to the last step, 5-degree actions around home, hands open -- resident steps (step_dev) with and without the guard, and
the guard kernel alone (back-to-back peeks on device buffers).  Prints one JSON line.
usage: python tools/collision_guard_bench.py [--n N] [--steps K] [--warmup W]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "robot-control-stack_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    args = ap.parse_args()
    from rcs_amd import _lib
    from rcs_amd.envs import MAX_JOINT_MOV, make_vec_env

    n = args.n
    rng = np.random.default_rng(0)
    # +-5 degrees per joint as the headline benchmark draws them, but every four draws are followed by their negatives: the arms stay
    # near home instead of walking a radian away over the run; hands open
    acts = []
    for _ in range(8):
        four = [np.ascontiguousarray((rng.random((n, 7)) * 2 - 1) * MAX_JOINT_MOV) for _ in range(4)]
        acts += four + [np.ascontiguousarray(-a) for a in four]
    grip = np.ones(n, dtype=np.float32)
    out = {"metric": "collision_guard_ms_per_step", "n_envs": n, "steps": args.steps, "mode": "JOINTS, LAST_STEP, async 30 Hz"}
    for guard in (False, True):
        venv = make_vec_env(n, True)
        L, h = venv._L, venv.sim._h

        def dalloc(nbytes):
            p = C.c_void_p()
            _lib.check(L.rcsh_dev_alloc(h, nbytes, C.byref(p)))
            return p

        d_act = [dalloc(n * 7 * 8) for _ in acts]
        for p, a in zip(d_act, acts):
            _lib.check(L.rcsh_dev_upload(h, p, C.c_void_p(a.ctypes.data), a.nbytes))
        d_grip, d_obs, d_info = dalloc(n * 4), dalloc(n * venv.obs_width * 8), dalloc(n * 8)
        _lib.check(L.rcsh_dev_upload(h, d_grip, C.c_void_p(grip.ctypes.data), grip.nbytes))
        venv.reset()
        step = lambda t: venv.step_dev(d_act[t % 64].value, d_grip.value, d_obs.value, d_info.value)  # noqa: E731
        for t in range(args.warmup):  # (the hands open: closed pads touch at a gap of exactly 0, which nothing certifies)
            step(t)
        if guard:
            venv.configure_guard()
        for t in range(args.warmup):
            step(t)
        venv.sim.synchronize()
        t0 = time.perf_counter()
        for t in range(args.steps):
            step(t)
        venv.sim.synchronize()
        ms = 1e3 * (time.perf_counter() - t0) / args.steps
        out["guarded_ms_per_step" if guard else "unguarded_ms_per_step"] = round(ms, 4)
        if guard:
            blocked, result, _ = venv.guard_last()
            out["last_step_results_free_contact_undecided"] = np.bincount(result, minlength=3).tolist()
            # (an open finger rests ON its joint limit and the soft limit lets it overshoot by micrometres: beyond the stroke the levers
            # were built for a segment is never certified -- query_team.h -- so such an environment is undecided)
            rng_hi = np.asarray(venv.sim.model.jnt_range)[7:9, 1]
            beyond = (venv.sim.qpos[:, 7:9] > rng_hi).any(axis=1)
            out["undecided_with_a_finger_beyond_its_stroke"] = int((beyond & (result == 2)).sum())
            out["fingers_beyond_stroke"] = int(beyond.sum())
            out["max_finger_overshoot_m"] = float((venv.sim.qpos[:, 7:9] - rng_hi).max())
            d_res, d_tc, d_blk = dalloc(n * 4), dalloc(n * 8), dalloc(n)
            peek = lambda t: _lib.check(L.rcsh_env_guard_peek_dev(h, d_act[t % 64], d_res, d_tc, d_blk))  # noqa: E731
            for t in range(10):
                peek(t)
            venv.sim.synchronize()
            t0 = time.perf_counter()
            for t in range(args.steps):
                peek(t)
            venv.sim.synchronize()
            out["guard_kernel_ms"] = round(1e3 * (time.perf_counter() - t0) / args.steps, 4)
        venv.close()
    out["guard_cost_ms_per_step"] = round(out["guarded_ms_per_step"] - out["unguarded_ms_per_step"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
