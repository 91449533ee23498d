"""Throughput of the batched dynamics derivatives (SimRobot.dynamics_derivatives, csrc/dynamics_grad_team.h): rows per second at
M = 4096 and 65536 random states within the joint limits on fr3_empty_world (9 dofs),

  * host-pointer form and device-pointer form (the latter: launch to completion, no copies),
  * every output, and dqfrc_inverse_dq + dqfrc_inverse_dqvel alone,

and, in the same process, what a caller does today for ONE of these matrices: 2 nl calls of rcsh_dynamics_query_dev asking for
qfrc_inverse at the same M -- one central-difference Jacobian -- against the device-pointer call for dqfrc_inverse_dq alone.
Warm-up, `--reps` repeats, the median with its min and max.  Prints one JSON line and writes it to --out.
usage: python tools/dynamics_derivatives_bench.py [--reps R] [--out profiles/dynamics_derivatives/bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "robot-control-stack_amd"))


def _median_s(fn, reps):
    fn()  # (warm-up: module load, staging growth)
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def _rec(m, stats):
    t, t_lo, t_hi = stats
    return {"rows_per_s": round(m / t), "ms": round(1e3 * t, 3), "ms_min_max": [round(1e3 * t_lo, 3), round(1e3 * t_hi, 3)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dynamics_derivatives", "bench.json"))
    args = ap.parse_args()
    from rcs_amd import _lib, sim as S
    from rcs_amd.envs import default_sim_gripper_cfg, default_sim_robot_cfg
    from rcs_amd.mjcf import compile_mjcf

    out = {"metric": "dynamics_derivative_rows_per_s", "scene": "fr3_empty_world", "reps": args.reps}
    cfg = default_sim_robot_cfg("fr3_empty_world")
    simu = S.Sim(cfg.mjcf_scene_path, S.SimConfig(), n_envs=1)
    robot = S.SimRobot(simu, None, cfg)
    S.SimGripper(simu, default_sim_gripper_cfg())
    cm = compile_mjcf(cfg.mjcf_scene_path)
    nl = int(cm.nq)
    lo, hi = cm.jnt_range[:nl, 0], cm.jnt_range[:nl, 1]
    rng = np.random.default_rng(0)
    L, h = simu._L, simu._h
    names = S.SimRobot.DYNAMICS_DERIVATIVES
    pair = ("dqfrc_inverse_dq", "dqfrc_inverse_dqvel")

    def alloc(nbytes):
        p = C.c_void_p()
        _lib.check(L.rcsh_dev_alloc(h, nbytes, C.byref(p)))
        return p

    def upload(a):
        a = np.ascontiguousarray(a)
        p = alloc(a.nbytes)
        _lib.check(L.rcsh_dev_upload(h, p, C.c_void_p(a.ctypes.data), a.nbytes))
        return p

    for m in (4096, 65536):
        q = rng.uniform(lo, hi, (m, nl))
        v, a, f = rng.uniform(-1, 1, (m, nl)), rng.uniform(-5, 5, (m, nl)), rng.uniform(-20, 20, (m, nl))
        dq, dv, da, df = upload(q), upload(v), upload(a), upload(f)
        mats = {k: alloc(8 * m * nl * nl) for k in names}
        vec = alloc(8 * m * nl)
        held = [dq, dv, da, df, vec, *mats.values()]

        def dev_call(want):
            o = _lib.DynamicsGradOut(**{k: mats[k].value for k in want})

            def go():
                _lib.check(L.rcsh_dynamics_derivatives_dev(h, dq, dv, da, df, m, C.byref(o)))
                simu.synchronize()
            return go

        def central_difference_calls():
            # what a caller does today for one Jacobian: 2 nl calls of the dynamics query (the perturbed rows are taken as already on
            # the device: the same rows stand in for them, the kernel's time does not depend on the values)
            o = _lib.DynamicsOut(qfrc_inverse=vec.value)
            for _ in range(2 * nl):
                _lib.check(L.rcsh_dynamics_query_dev(h, dq, dv, da, None, m, None, C.byref(o)))
            simu.synchronize()

        rec = {"host_all_outputs": _rec(m, _median_s(lambda: robot.dynamics_derivatives(q, qvel=v, qacc=a, qfrc=f), args.reps)),
               "host_inverse_pair": _rec(m, _median_s(lambda: robot.dynamics_derivatives(q, qvel=v, qacc=a, want=pair), args.reps)),
               "dev_all_outputs": _rec(m, _median_s(dev_call(names), args.reps)),
               "dev_inverse_pair": _rec(m, _median_s(dev_call(pair), args.reps)),
               "dev_dqfrc_inverse_dq": _rec(m, _median_s(dev_call(("dqfrc_inverse_dq",)), args.reps)),
               "dev_central_differences_2nl_queries": _rec(m, _median_s(central_difference_calls, args.reps))}
        rec["analytic_over_central_differences"] = round(rec["dev_dqfrc_inverse_dq"]["ms"] / rec["dev_central_differences_2nl_queries"]["ms"], 4)
        out[f"M{m}"] = rec
        for p in held:
            _lib.check(L.rcsh_dev_free(h, p))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
