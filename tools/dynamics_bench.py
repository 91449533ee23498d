"""Throughput of the batched dynamics queries (SimRobot.dynamics_query, csrc/dynamics_team.h): rows per second at M = 4096 and 65536
random states within the joint limits on fr3_empty_world (9 dofs), once with every output (qM, qfrc_bias, gravity, qfrc_gravcomp, jac,
qfrc_inverse, qacc) and once with qM and qfrc_bias alone.  Host-pointer forms, so the copies -- 1.1 KB of qM per row among them -- are
part of every figure.  Warm-up, `--reps` repeats, the median.  Prints one JSON line and writes it to --out.
usage: python tools/dynamics_bench.py [--reps R] [--out profiles/dynamics_query/bench.json]"""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dynamics_query", "bench.json"))
    args = ap.parse_args()
    from rcs_amd import sim as S
    from rcs_amd.envs import default_sim_gripper_cfg, default_sim_robot_cfg
    from rcs_amd.mjcf import compile_mjcf

    out = {"metric": "dynamics_rows_per_s", "scene": "fr3_empty_world", "reps": args.reps}
    cfg = default_sim_robot_cfg("fr3_empty_world")
    simu = S.Sim(cfg.mjcf_scene_path, S.SimConfig(), n_envs=1)
    robot = S.SimRobot(simu, None, cfg)
    S.SimGripper(simu, default_sim_gripper_cfg())
    cm = compile_mjcf(cfg.mjcf_scene_path)
    nl = int(cm.nq)
    lo, hi = cm.jnt_range[:nl, 0], cm.jnt_range[:nl, 1]
    rng = np.random.default_rng(0)
    for m in (4096, 65536):
        q = rng.uniform(lo, hi, (m, nl))
        v, a, f = rng.uniform(-1, 1, (m, nl)), rng.uniform(-5, 5, (m, nl)), rng.uniform(-20, 20, (m, nl))
        rec = {}
        for name, call in (("all_outputs", lambda: robot.dynamics_query(q, qvel=v, qacc=a, qfrc=f)),
                           ("qM_qfrc_bias", lambda: robot.dynamics_query(q, qvel=v, want=("qM", "qfrc_bias")))):
            t, t_lo, t_hi = _median_s(call, args.reps)
            rec[name] = {"rows_per_s": round(m / t), "ms": round(1e3 * t, 3), "ms_min_max": [round(1e3 * t_lo, 3), round(1e3 * t_hi, 3)]}
        out[f"M{m}"] = rec
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
