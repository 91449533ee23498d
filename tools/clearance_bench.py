"""Throughput of the batched clearance queries (SimRobot.check_clearance, csrc/clearance_team.h) next to the point query on the same
rows: configurations per second at M = 4096 and 65536 random configurations within the joint limits, on fr3_empty_world (kinds = 3)
and -- with box poses -- on fr3_simple_pick_up (kinds = 7), each with d_max = inf and d_max = 0.05.  Host-pointer forms, so the copies
are part of every figure, the point query's included.  Warm-up, `--reps` repeats, the median.  Prints one JSON line.
A library without the clearance queries (an older commit) reports the point query alone.
usage: python tools/clearance_bench.py [--reps R]"""
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
    args = ap.parse_args()
    from rcs_amd import sim as S
    from rcs_amd.envs import default_sim_gripper_cfg, default_sim_robot_cfg
    from rcs_amd.mjcf import compile_mjcf

    out = {"metric": "clearance_configurations_per_s", "reps": args.reps}
    for scene, kinds in (("fr3_empty_world", 3), ("fr3_simple_pick_up", 7)):
        cfg = default_sim_robot_cfg(scene)
        simu = S.Sim(cfg.mjcf_scene_path, S.SimConfig(), n_envs=1)
        robot = S.SimRobot(simu, None, cfg)
        S.SimGripper(simu, default_sim_gripper_cfg())
        cm = compile_mjcf(cfg.mjcf_scene_path)
        nl = int(cm.nq)
        lo, hi = cm.jnt_range[:nl, 0], cm.jnt_range[:nl, 1]
        rng = np.random.default_rng(0)
        has_clearance = hasattr(robot, "check_clearance")
        for m in (4096, 65536):
            q = rng.uniform(lo, hi, (m, nl))
            q[:, 7:] = rng.uniform(0, 0.04, (m, 1))
            boxes = None
            if scene == "fr3_simple_pick_up":
                boxes = np.zeros((m, 7))
                boxes[:, 0] = rng.uniform(0.2, 0.7, m); boxes[:, 1] = rng.uniform(-0.25, 0.25, m); boxes[:, 2] = 0.0288
                boxes[:, 3] = 1.0
            tp, tp_lo, tp_hi = _median_s(lambda: robot.check_collision(q, boxes, kinds=kinds), args.reps)
            rec = {"kinds": kinds, "point_per_s": round(m / tp), "point_ms": round(1e3 * tp, 3), "point_ms_min_max": [round(1e3 * tp_lo, 3), round(1e3 * tp_hi, 3)]}
            if has_clearance:
                for name, d_max in (("inf", np.inf), ("0.05", 0.05)):
                    tc, lo_, hi_ = _median_s(lambda: robot.check_clearance(q, free_qpos=boxes, kinds=kinds, d_max=d_max), args.reps)
                    dist, status, *_ = robot.check_clearance(q, free_qpos=boxes, kinds=kinds, d_max=d_max)
                    rec[f"clearance_dmax_{name}"] = {"per_s": round(m / tc), "ms": round(1e3 * tc, 3), "ms_min_max": [round(1e3 * lo_, 3), round(1e3 * hi_, 3)],
                                                      "time_over_point_query": round(tc / tp, 2),
                                                      "status_apart_beyond_contact_open": np.bincount(status, minlength=4).tolist()}
            out[f"{scene}_M{m}"] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
