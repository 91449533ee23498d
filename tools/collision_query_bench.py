"""Throughput of the batched collision queries (SimRobot.check_collision / check_motion, csrc/query_team.h): point and motion
queries per second at M = 4096 and 65536 random configurations within the joint limits, on fr3_empty_world and -- with box poses --
on fr3_simple_pick_up, and the mix of motion results.  Prints one JSON line.
usage: python tools/collision_query_bench.py [--reps R] [--resolution RES]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "robot-control-stack_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--resolution", type=float, default=1e-3)
    args = ap.parse_args()
    from rcs_amd import sim as S
    from rcs_amd.envs import default_sim_gripper_cfg, default_sim_robot_cfg
    from rcs_amd.mjcf import compile_mjcf

    out = {"metric": "collision_queries_per_s", "resolution": args.resolution}
    for scene in ("fr3_empty_world", "fr3_simple_pick_up"):
        cfg = default_sim_robot_cfg(scene)
        simu = S.Sim(cfg.mjcf_scene_path, S.SimConfig(), n_envs=1)
        robot = S.SimRobot(simu, None, cfg)
        S.SimGripper(simu, default_sim_gripper_cfg())
        cm = compile_mjcf(cfg.mjcf_scene_path)
        nl = int(cm.nq)
        lo, hi = cm.jnt_range[:nl, 0], cm.jnt_range[:nl, 1]
        rng = np.random.default_rng(0)
        for m in (4096, 65536):
            qa = rng.uniform(lo, hi, (m, nl))
            qb = rng.uniform(lo, hi, (m, nl))
            qa[:, 7:] = qb[:, 7:] = rng.uniform(0, 0.04, (m, 1))
            boxes = None
            if scene == "fr3_simple_pick_up":
                boxes = np.zeros((m, 7))
                boxes[:, 0] = rng.uniform(0.2, 0.7, m); boxes[:, 1] = rng.uniform(-0.25, 0.25, m); boxes[:, 2] = 0.0288
                boxes[:, 3] = 1.0
            robot.check_collision(qa, boxes)  # (warm-up: module load)
            t0 = time.perf_counter()
            for _ in range(args.reps):
                robot.check_collision(qa, boxes)
            tp = (time.perf_counter() - t0) / args.reps
            robot.check_motion(qa[:64], qb[:64], resolution=args.resolution, free_qpos=None if boxes is None else boxes[:64])
            t0 = time.perf_counter()
            for _ in range(args.reps):
                res, _ = robot.check_motion(qa, qb, resolution=args.resolution, free_qpos=boxes)
            tm = (time.perf_counter() - t0) / args.reps
            key = f"{scene}_M{m}"
            out[key] = {"point_per_s": round(m / tp), "motion_per_s": round(m / tm), "point_ms": round(1e3 * tp, 3),
                        "motion_ms": round(1e3 * tm, 3), "motion_mix_free_contact_undecided": np.bincount(res, minlength=3).tolist()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
