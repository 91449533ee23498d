"""Throughput of the batched swept clearance (SimRobot.swept_clearance, csrc/swept_team.h) on fr3_empty_world: rows per second, the
evaluated configurations per row and the mix of statuses at M = 4096 and 65536, for tolerances 1e-3 and 1e-4, on the random segments
tools/collision_query_bench.py uses for its motion rows (both ends uniform within the joint limits).  In the same session, on the same
rows: the motion query at the same resolution, and the clearance query on K uniformly spaced configurations per row, K = the swept
kernel's mean evals -- what a host gets for the same work with no guarantee.  Host copies included.  Prints one JSON line.
usage: python tools/swept_clearance_bench.py [--reps R] [--resolution RES] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "robot-control-stack_amd"))


def timed(fn, reps):
    """median, min and max seconds of `reps` calls after one warm call; the last result"""
    out = fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts)), float(max(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--resolution", type=float, default=1e-3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from rcs_amd import sim as S
    from rcs_amd.envs import default_sim_gripper_cfg, default_sim_robot_cfg
    from rcs_amd.mjcf import compile_mjcf

    scene = "fr3_empty_world"
    cfg = default_sim_robot_cfg(scene)
    simu = S.Sim(cfg.mjcf_scene_path, S.SimConfig(), n_envs=1)
    robot = S.SimRobot(simu, None, cfg)
    S.SimGripper(simu, default_sim_gripper_cfg())
    cm = compile_mjcf(cfg.mjcf_scene_path)
    nl = int(cm.nq)
    lo, hi = cm.jnt_range[:nl, 0], cm.jnt_range[:nl, 1]
    rng = np.random.default_rng(0)
    mask = robot.clearance_mask(3)
    out = {"metric": "swept_clearance_rows_per_s", "scene": scene, "kinds": 3, "resolution": args.resolution, "reps": args.reps}
    # warm clocks: a second of point queries before anything is timed
    warm = rng.uniform(lo, hi, (65536, nl))
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 1.0:
        robot.check_collision(warm, kinds=3)
    for m in args.sizes:
        qa = rng.uniform(lo, hi, (m, nl))
        qb = rng.uniform(lo, hi, (m, nl))
        qa[:, 7:] = qb[:, 7:] = rng.uniform(0, 0.04, (m, 1))
        rec = {}
        med, tmin, tmax, (res, _) = timed(lambda: robot.check_motion(qa, qb, resolution=args.resolution, kinds=3), args.reps)
        rec["motion"] = {"rows_per_s": round(m / med), "ms": round(1e3 * med, 3), "ms_min_max": [round(1e3 * tmin, 3), round(1e3 * tmax, 3)],
                         "mix_free_contact_undecided": np.bincount(res, minlength=3).tolist()}
        for tol in (1e-3, 1e-4):
            med, tmin, tmax, r = timed(lambda: robot.swept_clearance(qa, qb, tolerance=tol, resolution=args.resolution, kinds=3, pair_mask=mask,
                                                                     want_grad=False), args.reps)
            k = max(int(round(float(r["evals"].mean()))), 2)
            # the same work from the host: K uniform samples per row through the clearance query, in chunks that fit the staging buffer
            rows_per_chunk = max(1, (1 << 21) // k)
            s = np.linspace(0.0, 1.0, k)

            def sampled():
                best = np.empty(m)
                for i in range(0, m, rows_per_chunk):
                    a, b = qa[i:i + rows_per_chunk], qb[i:i + rows_per_chunk]
                    q = (a[:, None, :] + s[None, :, None] * (b - a)[:, None, :]).reshape(-1, nl)
                    d = robot.check_clearance(q, kinds=3, pair_mask=mask, want_grad=False)[0]
                    best[i:i + rows_per_chunk] = d.reshape(len(a), k).min(axis=1)
                return best
            smed, smin, smax, dense = timed(sampled, max(1, args.reps // 2))
            apart = r["status"] != 2
            rec[f"tol_{tol:g}"] = {
                "rows_per_s": round(m / med), "ms": round(1e3 * med, 3), "ms_min_max": [round(1e3 * tmin, 3), round(1e3 * tmax, 3)],
                "evals_mean": round(float(r["evals"].mean()), 1), "evals_max": int(r["evals"].max()),
                "status_bracketed_beyond_contact_open": np.bincount(r["status"], minlength=4).tolist(),
                "sampled_clearance": {"K": k, "rows_per_s": round(m / smed), "ms": round(1e3 * smed, 3),
                                      "ms_min_max": [round(1e3 * smin, 3), round(1e3 * smax, 3)],
                                      "rows_where_sampling_missed_more_than_tolerance": int((dense[apart] > r["distance"][apart] + tol).sum()),
                                      "rows_below_the_proven_bound": int((dense[apart] < r["lower"][apart] - 1e-9).sum())}}
        out[f"M{m}"] = rec
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
