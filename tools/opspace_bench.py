"""Throughput of the batched operational-space queries (SimRobot.opspace_query, csrc/opspace_team.h): rows per second at M = 4096
and 65536 random states within the joint limits on fr3_empty_world (9 dofs),

  * host-pointer form and device-pointer form (the latter: launch to completion, no copies),
  * every output, and qfrc alone,

and, in the same process, what a caller does today for the same law at the same M: dynamics_query(want = qM, qfrc_bias, jac) plus the
numpy of the impedance snippet this query replaces (invert the arm's block of qM, form Lambda, map the task force back).
Warm-up, `--reps` repeats, the median with its min and max.  Each M runs in a child process of its own under `timeout`; the first
failure ends the run.  No ratio is fixed in advance: the file records what was measured.  Prints one JSON line and writes it to --out.
usage: python tools/opspace_bench.py [--reps R] [--out profiles/opspace/bench.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "robot-control-stack_amd"))
SIZES = (4096, 65536)
STEP_TIMEOUT_S = 240


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


def one_size(m, reps):
    from rcs_amd import _lib, sim as S
    from rcs_amd.envs import default_sim_gripper_cfg, default_sim_robot_cfg
    from rcs_amd.mjcf import compile_mjcf

    cfg = default_sim_robot_cfg("fr3_empty_world")
    simu = S.Sim(cfg.mjcf_scene_path, S.SimConfig(), n_envs=1)
    robot = S.SimRobot(simu, None, cfg)
    S.SimGripper(simu, default_sim_gripper_cfg())
    cm = compile_mjcf(cfg.mjcf_scene_path)
    nl = int(cm.nq)
    lo, hi = cm.jnt_range[:nl, 0], cm.jnt_range[:nl, 1]
    rng = np.random.default_rng(0)
    L, h = simu._L, simu._h
    names = S.SimRobot.OPSPACE_OUTPUTS
    q = rng.uniform(lo, hi, (m, nl))
    v, x, f = rng.uniform(-1, 1, (m, nl)), rng.uniform(-1, 1, (m, 6)), rng.uniform(-1, 1, (m, nl))

    def upload(a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        _lib.check(L.rcsh_dev_alloc(h, a.nbytes, C.byref(p)))
        _lib.check(L.rcsh_dev_upload(h, p, C.c_void_p(a.ctypes.data), a.nbytes))
        return p

    dq, dv, dx, df = upload(q), upload(v), upload(x), upload(f)
    arrays, _ = robot._opspace_buffers(names, m, nl)
    bufs = {k: upload(a) for k, a in arrays.items()}

    def dev_call(want):
        o = _lib.OpspaceOut(**{k: bufs[k].value for k in want})

        def go():
            _lib.check(L.rcsh_opspace_query_dev(h, dq, dv, dx, df, m, None, C.byref(o)))
            simu.synchronize()
        return go

    def today():
        # the impedance law on the caller's side: the arm's block of qM inverted with the fingers frozen
        d = robot.dynamics_query(q, qvel=v, want=("qM", "qfrc_bias", "jac"))
        J = d["jac"][:, :, :7]
        Minv = np.linalg.inv(d["qM"][:, :7, :7])
        Lam = np.linalg.inv(J @ Minv @ J.transpose(0, 2, 1))
        F = np.einsum("nij,nj->ni", Lam, x)
        return np.einsum("nji,nj->ni", J, F) + d["qfrc_bias"][:, :7]

    rec = {"host_all_outputs": _rec(m, _median_s(lambda: robot.opspace_query(q, qvel=v, xacc=x, qfrc_null=f), reps)),
           "host_qfrc": _rec(m, _median_s(lambda: robot.opspace_query(q, qvel=v, xacc=x, qfrc_null=f, want=("qfrc",)), reps)),
           "dev_all_outputs": _rec(m, _median_s(dev_call(names), reps)),
           "dev_qfrc": _rec(m, _median_s(dev_call(("qfrc",)), reps)),
           "today_dynamics_query_plus_numpy": _rec(m, _median_s(today, reps))}
    status = robot.opspace_query(q, want=("status",))["status"]
    rec["rows_of_status_1"] = int(status.sum())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "opspace", "bench.json"))
    ap.add_argument("--m", type=int, default=0, help="one size, in this process (what the parent starts per size)")
    args = ap.parse_args()
    if args.m:
        print(json.dumps(one_size(args.m, args.reps)))
        return
    out = {"metric": "opspace_rows_per_s", "scene": "fr3_empty_world", "reps": args.reps}
    for m in SIZES:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--m", str(m), "--reps", str(args.reps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.exit(f"M = {m}: exit status {r.returncode}; nothing more is started")
        out[f"M{m}"] = json.loads(r.stdout.strip().splitlines()[-1])
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
