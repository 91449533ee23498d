"""What an env step in the impedance control modes costs (rcsh_env_step_dev, csrc/env_torque_team.h) against the launches it is made
of: env-steps per second at N = 4096 and 65536 environments of fr3_empty_world made torque-actuated, 17 substeps a step,

  (a) rcsh_env_step_dev in JOINT_IMPEDANCE with task_mask = 0, resident action and output rows,
  (b) the same in CARTESIAN_IMPEDANCE_TQUAT with the full mask,
  (c) rcsh_sim_step_torque(17) with the same two laws at the default check cadence: the two launches an env step is made of,
      without the action row, the target write and the observation row.

Where a difference goes: every round also measures the env step WITHOUT its output rows (null obs / info / gripper-width / substeps
pointers: the observing pass then carries the check alone, as it does behind rcsh_sim_step_torque), so that
  no_rows - (c)  is the stepping launch's prologue (action row, wrapper arithmetic, target write), and
  (a) - no_rows  is the observation, info and gripper-width rows of the observing pass.
(a) and (c, joint law), then (b) and (c, full mask), are measured INTERLEAVED: `--rounds` rounds of one median each, alternating, in
the same process, so that the spread of (c) over the rounds is the yardstick for (a) - (c).  A call ends in a device synchronise; the
clock is the host's around it.  Actions are small relative motions drawn once; every round starts from a reset.  Each N runs in a
child process of its own under `timeout`; the first failure ends the run.  Prints one JSON line and writes it to --out.
usage: python tools/env_torque_bench.py [--reps R] [--rounds K] [--out profiles/env_torque/bench.json]"""
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
SUBSTEPS = 17
STEP_TIMEOUT_S = 280
LAW = dict(task_k=100.0, task_d=20.0, joint_k=10.0, joint_d=2.0)


def _median_s(fn, reps):
    fn()  # (warm-up)
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def _summary(n, medians):
    m = np.array(medians)
    return {"env_steps_per_s": round(n / float(np.median(m))), "ms_per_call": round(1e3 * float(np.median(m)), 4),
            "ms_rounds": [round(1e3 * float(x), 4) for x in m]}


def one_size(n, reps, rounds):
    from rcs_amd import _lib, envs
    from rcs_amd.envs import ControlMode

    rng = np.random.default_rng(0)
    rec = {}
    for name, mode, mask, width in (("joint_impedance_mask0", ControlMode.JOINT_IMPEDANCE, 0, 7),
                                    ("cartesian_impedance_tquat_full", ControlMode.CARTESIAN_IMPEDANCE_TQuat, 0x3F, 7)):
        venv = envs.make_vec_env(n, True, robot="fr3", torque_actuated=True, control_mode=mode, torque_law=dict(LAW, task_mask=mask),
                                 max_relative_movement=0.05)
        simu = venv.sim
        L, h = simu._L, simu._h
        if mode == ControlMode.JOINT_IMPEDANCE:
            act = rng.uniform(-0.05, 0.05, (n, width))
        else:
            act = np.zeros((n, width))
            act[:, :3] = rng.uniform(-0.02, 0.02, (n, 3))
            act[:, 6] = 1.0
        grip = np.ones(n, dtype=np.float32)

        def alloc(nbytes):
            p = C.c_void_p()
            _lib.check(L.rcsh_dev_alloc(h, nbytes, C.byref(p)))
            return p

        d_act, d_grip = alloc(act.nbytes), alloc(grip.nbytes)
        _lib.check(L.rcsh_dev_upload(h, d_act, C.c_void_p(act.ctypes.data), act.nbytes))
        _lib.check(L.rcsh_dev_upload(h, d_grip, C.c_void_p(grip.ctypes.data), grip.nbytes))
        d_obs, d_info, d_gw, d_sub = alloc(n * venv.obs_width * 8), alloc(n * 8), alloc(n * 8), alloc(n * 4)

        def env_step():
            venv.step_dev(d_act.value, d_grip.value, d_obs.value, d_info.value, d_gw.value, d_sub.value)
            simu.synchronize()

        def env_step_no_rows():
            venv.step_dev(d_act.value, d_grip.value, None)
            simu.synchronize()

        def law_step():
            simu.step_torque(SUBSTEPS)

        a, b, c = [], [], []
        for _ in range(rounds):
            venv.reset_dev(d_obs.value, d_info.value, d_gw.value)
            a.append(_median_s(env_step, reps))
            venv.reset_dev(d_obs.value, d_info.value, d_gw.value)
            b.append(_median_s(env_step_no_rows, reps))
            venv.reset_dev(d_obs.value, d_info.value, d_gw.value)
            c.append(_median_s(law_step, reps))
        rec[f"env_step_{name}"] = _summary(n, a)
        rec[f"env_step_no_rows_{name}"] = _summary(n, b)
        rec[f"step_torque_{name}"] = _summary(n, c)
        rec[f"prologue_ms_{name}"] = round(1e3 * (float(np.median(b)) - float(np.median(c))), 4)
        rec[f"output_rows_ms_{name}"] = round(1e3 * (float(np.median(a)) - float(np.median(b))), 4)
        spread = float(np.max(c) - np.min(c))
        rec[f"env_minus_law_ms_{name}"] = round(1e3 * (float(np.median(a)) - float(np.median(c))), 4)
        rec[f"law_spread_ms_{name}"] = round(1e3 * spread, 4)
        rec[f"singular_{name}"] = int(venv.robot.torque_status().sum())
        assert np.isfinite(simu.qpos).all()
        venv.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "env_torque", "bench.json"))
    ap.add_argument("--n", type=int, default=0, help="one size, in this process (what the parent starts per size)")
    args = ap.parse_args()
    if args.n:
        print(json.dumps(one_size(args.n, args.reps, args.rounds)))
        return
    out = {"metric": "env_steps_per_s", "scene": "fr3_empty_world (torque-actuated variant)", "substeps_per_step": SUBSTEPS, "reps": args.reps,
           "rounds": args.rounds}
    for n in SIZES:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--n", str(n), "--reps", str(args.reps),
               "--rounds", str(args.rounds)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.exit(f"N = {n}: exit status {r.returncode}; nothing more is started")
        out[f"N{n}"] = json.loads(r.stdout.strip().splitlines()[-1])
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
