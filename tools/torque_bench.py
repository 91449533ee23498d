"""What the substep-rate torque law costs (Sim.step_torque, csrc/torque_team.h): substeps per second at N = 4096 and 65536 environments
of fr3_empty_world made torque-actuated, 17 substeps a call, every environment on its way to a reachable target of its own,

  (a) Sim.step_torque(17) with the full-mask law, and with task_mask = 0 (the joint law),
  (b) Sim.step(17) on the same scene with the torques held: the stepping alone,
  (c) the same full-mask law composed per substep by the caller: state and pose reads, rcsh_env_dynamics_dev and two
      rcsh_env_opspace_dev launches into device buffers, the numpy between them (pose error, task acceleration, null-space torque,
      less the gravity compensation: there is no device entry point for these), rcsh_robot_set_joint_torque_dev and Sim.step(1).

A call ends in a device synchronise; the clock is the host's around it.  Warm-up, `--reps` repeats ((c): a third as many), the median with
its min and max.  Each N runs in a child process of its own under `timeout`; the first failure ends the run.  No figure is fixed in
advance; (a) / (b) is what the law phase costs, (a) against (c) is why the launch is fused.  Prints one JSON line and writes it to --out.
usage: python tools/torque_bench.py [--reps R] [--out profiles/torque_control/bench.json]"""
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
TASK_K, TASK_D, JOINT_K, JOINT_D = 100.0, 20.0, 10.0, 2.0


def _median_s(fn, reps):
    fn()  # (warm-up: module load, staging growth)
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def _rec(n, stats):
    t, t_lo, t_hi = stats
    return {"substeps_per_s": round(n * SUBSTEPS / t), "ms_per_call": round(1e3 * t, 3), "ms_min_max": [round(1e3 * t_lo, 3), round(1e3 * t_hi, 3)]}


def _quat_mul(a, b):
    ax, ay, az, aw = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    bx, by, bz, bw = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], axis=1)


def _rotvec(q_des, q_cur):
    qe = _quat_mul(q_des, q_cur * np.array([-1.0, -1.0, -1.0, 1.0]))
    sg = np.where(qe[:, 3] < 0.0, -1.0, 1.0)
    nv = np.linalg.norm(qe[:, :3], axis=1)
    f = np.where(nv > 1e-12, sg * 2.0 * np.arctan2(nv, sg * qe[:, 3]) / np.where(nv > 1e-12, nv, 1.0), 2.0 * sg)
    return f[:, None] * qe[:, :3]


def one_size(n, reps):
    from rcs_amd import _lib, envs

    venv = envs.make_vec_env(n, True, robot="fr3", torque_actuated=True, resolve_robot_contacts=False)
    simu, robot = venv.sim, venv.robot
    L, h = simu._L, simu._h
    nl, narm = int(simu.model.nq), robot.dof
    rng = np.random.default_rng(0)
    home = simu.qpos[0].copy()
    home[narm:] = 0.02
    q_des = home[:narm] + rng.uniform(-0.3, 0.3, (n, narm))
    pose_des = robot.get_ik().forward(q_des)

    def start():
        q0 = np.tile(home, (n, 1))
        q0[:, :narm] += rng.uniform(-0.1, 0.1, (n, narm))
        simu.set_qpos(q0)
        simu.set_qvel(np.zeros((n, nl)))
        venv.gripper.set_normalized_width(np.full(n, 0.5))
        robot.set_joint_torque(np.zeros((n, narm)))
        robot.set_torque_target(pose=pose_des, q=q_des)

    def fused(mask):
        robot.configure_torque_law(TASK_K, TASK_D, JOINT_K, JOINT_D, task_mask=mask)
        return lambda: simu.step_torque(SUBSTEPS)

    def alloc(count, dtype=np.float64):
        p = C.c_void_p()
        _lib.check(L.rcsh_dev_alloc(h, count * np.dtype(dtype).itemsize, C.byref(p)))
        return p

    d_bias, d_gc, d_tw, d_xacc, d_null, d_qfrc, d_tau = alloc(n * nl), alloc(n * nl), alloc(n * 6), alloc(n * 6), alloc(n * nl), alloc(n * nl), alloc(n * narm)
    bias, gc, tw, qfrc = np.zeros((n, nl)), np.zeros((n, nl)), np.zeros((n, 6)), np.zeros((n, nl))
    dyn_out = _lib.DynamicsOut(qfrc_bias=d_bias.value, qfrc_gravcomp=d_gc.value)
    tw_out = _lib.OpspaceOut(twist=d_tw.value)
    qf_out = _lib.OpspaceOut(qfrc=d_qfrc.value)
    opts = _lib.OpspaceOpts(tcp_offset7=None, task_mask=0x3F, damping=0.0)

    def down(dst, src):
        _lib.check(L.rcsh_dev_download(h, C.c_void_p(dst.ctypes.data), src, dst.nbytes))

    def up(dst, src):
        src = np.ascontiguousarray(src)
        _lib.check(L.rcsh_dev_upload(h, dst, C.c_void_p(src.ctypes.data), src.nbytes))

    def composed():
        for _ in range(SUBSTEPS):
            q, v = simu.qpos, simu.qvel
            pose = robot.get_ik().forward(q[:, :narm])
            _lib.check(L.rcsh_env_dynamics_dev(h, None, None, None, C.byref(dyn_out)))
            _lib.check(L.rcsh_env_opspace_dev(h, None, None, C.byref(opts), C.byref(tw_out)))
            down(bias, d_bias); down(gc, d_gc); down(tw, d_tw)
            x_err = np.concatenate([pose_des[:, :3] - pose[:, :3], _rotvec(pose_des[:, 3:], pose[:, 3:])], axis=1)
            null = bias.copy()
            null[:, :narm] += JOINT_K * (q_des - q[:, :narm]) - JOINT_D * v[:, :narm]
            up(d_xacc, TASK_K * x_err - TASK_D * tw); up(d_null, null)
            _lib.check(L.rcsh_env_opspace_dev(h, d_xacc, d_null, C.byref(opts), C.byref(qf_out)))
            down(qfrc, d_qfrc)
            up(d_tau, (qfrc - gc)[:, :narm])
            _lib.check(L.rcsh_robot_set_joint_torque_dev(h, d_tau, None))
            simu.step(1)

    rec = {}
    start()
    rec["a_step_torque_full_mask"] = _rec(n, _median_s(fused(0x3F), reps))
    start()
    rec["a_step_torque_joint_law"] = _rec(n, _median_s(fused(0), reps))
    start()
    rec["b_step_torques_held"] = _rec(n, _median_s(lambda: simu.step(SUBSTEPS), reps))
    start()
    rec["c_composed_per_substep"] = _rec(n, _median_s(composed, max(reps // 3, 1)))
    rec["a_over_b_full_mask"] = round(rec["a_step_torque_full_mask"]["ms_per_call"] / rec["b_step_torques_held"]["ms_per_call"], 3)
    rec["a_over_b_joint_law"] = round(rec["a_step_torque_joint_law"]["ms_per_call"] / rec["b_step_torques_held"]["ms_per_call"], 3)
    rec["c_over_a_full_mask"] = round(rec["c_composed_per_substep"]["ms_per_call"] / rec["a_step_torque_full_mask"]["ms_per_call"], 1)
    rec["singular_environments"] = int(robot.torque_status().sum())
    assert np.isfinite(simu.qpos).all()
    venv.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "torque_control", "bench.json"))
    ap.add_argument("--n", type=int, default=0, help="one size, in this process (what the parent starts per size)")
    args = ap.parse_args()
    if args.n:
        print(json.dumps(one_size(args.n, args.reps)))
        return
    out = {"metric": "torque_substeps_per_s", "scene": "fr3_empty_world (torque-actuated variant)", "substeps_per_call": SUBSTEPS, "reps": args.reps}
    for n in SIZES:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--n", str(n), "--reps", str(args.reps)]
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
