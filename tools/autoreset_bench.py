"""What autoreset inside the fused env step costs (VecSimEnv.configure_autoreset, csrc/episode_team.h): 4096 environments in the
headline configuration (FR3 + hand, JOINTS, relative to the last step, async 30 Hz, contacts resolved environment by environment),
or with --task pick_up the pick-up task env (Cartesian delta actions).  Three resident loops of equal length:
  (a) plain step_dev;
  (b) autoreset enabled with a time limit longer than the run: nobody ends, the cost is k_episode_end + the empty reset launch(es);
  (c) a time limit of 50 steps with staggered starts, against the manual loop on the same build: step_dev, download of info, numpy
      mask, upload, reset_dev.
Writes the figures (ms per step) under the task's key into --out (default profiles/autoreset_bench.json) and prints them as one JSON line.
usage: python tools/autoreset_bench.py [--task pick_up] [--n N] [--steps K] [--warmup W] [--commit HASH] [--out FILE]"""
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

LIMIT = 50


def make_env(task, n):
    if task == "pick_up":
        from rcs_amd.envs.creators import FR3SimplePickUpSimEnvCreator

        return FR3SimplePickUpSimEnvCreator()(n_envs=n)
    from rcs_amd.envs import make_vec_env

    return make_vec_env(n, True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default="headline", choices=["headline", "pick_up"])
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "autoreset_bench.json"))
    args = ap.parse_args()
    from rcs_amd import _lib
    from rcs_amd.envs import MAX_JOINT_MOV

    n, task = args.n, args.task == "pick_up"
    rng = np.random.default_rng(0)
    probe = make_env(args.task, 4)
    aw = probe.action_width
    probe.close()
    # actions as the headline benchmark draws them, every four followed by their negatives: the arms stay near where they start
    scale = np.array([0.01, 0.01, 0.01, 0, 0, 0]) if task else np.full(aw, MAX_JOINT_MOV)
    acts = []
    for _ in range(8):
        four = [np.ascontiguousarray((rng.random((n, aw)) * 2 - 1) * scale) for _ in range(4)]
        acts += four + [np.ascontiguousarray(-a) for a in four]
    grip = np.ones(n, dtype=np.float32)
    stagger = np.arange(n) % LIMIT

    def run(mode):
        """ms per step of one loop; mode: plain | idle (autoreset, nobody ends) | autoreset (limit 50) | manual (limit 50 by hand)"""
        venv = make_env(args.task, n)
        L, h = venv._L, venv.sim._h

        def dalloc(nbytes):
            p = C.c_void_p()
            _lib.check(L.rcsh_dev_alloc(h, nbytes, C.byref(p)))
            return p

        d_act = [dalloc(n * aw * 8) for _ in acts]
        for p, a in zip(d_act, acts):
            _lib.check(L.rcsh_dev_upload(h, p, C.c_void_p(a.ctypes.data), a.nbytes))
        d_grip, d_obs, d_info, d_gw, d_task, d_mask, d_rinfo = (dalloc(n * 4), dalloc(n * venv.obs_width * 8), dalloc(n * 8), dalloc(n * 8),
                                                               dalloc(n * 9 * 8), dalloc(n), dalloc(n * 8))
        _lib.check(L.rcsh_dev_upload(h, d_grip, C.c_void_p(grip.ctypes.data), grip.nbytes))
        venv.reset()
        if task:
            step = lambda t: venv.step_task_dev(d_act[t % 64].value, d_grip.value, d_obs.value, d_info.value, d_gw.value, None, d_task.value)  # noqa: E731
        else:
            step = lambda t: venv.step_dev(d_act[t % 64].value, d_grip.value, d_obs.value, d_info.value, d_gw.value)  # noqa: E731
        for t in range(args.warmup):
            step(t)
        ended = 0
        if mode == "idle":
            venv.configure_autoreset(max_episode_steps=10 * (args.steps + LIMIT))
        if mode == "autoreset":
            venv.configure_autoreset(max_episode_steps=LIMIT)
            for k in range(LIMIT):  # staggered starts: environment e begins its episode at warm-up step e % 50
                step(k)
                venv.reset(mask=stagger == k)
        elapsed = (LIMIT - 1 - stagger).astype(np.int64)  # (manual: the same stagger)
        info = np.zeros((n, 8), dtype=np.uint8)
        task_rows = np.zeros((n, 9))
        box = np.zeros((n, 7))
        d_box = dalloc(n * 7 * 8)
        venv.sim.synchronize()
        t0 = time.perf_counter()
        for t in range(args.steps):
            step(t)
            if mode == "manual":
                _lib.check(L.rcsh_dev_download(h, C.c_void_p(info.ctypes.data), d_info, info.nbytes))
                elapsed += 1
                done = (info[:, 4] != 0) | (elapsed >= LIMIT)
                if task:
                    _lib.check(L.rcsh_dev_download(h, C.c_void_p(task_rows.ctypes.data), d_task, task_rows.nbytes))
                    done |= task_rows[:, 8] != 0
                elapsed[done] = 0
                ended += int(done.sum())
                m = done.astype(np.uint8)
                _lib.check(L.rcsh_dev_upload(h, d_mask, C.c_void_p(m.ctypes.data), m.nbytes))
                if task:
                    box[:] = venv.draw_box_qpos()  # (the Python loop over N the env's explicit reset runs)
                    _lib.check(L.rcsh_dev_upload(h, d_box, C.c_void_p(box.ctypes.data), box.nbytes))
                    venv.reset_task_dev(d_box.value, d_obs.value, d_rinfo.value, d_gw.value, d_mask.value)
                else:
                    venv.reset_dev(d_obs.value, d_rinfo.value, d_gw.value, d_mask.value)
        venv.sim.synchronize()
        ms = 1e3 * (time.perf_counter() - t0) / args.steps
        if mode in ("idle", "autoreset"):
            ended = int(venv.autoreset_last(("episodes",))["episodes"].sum())
        venv.close()
        return round(ms, 4), ended

    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
        except Exception:
            commit = "unknown"
    res = {"metric": "ms_per_env_step", "n_envs": n, "steps": args.steps, "time_limit_of_c": LIMIT, "commit": commit}
    res["a_plain_step_dev"], _ = run("plain")
    res["b_autoreset_nobody_ends"], res["b_episodes_ended"] = run("idle")
    res["c_autoreset_limit_50"], res["c_autoreset_episodes_ended"] = run("autoreset")
    res["c_manual_limit_50"], res["c_manual_episodes_ended"] = run("manual")
    res["b_over_a"] = round(res["b_autoreset_nobody_ends"] / res["a_plain_step_dev"], 4)
    res["c_autoreset_over_manual"] = round(res["c_autoreset_limit_50"] / res["c_manual_limit_50"], 4)
    table = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            table = json.load(f)
    table[args.task] = res
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({args.task: res}))


if __name__ == "__main__":
    main()
