"""The torque and impedance control modes of the fused env step (csrc/env_torque_team.h) against their composition from the entry
points that existed and are held to the oracle (tests/test_gpu_torque_control.py): the wrapper arithmetic in numpy
(tests/env_torque_cases.py, itself held to the oracle's wrapper stack by tests/test_env_torque_cases_cpu.py), targets written with
set_torque_target only when the gate commands, torques with set_joint_torque, the substeps as step_torque(17) (Sim.step(17) in TORQUE
mode), a reset as gripper reset + Sim.reset + robot.reset + step_torque(1).

Bars: qpos, qvel and the law's targets 1e-9; ctrl 1e-9 of the joint's torque limit on the FR3 runs, elsewhere the amplification rule
of test_fused_law_agrees_with_its_composition -- max(1e-9 limit, 1e-13 cond(A) |tau|) with cond(A) and |tau| taken at both ends of the
env-step (the composition runs the step's seventeen substeps in one launch, so there is no substep in between to ask at); bit equality
where only adds and clamps are involved (q_des, ORIGIN / LASTA / PREVA of the joint branch) and for the observation rows against
get_cartesian_position / qpos read at the same state.  The measured worst values are printed (profiles/env_torque/tests.txt).
"""

import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import env_torque_cases as EC  # noqa: E402
import opspace_cases as OC  # noqa: E402
import torque_cases as TC  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-9
N = EC.N
WORST = {}


def _note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))


def _report(prefix):
    print("worst deviations:", {k: v for k, v in WORST.items() if k.startswith(prefix)})


def _mode(name):
    from rcs_amd.envs import ControlMode

    return {"torque": ControlMode.TORQUE, EC.JOINTS: ControlMode.JOINT_IMPEDANCE, EC.TRPY: ControlMode.CARTESIAN_IMPEDANCE_TRPY,
            EC.TQUAT: ControlMode.CARTESIAN_IMPEDANCE_TQuat}[name]


def _env(tag, mode, relative_to=EC.LAST_STEP, task_mask=0x3F, n=N, law=True, damping=0.0, **kw):
    from rcs_amd import envs

    if mode == "torque":
        law, relative_to = False, None
    law_kw = dict(EC.LAW, task_mask=task_mask, damping=damping) if law else None
    if isinstance(law, dict):
        law_kw = law
    mm = None if relative_to is None else (EC.MAX_JOINT_MOV if mode == EC.JOINTS else EC.MAX_CART_MOV)
    args = dict(robot=tag, torque_actuated=True, control_mode=_mode(mode), relative=relative_to is not None,
                relative_to=relative_to or EC.LAST_STEP, max_relative_movement=mm, torque_law=law_kw)
    if tag == "fr3" and mode in (EC.TRPY, EC.TQUAT):
        cfg = envs.factory.robot_cfg_for("fr3")
        cfg.tcp_offset = EC.fr3_tcp()  # (a TCP that is not the site: the law's offset defaults to its inverse)
        args["robot_cfg"] = cfg
    args.update(kw)
    return envs.make_vec_env(n, True, **args)


def _limits(venv):
    return np.asarray(venv._low, dtype=np.float64), np.asarray(venv._high, dtype=np.float64)


def _wrappers(venv, mode, relative_to, n):
    low, high = _limits(venv)
    mm = EC.MAX_JOINT_MOV if mode == EC.JOINTS else EC.MAX_CART_MOV
    return [EC.Wrapper(mode, relative_to, mm, low, high) for _ in range(n)]


def _current(venv, mode):
    return venv.sim.qpos[:, : venv.dof] if mode == EC.JOINTS else venv.robot.get_cartesian_position()


def _fields(venv):
    sim = venv.sim
    return EC.state_fields(sim.get_state(), venv.n_envs, sim.qpos.shape[1], sim.ctrl.shape[1], venv.dof)


def _grip_width(g):
    g = np.clip(np.round(np.asarray(g, dtype=np.float32)), 0.0, 1.0)  # GripperWrapper.action, binary (base.py:721-735)
    return np.where(g == 0.0, 0.0, 1.0), g


def _snapshot(venv):
    sim, robot = venv.sim, venv.robot
    pose, q = robot.torque_target()
    return dict(qpos=sim.qpos, qvel=sim.qvel, ctrl=sim.ctrl, time=sim.time, pose=pose, q_des=q, tcp=robot.get_cartesian_position(),
                fields=_fields(venv), singular=robot.torque_status())


def _restore(venv, blob, snap):
    """Back to a recorded state: the blob does not carry the law's targets."""
    venv.sim.set_state(blob)
    venv.robot.set_torque_target(pose=snap["pose"], q=snap["q_des"])


def _amp(venv, task_mask, ctrl):
    """cond(A) of the selected task rows times the torque's size, per environment (tests/test_gpu_torque_control.py's rule)."""
    sel = [r for r in range(6) if (task_mask >> r) & 1]
    cond = np.ones(venv.n_envs)
    if sel:
        tcp = venv.robot.get_config().tcp_offset.inverse().as_vec7()
        A = venv.opspace(want=("lambda_inv",), tcp_offset=tcp, task_mask=task_mask)["lambda_inv"][:, sel][:, :, sel]
        cond = np.linalg.cond(A)
    return cond * np.abs(ctrl[:, : venv.dof]).max(axis=1)


def _compare(key, tag, fused, ref, lim, amp=None, rows=None):
    """qpos, qvel, targets to TOL; ctrl to TOL of the limit (FR3) or the amplification rule."""
    rows = slice(None) if rows is None else rows
    na = len(lim)
    dq = float(np.abs(fused["qpos"][rows] - ref["qpos"][rows]).max())
    dv = float(np.abs(fused["qvel"][rows] - ref["qvel"][rows]).max())
    err = np.abs(fused["ctrl"][rows][:, :na] - ref["ctrl"][rows][:, :na])
    dc = float((err / lim).max())
    dp = float(np.abs(fused["pose"][rows][:, :3] - ref["pose"][rows][:, :3]).max())
    dr = float(np.abs(TC.rotvec(fused["pose"][rows][:, 3:], ref["pose"][rows][:, 3:])).max())
    dd = float(np.abs(fused["q_des"][rows] - ref["q_des"][rows]).max())
    for name, v in (("qpos", dq), ("qvel", dv), ("ctrl_over_limit", dc), ("target_pos", dp), ("target_rot", dr), ("q_des", dd)):
        _note(f"{key}/{name}", v)
    assert dq < TOL and dv < TOL and dp < TOL and dr < TOL and dd < TOL, (key, dq, dv, dp, dr, dd)
    if tag == "fr3" or amp is None:
        assert dc < TOL, (key, dc)
    else:
        bar = np.maximum(TOL * lim[None, :], (1e-13 * amp[rows])[:, None])
        _note(f"{key}/ctrl_over_bar", float((err / bar).max()))
        assert (err < bar).all(), (key, float((err / bar).max()), dc)
    assert np.array_equal(fused["ctrl"][rows][:, na:], ref["ctrl"][rows][:, na:])  # (the gripper's ctrl: one product and one sum)
    assert np.array_equal(fused["time"][rows], ref["time"][rows])


def _obs_is_the_state(venv, o):
    """The observing pass: the rows are what get_cartesian_position / qpos give at the same state, bit for bit."""
    assert np.array_equal(o["tquat"], venv.robot.get_cartesian_position())
    assert np.array_equal(o["joints"], venv.sim.qpos[:, : venv.dof])


def _compose_step(venv, mode, wrappers, a, g, task_mask, margins):
    """One env step from the entry points that existed.  Returns what the wrappers decided."""
    sim, robot = venv.sim, venv.robot
    n = venv.n_envs
    cur = _current(venv, mode)
    out, cmd = [], np.zeros(n, dtype=bool)
    for e in range(n):
        o, c, m = wrappers[e].action(a[e], cur[e])
        out.append(o)
        cmd[e] = c
        margins.append(m)
    out = np.array(out)
    if cmd.any():
        if mode == EC.JOINTS:
            robot.set_torque_target(q=out, mask=cmd)
        else:
            robot.set_torque_target(pose=np.array([w.target7(o) for w, o in zip(wrappers, out)]), mask=cmd)
    if venv.gripper is not None:
        venv.gripper.set_normalized_width(_grip_width(g)[0])
    amp0 = _amp(venv, task_mask, sim.ctrl)
    sim.step_torque(EC.SUBSTEPS)
    return out, cmd, np.maximum(amp0, _amp(venv, task_mask, sim.ctrl))


def _run_impedance(tag, mode, task_mask, relative_to, actions):
    key = f"{mode}/{tag}/{task_mask:#x}/{relative_to}"
    venv = _env(tag, mode, relative_to, task_mask)
    sim, robot = venv.sim, venv.robot
    lim = np.array(TC.RANGES[tag])
    grips = EC.gripper_actions(len(actions))
    dof = venv.dof
    o, _ = venv.reset()
    _obs_is_the_state(venv, o)
    blob, start = sim.get_state(), _snapshot(venv)
    fused = []
    for k, a in enumerate(actions):
        act = {venv.action_key: a}
        if venv.gripper is not None:
            act["gripper"] = grips[k]
        o, _, _, _, info = venv.step(act)
        assert (info["substeps"] == EC.SUBSTEPS).all() and not info["torque_singular"].any()
        _obs_is_the_state(venv, o)
        if venv.gripper is not None:
            assert np.array_equal(o["gripper"], _grip_width(grips[k])[1])
        fused.append(_snapshot(venv))
    moved = float(np.abs(fused[-1]["qpos"] - start["qpos"]).max())
    assert moved > 1e-3  # (the law moved the arm: not a comparison of two arms at rest)
    # ---- the composition, from the same start
    _restore(venv, blob, start)
    wrappers = _wrappers(venv, mode, relative_to, N)
    cur = _current(venv, mode)
    for e, w in enumerate(wrappers):
        w.reset(cur[e])
    margins, held, clamped, boxed, limited = [], 0, 0, 0, 0
    low, high = _limits(venv)
    for k, a in enumerate(actions):
        before = robot.torque_target()
        out, cmd, amp = _compose_step(venv, mode, wrappers, a, grips[k], task_mask, margins)
        ref = _snapshot(venv)
        _compare(key, tag, fused[k], ref, lim, amp)
        f = fused[k]["fields"]
        if mode == EC.JOINTS:
            # adds and clamps: bit for bit
            assert np.array_equal(fused[k]["q_des"], ref["q_des"]), (key, k)
            assert np.array_equal(f["preva"][:, :dof], out), (key, k)
            if relative_to is not None:
                assert np.array_equal(f["origin"][:, :dof], np.array([w.origin for w in wrappers])), (key, k)
                assert np.array_equal(f["lasta"][:, :dof], np.array([w.last for w in wrappers])), (key, k)
                clamped += int(((out == low) | (out == high)).any())
        else:
            w7 = out.shape[1]
            _note(f"{key}/preva", np.abs(f["preva"][:, :w7] - out).max())
            assert np.abs(f["preva"][:, :w7] - out).max() < TOL
            org = np.array([w.origin.as_vec7() for w in wrappers])
            last = np.array([w.last.as_vec7() for w in wrappers])
            assert np.abs(f["origin"][:, :3] - org[:, :3]).max() < TOL and np.abs(TC.rotvec(f["origin"][:, 3:], org[:, 3:])).max() < TOL
            assert np.abs(f["lasta"][:, :3] - last[:, :3]).max() < TOL and np.abs(TC.rotvec(f["lasta"][:, 3:], last[:, 3:])).max() < TOL
            boxed += int((out[:, 2] == 0.0).any())
            limited += int(any(abs(w.last.total_angle() - EC.MAX_CART_MOV[1]) < 1e-9 for w in wrappers))
        # a gated-out action leaves the law's targets as they were, bit for bit
        if (~cmd).any():
            held += int((~cmd).sum())
            assert np.array_equal(fused[k]["pose"][~cmd], (fused[k - 1] if k else start)["pose"][~cmd])
            assert np.array_equal(fused[k]["q_des"][~cmd], (fused[k - 1] if k else start)["q_des"][~cmd])
            assert np.array_equal(before[0][~cmd], ref["pose"][~cmd]) and np.array_equal(before[1][~cmd], ref["q_des"][~cmd])
        # nothing of the position servo's bookkeeping
        st = robot.get_state()
        assert not st.is_moving.any()
    print(key, "smallest gate margin", min(margins), "held", held, "clamped steps", clamped, "box steps", boxed, "rotation-limit steps", limited,
          "moved", moved)
    assert min(margins) >= EC.GATE_MARGIN, (key, min(margins))
    if relative_to != EC.LAST_STEP:
        assert held >= N  # (the repeated action)
    if mode == EC.JOINTS and relative_to is not None:
        assert clamped >= 1
    if mode != EC.JOINTS:
        assert boxed >= 1 and limited >= 1  # (the workspace box was reached, the rotation limit bit, on the simulated states)
    _report(key)
    venv.close()


# ---- 1. TORQUE
@pytest.mark.parametrize("tag", EC.TORQUE_RUNS)
def test_torque_mode_is_set_joint_torque_and_seventeen_substeps(tag):
    q0, taus = EC.torque_actions(tag)
    venv = _env(tag, "torque")
    sim, robot = venv.sim, venv.robot
    lim = np.array(TC.RANGES[tag])
    grips = EC.gripper_actions(len(taus))
    sim.set_qpos(q0)
    sim.set_qvel(np.zeros_like(q0))
    if venv.gripper is not None:
        venv.gripper.set_normalized_width(np.full(N, 0.5))
    robot.set_joint_torque(np.zeros((N, venv.dof)))
    blob, start = sim.get_state(), _snapshot(venv)
    fused = []
    for k, tau in enumerate(taus):
        act = {"torque": tau}
        if venv.gripper is not None:
            act["gripper"] = grips[k]
        o, _, _, _, info = venv.step(act)
        assert (info["substeps"] == EC.SUBSTEPS).all() and not info["torque_singular"].any()
        _obs_is_the_state(venv, o)
        assert np.array_equal(sim.ctrl[:, : venv.dof], tau)  # (ctrl is the action; the clamp acts on the force)
        fused.append(_snapshot(venv))
    assert (np.abs(taus[0][1]) > lim).sum() == 2
    _restore(venv, blob, start)
    for k, tau in enumerate(taus):
        robot.set_joint_torque(tau)
        if venv.gripper is not None:
            venv.gripper.set_normalized_width(_grip_width(grips[k])[0])
        sim.step(EC.SUBSTEPS)
        _compare(f"torque/{tag}", "fr3", fused[k], _snapshot(venv), lim)
        assert np.array_equal(fused[k]["pose"], start["pose"]) and np.array_equal(fused[k]["q_des"], start["q_des"])  # (no law, no target)
    _report(f"torque/{tag}")
    venv.close()


# ---- 2. JOINT_IMPEDANCE
@pytest.mark.parametrize("tag,task_mask,relative_to", EC.JOINT_RUNS)
def test_joint_impedance_agrees_with_its_composition(tag, task_mask, relative_to):
    r = TC.oracle_robot(tag)
    _run_impedance(tag, EC.JOINTS, task_mask, relative_to, EC.joint_actions(r["q_home"], r["low"], r["high"], relative_to))


# ---- 3. CARTESIAN_IMPEDANCE
@pytest.mark.parametrize("tag,mode,task_mask,relative_to", EC.CART_RUNS)
def test_cartesian_impedance_agrees_with_its_composition(tag, mode, task_mask, relative_to):
    _run_impedance(tag, mode, task_mask, relative_to, EC.cart_actions(mode))


# ---- 4. reset
def _compose_reset(venv, mask):
    sim, robot = venv.sim, venv.robot
    if venv.gripper is not None:
        venv.gripper.reset(mask)  # (before Sim.reset, which overwrites what it wrote to qpos / ctrl: quirk Q1)
    sim.reset(mask)
    robot.reset(mask)
    sim.step_torque(1)  # (every environment steps: only the masked rows are compared)


@pytest.mark.parametrize("tag,mode,relative_to", [("fr3", EC.JOINTS, EC.CONFIGURED_ORIGIN), ("fr3", EC.TQUAT, EC.LAST_STEP),
                                                  ("fr3", "torque", None), ("xarm7", EC.JOINTS, EC.LAST_STEP)])
def test_reset_whole_batch_and_masked_against_the_composition(tag, mode, relative_to):
    key = f"reset/{mode}/{tag}"
    venv = _env(tag, mode, relative_to, 0x3F if tag == "fr3" else 0)
    sim, robot = venv.sim, venv.robot
    lim = np.array(TC.RANGES[tag])
    dof = venv.dof
    home = np.asarray(TC.oracle_robot(tag)["q_home"], dtype=np.float64)
    if mode == "torque":
        acts = [0.2 * lim * EC.signs(dof, 3), -0.1 * lim * EC.signs(dof, 4)]
    elif mode == EC.JOINTS:
        r = TC.oracle_robot(tag)
        acts = EC.joint_actions(r["q_home"], r["low"], r["high"], relative_to)[:2]
    else:
        acts = EC.cart_actions(mode)[:2]
    grips = EC.gripper_actions(4)
    wrappers = _wrappers(venv, mode, relative_to, N) if mode != "torque" else None
    margins = []

    def step(k, a):
        act = {venv.action_key: a}
        if venv.gripper is not None:
            act["gripper"] = grips[k]
        return venv.step(act)

    def check_reset(mask, o):
        rows = np.ones(N, dtype=bool) if mask is None else mask
        after = _snapshot(venv)
        _obs_is_the_state(venv, o)
        f = after["fields"]
        if relative_to is not None:  # the origin: the state after the reset's substep
            if mode == EC.JOINTS:
                assert np.array_equal(f["origin"][rows][:, :dof], after["qpos"][rows][:, :dof])
            else:
                assert np.abs(f["origin"][rows] - after["tcp"][rows]).max() < 1e-12
        assert np.array_equal(after["q_des"][rows], np.tile(home, (int(rows.sum()), 1)))
        if mode == "torque":
            assert not after["ctrl"][rows].any()  # (zero torque, never q_home)
        else:
            assert np.abs(after["ctrl"][rows][:, :dof] - home).max() > 1e-3 and after["ctrl"][rows][:, :dof].any()
        assert not after["singular"].any()
        return after

    # whole batch, from a state the steps have moved
    o, _ = venv.reset()
    step(0, acts[0])
    step(1, acts[1])
    blob, pre = sim.get_state(), _snapshot(venv)
    o, _ = venv.reset()
    whole = check_reset(None, o)
    _restore(venv, blob, pre)
    _compose_reset(venv, None)
    _compare(key + "/whole", tag, whole, _snapshot(venv), lim)
    # masked, and the steps after it (kHasLastAction cleared, PREVA kept: the wrappers of the composition do the same)
    mask = np.arange(N) % 2 == 0
    _restore(venv, blob, pre)
    o, _ = venv.reset(mask=mask)
    part = check_reset(mask, o)
    for name in ("qpos", "qvel", "ctrl", "time", "pose", "q_des"):
        assert np.array_equal(part[name][~mask], pre[name][~mask]), name  # (a zero byte sits the environment out)
    for name in ("preva", "origin", "lasta"):
        assert np.array_equal(part["fields"][name][~mask], pre["fields"][name][~mask]), name
    assert np.array_equal(part["fields"]["preva"], pre["fields"]["preva"])  # (PREVA survives a reset: the reference's quirk)
    blob2 = sim.get_state()
    fused_next = []
    for k in (2, 3):
        step(k, acts[1])
        fused_next.append(_snapshot(venv))
    _restore(venv, blob, pre)
    _compose_reset(venv, None)
    _compare(key + "/masked", tag, part, _snapshot(venv), lim, rows=mask)
    if mode != "torque":
        # the two steps after the masked reset, composed from the state it left
        sim.set_state(blob2)  # (the targets follow)
        robot.set_torque_target(pose=part["pose"], q=part["q_des"])
        for e, w in enumerate(wrappers):  # the wrappers as two steps and a masked reset leave them: read from the state
            w.prev = part["fields"]["preva"][e][: (dof if mode == EC.JOINTS else 7)].copy()
            if relative_to is not None:
                org, last = part["fields"]["origin"][e], part["fields"]["lasta"][e]
                if mode == EC.JOINTS:
                    w.origin, w.last = org[:dof].copy(), (None if mask[e] else last[:dof].copy())
                else:
                    from rcs_amd.common import Pose

                    w.origin = Pose(translation=org[:3], quaternion=org[3:])
                    w.last = None if mask[e] else Pose(translation=last[:3], quaternion=last[3:])
        for i, k in enumerate((2, 3)):
            _, _, amp = _compose_step(venv, mode, wrappers, acts[1], grips[k], 0x3F if tag == "fr3" else 0, margins)
            _compare(key + "/after", tag, fused_next[i], _snapshot(venv), lim, amp)
        assert min(margins) >= EC.GATE_MARGIN, min(margins)
    _report(key)
    venv.close()


# ---- 5. an environment reads its own inputs only
def test_an_environment_reads_its_own_inputs_only():
    actions = EC.cart_actions(EC.TQUAT)[:3]
    grips = EC.gripper_actions(3)

    def go(order):
        venv = _env("fr3", EC.TQUAT, EC.LAST_STEP, n=len(order))
        o, _ = venv.reset()
        out = [o["tquat"], o["joints"]]
        for k in range(3):
            o, _, _, _, _ = venv.step({"tquat": actions[k][order], "gripper": grips[k][order]})
            s = _snapshot(venv)
            out += [o["tquat"], s["qpos"], s["qvel"], s["ctrl"], s["pose"], s["q_des"], s["fields"]["preva"], s["fields"]["origin"]]
        venv.close()
        return out

    batch = go(np.arange(N))
    rev = go(np.arange(N)[::-1])
    for a, b in zip(batch, rev):
        assert np.array_equal(a, b[::-1])
    for e in range(N):
        alone = go(np.array([e]))
        for a, b in zip(batch, alone):
            assert np.array_equal(a[e], b[0])


# ---- 6. the singular environment
def test_a_singular_environment_keeps_its_torque_and_raises_its_flag():
    s = OC.sample("ur5e", "0s")
    assert int(s["status"]) == 1 and int(s["task_mask"]) == 0x3F and float(s["damping"]) == 0.0
    q0, dp, dq, _ = TC.law_start("ur5e", seed=9)
    expect = np.arange(N) == 2

    def go(q_start):
        venv = _env("ur5e", EC.TQUAT, None, 0x3F, damping=0.0)
        sim, robot = venv.sim, venv.robot
        sim.set_qpos(q_start)
        sim.set_qvel(np.zeros_like(q_start))
        hold = venv.dynamics(want=("gravity",))["gravity"]
        robot.set_joint_torque(hold)
        tcp = robot.get_config().tcp_offset.inverse().as_vec7()
        pose_des = TC.pose_targets(robot.get_ik().forward(q0, tcp), dp, dq)  # (the same targets in both runs)
        o, _, _, _, info = venv.step({"tquat": pose_des})
        out = (sim.qpos, sim.qvel, sim.ctrl, o["tquat"], info["torque_singular"], hold)
        venv.close()
        return out

    q_sing = q0.copy()
    q_sing[2] = s["qpos"]
    with_it = go(q_sing)
    assert np.array_equal(with_it[4], expect)
    assert np.array_equal(with_it[2][2], with_it[5][2])  # (its torque is kept bit for bit)
    for a in with_it[:4]:
        assert np.isfinite(a).all()
    assert not np.array_equal(with_it[2][~expect], with_it[5][~expect])  # (the neighbours' law did act)
    q_reg = q0.copy()
    q_reg[2] = q0[3]
    without = go(q_reg)
    assert not without[4].any()
    for a, b in zip(with_it[:4], without[:4]):
        assert np.array_equal(a[~expect], b[~expect])


# ---- 7. autoreset
def test_autoreset_resets_done_environments_with_the_torque_reset():
    r = TC.oracle_robot("fr3")
    acts = EC.joint_actions(r["q_home"], r["low"], r["high"], EC.LAST_STEP)
    grips = EC.gripper_actions(3)
    lim = np.array(TC.RANGES["fr3"])
    early = np.arange(N) % 3 == 0  # reset once more after the first step: their episodes are one step behind

    def go(autoreset):
        venv = _env("fr3", EC.JOINTS, EC.LAST_STEP, 0)
        if autoreset:
            venv.configure_autoreset(max_episode_steps=2)
        venv.reset()
        venv.step({"joints": acts[0], "gripper": grips[0]})
        venv.reset(mask=early)
        return venv

    plain = go(False)
    auto = go(True)
    o_plain, _, _, _, _ = plain.step({"joints": acts[1], "gripper": grips[1]})
    after_plain = _snapshot(plain)
    o_auto, _, _, trunc, info = auto.step({"joints": acts[1], "gripper": grips[1]})
    after_auto = _snapshot(auto)
    done = info["autoreset"]
    assert np.array_equal(done, ~early) and np.array_equal(info["TimeLimit.truncated"], ~early)
    # rows that are not done: bit for bit the run without autoreset
    for name in ("qpos", "qvel", "ctrl", "time", "pose", "q_des"):
        assert np.array_equal(after_auto[name][~done], after_plain[name][~done]), name
    for name in ("tquat", "joints", "xyzrpy", "gripper"):
        assert np.array_equal(o_auto[name][~done], o_plain[name][~done]), name
        assert np.array_equal(info["final_obs"][name][done], o_plain[name][done]), name  # (the terminal observation)
    # done rows: the new episode's first observation, the targets at home, the state of the masked reset
    _obs_is_the_state(auto, o_auto)
    home = np.asarray(r["q_home"], dtype=np.float64)
    assert np.array_equal(after_auto["q_des"][done], np.tile(home, (int(done.sum()), 1)))
    blob, pre = plain.sim.get_state(), after_plain
    o_reset, _ = plain.reset(mask=done)
    fused_reset = _snapshot(plain)
    for name in ("qpos", "qvel", "ctrl", "time", "pose", "q_des"):
        assert np.array_equal(after_auto[name], fused_reset[name]), name
    assert np.array_equal(o_auto["tquat"], o_reset["tquat"]) and np.array_equal(o_auto["joints"], o_reset["joints"])
    _restore(plain, blob, pre)
    _compose_reset(plain, done)
    _compare("autoreset", "fr3", after_auto, _snapshot(plain), lim, rows=done)
    _report("autoreset")
    plain.close()
    auto.close()


# ---- 8. refusals
def _configure(venv, mode, relative_to=0):
    from rcs_amd import _lib

    d = _lib.EnvDesc()
    d.control_mode, d.relative_to, d.binary_gripper = mode, relative_to, 1
    d.max_mov[:] = [0.1, 0.1]
    d.joint_low = venv._low.ctypes.data_as(C.POINTER(C.c_double))
    d.joint_high = venv._high.ctypes.data_as(C.POINTER(C.c_double))
    return venv._L.rcsh_env_configure(venv.sim._h, C.byref(d))


def _scheduled_camera(simu):
    """A rate-driven camera on the scene's wrist camera (the torque-actuated variant keeps the scene's cameras): frames are scheduled
    by the stepping launches, which the fused torque launch does not serve."""
    from rcs_amd.camera import SimCameraConfig, SimCameraSet

    cams = {"wrist_0": SimCameraConfig(identifier="wrist_0", frame_rate=30, resolution_width=8, resolution_height=6)}
    return SimCameraSet(simu, cams, physical_units=True, render_on_demand=False, max_framesets=4)


def _unchanged(venv, blob, width):
    assert np.array_equal(venv.sim.get_state(), blob) and venv._L.rcsh_env_action_width(venv.sim._h) == width


def test_refusals_leave_state_and_configuration_alone():
    from rcs_amd import _lib, envs
    from rcs_amd.envs import ControlMode

    def err():
        return _lib.load().rcsh_last_error().decode()

    # a robot that is not torque-actuated
    venv = envs.make_vec_env(N, True, robot="fr3", resolve_robot_contacts=False)
    blob, width = venv.sim.get_state(), venv.action_width
    for mode in (3, 4, 5, 6):
        assert _configure(venv, mode) == _lib.RCSH_ERR_ARG and "not torque-actuated" in err()
    assert _configure(venv, 7) == _lib.RCSH_ERR_ARG
    _unchanged(venv, blob, width)
    venv.step({"joints": np.zeros((N, 7)), "gripper": np.ones(N, dtype=np.float32)})  # (and the JOINTS mode still steps)
    venv.close()
    with pytest.raises(ValueError, match="not torque-actuated"):
        envs.make_vec_env(N, True, robot="fr3", control_mode=ControlMode.TORQUE)
    # the torque variant in a position mode: resolved contacts, the guard, TORQUE with a relative action space
    venv = envs.make_vec_env(N, True, robot="fr3", torque_actuated=True, resolve_robot_contacts=True)
    blob, width = venv.sim.get_state(), venv.action_width
    assert _configure(venv, 4) == _lib.RCSH_ERR_ARG and "contacts are resolved" in err()
    _unchanged(venv, blob, width)
    venv.close()
    with pytest.raises(ValueError, match="resolves no contacts"):
        _env("fr3", EC.JOINTS, resolve_robot_contacts=True)
    venv = envs.make_vec_env(N, True, robot="fr3", torque_actuated=True, resolve_robot_contacts=False)
    blob, width = venv.sim.get_state(), venv.action_width
    assert _configure(venv, 3, relative_to=1) == _lib.RCSH_ERR_ARG and "relative" in err()
    venv.configure_guard()
    for mode in (3, 4, 5, 6):
        assert _configure(venv, mode) == _lib.RCSH_ERR_STATE and "guard" in err()
    _unchanged(venv, blob, width)
    venv.close()
    with pytest.raises(NotImplementedError):
        _env("fr3", EC.JOINTS, collision_guard=True)
    # async_control = 0
    venv = envs.make_vec_env(N, False, robot="fr3", torque_actuated=True, resolve_robot_contacts=False)
    blob, width = venv.sim.get_state(), venv.action_width
    for mode in (3, 4, 5, 6):
        assert _configure(venv, mode) == _lib.RCSH_ERR_ARG and "async_control" in err()
    _unchanged(venv, blob, width)
    venv.close()
    with pytest.raises(ValueError, match="async_control"):
        envs.make_vec_env(N, False, robot="fr3", torque_actuated=True, control_mode=ControlMode.TORQUE)
    # rate-driven cameras, scheduled before the mode is configured: rcsh_env_configure refuses
    venv = envs.make_vec_env(N, True, robot="fr3", torque_actuated=True, resolve_robot_contacts=False)
    cams = _scheduled_camera(venv.sim)
    blob, width = venv.sim.get_state(), venv.action_width
    for mode in (3, 4, 5, 6):
        assert _configure(venv, mode) == _lib.RCSH_ERR_ARG and "cameras are scheduled" in err()
    _unchanged(venv, blob, width)
    del cams
    venv.close()
    # ... and scheduled after it was accepted: only the step and the reset can refuse
    venv = _env("fr3", EC.JOINTS)
    venv.reset()
    venv.step({"joints": np.full((N, 7), 0.01), "gripper": np.ones(N, dtype=np.float32)})
    cams = _scheduled_camera(venv.sim)
    blob, start, width = venv.sim.get_state(), _snapshot(venv), venv.action_width
    with pytest.raises(ValueError, match="cameras are scheduled"):
        venv.step({"joints": np.full((N, 7), 0.02), "gripper": np.zeros(N, dtype=np.float32)})
    with pytest.raises(ValueError, match="cameras are scheduled"):
        venv.reset()
    with pytest.raises(ValueError, match="cameras are scheduled"):
        venv.reset(mask=np.arange(N) % 2 == 0)
    after = _snapshot(venv)
    _unchanged(venv, blob, width)
    assert np.array_equal(after["pose"], start["pose"]) and np.array_equal(after["q_des"], start["q_des"])
    assert np.array_equal(after["singular"], start["singular"])
    del cams
    venv.close()
    # a free body; the pick task
    cfg = TC.robot_cfg("fr3_pick")
    task = envs.creators.SimTaskEnvCreator()(cfg, control_mode=ControlMode.JOINTS, delta_actions=False, n_envs=N)
    blob = task.sim.get_state()
    assert _configure(task, 4) == _lib.RCSH_ERR_STATE and "pick task" in err()
    assert np.array_equal(task.sim.get_state(), blob)
    task.close()
    from rcs_amd import sim as S

    simu = S.Sim(cfg.mjcf_scene_path, S.SimConfig(async_control=True), n_envs=N)
    robot = S.SimRobot(simu, None, cfg)
    assert robot.torque_actuated
    with pytest.raises(ValueError, match="free body"):
        envs.creators.VecSimEnv(simu, robot, None, ControlMode.JOINT_IMPEDANCE, None, None)
    venv = envs.creators.VecSimEnv(simu, robot, None, ControlMode.JOINTS, None, None)
    blob, width = simu.get_state(), venv.action_width
    for mode in (3, 4, 5, 6):
        assert _configure(venv, mode) == _lib.RCSH_ERR_ARG and "free body" in err()
    _unchanged(venv, blob, width)
    simu.close()
    # a new mode configured: the guard and an impedance mode without an enabled law
    venv = _env("fr3", EC.JOINTS, law=False)
    blob, start = venv.sim.get_state(), _snapshot(venv)
    with pytest.raises(RuntimeError, match="guard"):
        venv.configure_guard()
    with pytest.raises(RuntimeError, match="enabled torque law"):
        venv.reset()
    with pytest.raises(RuntimeError, match="enabled torque law"):
        venv.step({"joints": np.zeros((N, 7)), "gripper": np.ones(N, dtype=np.float32)})
    venv.robot.configure_torque_law(**EC.LAW, enabled=False)
    with pytest.raises(RuntimeError, match="enabled torque law"):
        venv.step({"joints": np.zeros((N, 7)), "gripper": np.ones(N, dtype=np.float32)})
    after = _snapshot(venv)
    assert np.array_equal(venv.sim.get_state(), blob)
    assert np.array_equal(after["pose"], start["pose"]) and np.array_equal(after["q_des"], start["q_des"])
    venv.robot.configure_torque_law(**EC.LAW)
    venv.reset()  # (with the law enabled the same env works)
    venv.close()
    # the TCP mismatch: the robot's tcp_offset here is 10 cm along z and a turn about it, the law's TCP composes the INVERSE of its offset
    cfg_tcp = EC.fr3_tcp()
    for bad in (cfg_tcp.as_vec7(), np.zeros(7)):
        venv = _env("fr3", EC.TQUAT, law=dict(EC.LAW, tcp_offset=bad if bad.any() else None) if bad.any() else False)
        if not bad.any():
            venv.robot.configure_torque_law(**EC.LAW)  # (tcp_offset None: the site itself)
        blob, start = venv.sim.get_state(), _snapshot(venv)
        with pytest.raises(ValueError, match="same TCP"):
            venv.reset()
        with pytest.raises(ValueError, match="same TCP"):
            venv.step({"tquat": np.tile([0, 0, 0, 0, 0, 0, 1.0], (N, 1)), "gripper": np.ones(N, dtype=np.float32)})
        after = _snapshot(venv)
        assert np.array_equal(venv.sim.get_state(), blob) and np.array_equal(after["pose"], start["pose"])
        # the joint modes do not read the pose: they run with any offset
        assert _configure(venv, 4, relative_to=1) == _lib.RCSH_OK
        venv.close()
    # the negated quaternion is the same TCP
    inv = cfg_tcp.inverse().as_vec7()
    inv[3:] *= -1.0
    venv = _env("fr3", EC.TQUAT, law=dict(EC.LAW, tcp_offset=inv))
    venv.reset()
    venv.close()


# ---- 9. the resident loop
def test_step_dev_and_reset_dev_give_the_host_forms_rows():
    actions = EC.cart_actions(EC.TQUAT)[:3]
    grips = EC.gripper_actions(3)
    host = _env("fr3", EC.TQUAT, EC.CONFIGURED_ORIGIN)
    dev = _env("fr3", EC.TQUAT, EC.CONFIGURED_ORIGIN)
    L, h = dev._L, dev.sim._h
    from rcs_amd import _lib

    bufs = []

    def dalloc(nbytes):
        p = C.c_void_p()
        _lib.check(L.rcsh_dev_alloc(h, int(nbytes), C.byref(p)))
        bufs.append(p)
        return p

    def up(a):
        a = np.ascontiguousarray(a)
        p = dalloc(a.nbytes)
        _lib.check(L.rcsh_dev_upload(h, p, C.c_void_p(a.ctypes.data), a.nbytes))
        return p

    def down(p, shape, dtype=np.float64):
        a = np.zeros(shape, dtype=dtype)
        dev.sim.synchronize()
        _lib.check(L.rcsh_dev_download(h, C.c_void_p(a.ctypes.data), p, a.nbytes))
        return a

    ow = dev.obs_width
    d_obs, d_info, d_gw, d_sub = dalloc(N * ow * 8), dalloc(N * 8), dalloc(N * 8), dalloc(N * 4)

    def rows():
        return down(d_obs, (N, ow)), down(d_info, (N, 8), np.uint8), down(d_gw, (N,)), down(d_sub, (N,), np.int32)

    def host_rows(call):
        obs, info, gw, sub = np.zeros((N, ow)), np.zeros((N, 8), dtype=np.uint8), np.zeros(N), np.zeros(N, dtype=np.int32)
        call(obs, info, gw, sub)
        return obs, info, gw, sub

    Lh, hh = host._L, host.sim._h
    ref = host_rows(lambda o, i, g, s: _lib.check(Lh.rcsh_env_reset(hh, None, _lib.ptr(o), _lib.ptr(i), _lib.ptr(g))))
    dev.reset_dev(d_obs.value, d_info.value, d_gw.value)
    got = rows()
    for a, b in zip(ref[:3], got[:3]):
        assert np.array_equal(a, b)
    for k in range(3):
        a, g = np.ascontiguousarray(actions[k]), np.ascontiguousarray(grips[k])
        ref = host_rows(lambda o, i, gw, s: _lib.check(Lh.rcsh_env_step(hh, _lib.ptr(a), _lib.ptr(g), _lib.ptr(o), _lib.ptr(i), _lib.ptr(gw), _lib.ptr(s))))
        dev.step_dev(up(a).value, up(g).value, d_obs.value, d_info.value, d_gw.value, d_sub.value)
        for x, y in zip(ref, rows()):
            assert np.array_equal(x, y), k
        assert (ref[3] == EC.SUBSTEPS).all()
        if k == 1:  # a masked reset in between: the `_dev` form writes the masked rows only
            mask = (np.arange(N) % 2 == 1).astype(np.uint8)
            ref = host_rows(lambda o, i, gw, s: _lib.check(Lh.rcsh_env_reset(hh, _lib.ptr(mask), _lib.ptr(o), _lib.ptr(i), _lib.ptr(gw))))
            dev.reset_dev(d_obs.value, d_info.value, d_gw.value, up(mask).value)
            got = rows()
            for x, y in zip(ref[:3], got[:3]):
                assert np.array_equal(x[mask == 1], y[mask == 1])
    for name in ("qpos", "qvel", "ctrl"):
        assert np.array_equal(getattr(host.sim, name), getattr(dev.sim, name))
    hp, dp = host.robot.torque_target(), dev.robot.torque_target()
    assert np.array_equal(hp[0], dp[0]) and np.array_equal(hp[1], dp[1])
    for p in bufs:
        _lib.check(L.rcsh_dev_free(h, p))
    host.close()
    dev.close()
