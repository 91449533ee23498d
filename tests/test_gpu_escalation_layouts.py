"""Per-environment escalation at every batch layout (csrc/sim_kernels.h: esc_select, esc_finish; the redo from the launch's copy).

The property: an environment's trajectory depends on its own inputs only, BIT FOR BIT -- not on its index in the batch, on the batch
size, or on who else is escalated.  tests/escalation_cases.py scripts 16 characters and arranges replicas of them into batches that
reach every arm of the selection (1 to 4 environments per workgroup and both sides of each threshold, single escalated environments on
a word boundary, a partly filled last word, the second pass over the escalation words at more than 4096 environments, launches with
nobody to step).  One batch holds every character once and is held to the oracle at the project's bars; every environment of every
arrangement then has to equal its character's column of that batch exactly, after every launch, in every array the step leaves.

The bar of the arrangement tests is np.array_equal for every array but one part of one: the state's last 16 fields (Lay::SEP,
csrc/sim_kernels.h), the four separating directions the end-of-launch check remembers per environment (csrc/check_team.h).  Which of
an environment's near pairs finds a slot empty follows from the order in which the wavefront's rounds meet them, and a round's pair is
chosen over all four teams of the wavefront: with two folded characters side by side (the reference batch) slot 0 holds another pair
than with free neighbours (the mixed arrangements).  The slots are hints -- a direction that no longer certifies is found again --, the
oracle has no counterpart of them, and so they are held to what they must be in any layout instead: a slot is empty or holds a pair key
(a positive whole number) and a unit vector, to the project's 1e-9.  The dependence does not end with the slots: the direction that
proves a pair apart sets the pair's slack record (outside the state blob, compared by nothing here), which decides when the pair is
due again, and it can decide whether the certificate passes -- the `now` bit.  That `escalated.now` and every other array are
bit-equal on these layouts is measured, not implied by "the slots are hints": an arrangement that fails on `escalated.now` first
points at the slot choice in csrc/check_team.h, not at esc_select."""

import time

import numpy as np
import pytest

import escalation_cases as E

pytestmark = pytest.mark.gpu


def _state_columns(blob, n):
    from test_gpu_autoreset import _state_columns as columns

    S, flags, conv = columns(blob, n)
    return np.ascontiguousarray(S.T), flags.copy(), conv.copy()  # (every array: environment first)


SEP_WORDS = 16  # kCheckSep (csrc/check_team.h): four slots of (pair key, direction) at the end of an environment's state fields


def _check_remembered_directions(tag, sep):
    slots = sep.reshape(len(sep), SEP_WORDS // 4, 4)
    key, norm = slots[..., 0], np.linalg.norm(slots[..., 1:], axis=-1)
    used = key != 0.0
    assert ((key >= 0) & (key == np.floor(key))).all(), (tag, key[key != np.floor(key)])
    assert (np.abs(norm[used] - 1.0) <= 1e-9).all(), (tag, norm[used])


def _sim_arrays(simu, n):
    now, ever = simu.contact_escalated()
    S, flags, conv = _state_columns(simu.get_state(), n)
    return {"qpos": np.array(simu.qpos), "qvel": np.array(simu.qvel), "state.fields": S, "state.flags": flags, "state.convergence": conv,
            "escalated.now": now, "escalated.ever": ever, "contact_overflow()": simu.contact_overflow(), "contact_unresolved()": simu.contact_unresolved()}


def _env_rollout(arr, after_launch):
    """The arrangement through the fused env step; `after_launch(t, arrays)` gets every per-environment array of launch t."""
    from parity_util import make_vec_env

    start, act, grip = E.characters()
    n = len(arr)
    venv = make_vec_env(n, True)
    assert venv.sim.resolve_robot_contacts == 7
    venv.reset()
    venv.robot.set_joints_hard(np.ascontiguousarray(start[arr, :7]))
    venv.sim.set_qpos(np.ascontiguousarray(start[arr]))
    try:
        for t in range(E.LAUNCHES):
            obs, reward, terminated, truncated, info = venv.step({"joints": act[t][arr], "gripper": grip[t][arr]})
            row = {"reward": reward, "terminated": terminated, "truncated": truncated}
            row.update({"obs." + k: np.asarray(v) for k, v in obs.items()})
            row.update({"info." + k: np.asarray(v) for k, v in info.items()})
            row.update(_sim_arrays(venv.sim, n))
            assert all(a.shape[0] == n for a in row.values())
            after_launch(t, row)
    finally:
        venv.close()


FINE_CALLS = {"step": E.LAUNCHES, "converge": 6}


def _fine_rollout(arr, mode, after_launch):
    """The arrangement through the fine-grained API: set_joint_position, then Sim.step(17) ("step") or step_until_convergence
    ("converge": synchronous control; launch_run cuts it into pieces and carries the substep count across the redos).  The target of a
    launch is where the arm is plus the character's action -- the relative action space's rule, applied on the host."""
    from rcs_amd import sim as S
    from rcs_amd.envs import default_sim_gripper_cfg, default_sim_robot_cfg

    start, act, _ = E.characters()
    n = len(arr)
    cfg = default_sim_robot_cfg("fr3_empty_world")
    simu = S.Sim(cfg.mjcf_scene_path, S.SimConfig(async_control=mode == "step"), n_envs=n, resolve_robot_contacts=7)
    robot = S.SimRobot(simu, None, cfg)
    S.SimGripper(simu, default_sim_gripper_cfg())
    simu.step(1)
    robot.set_joints_hard(np.ascontiguousarray(start[arr, :7]))
    simu.set_qpos(np.ascontiguousarray(start[arr]))
    try:
        for t in range(FINE_CALLS[mode]):
            robot.set_joint_position(np.ascontiguousarray(simu.qpos[:, :7] + act[t][arr]))
            if mode == "step":
                simu.step(E.SUBSTEPS)
            else:
                simu.step_until_convergence()
            row = _sim_arrays(simu, n)
            row.update({"is_converged": simu.is_converged(), "convergence_steps": simu.convergence_steps()})
            after_launch(t, row)
    finally:
        simu.close()


def _collect(rollout, *args):
    rows = []
    rollout(np.arange(E.N_CHARACTERS), *args, lambda t, row: rows.append(row))
    return rows


@pytest.fixture(scope="module")
def reference():
    """The batch that holds every character once, in order, through the fused env step: every launch's arrays."""
    return _collect(_env_rollout)


@pytest.fixture(scope="module")
def fine_reference():
    return {mode: _collect(_fine_rollout, mode) for mode in FINE_CALLS}


def _compare(name, arr, ref_rows, rollout, *args):
    """Every environment of the arrangement against its character's column of the reference rows; returns the escalated count per launch."""
    counts = []

    def after_launch(t, row):
        ref = ref_rows[t]
        assert row.keys() == ref.keys()
        for k, a in row.items():
            want = ref[k][arr]
            if k == "state.fields":  # (the remembered directions: see the module's docstring)
                _check_remembered_directions((name, t), a[:, -SEP_WORDS:])
                a, want = a[:, :-SEP_WORDS], want[:, :-SEP_WORDS]
            if not np.array_equal(a, want):
                bad = np.flatnonzero((a != want).reshape(len(arr), -1).any(axis=1))
                raise AssertionError(f"{name}, launch {t}, {k}: {len(bad)} of {len(arr)} environments differ from their character's column "
                                     f"-- first {bad[:12].tolist()} (characters {arr[bad[:12]].tolist()})")
        counts.append(int(row["escalated.now"].sum()))

    t0 = time.perf_counter()
    rollout(arr, *args, after_launch)
    return counts, time.perf_counter() - t0


def test_reference_batch_matches_the_oracle(reference):
    """Joints and finger slides <= 1e-9, velocities <= 1e-8, collision / ik_success / truncated / gripper observation equal, in every
    launch; resolved-ever equals "the oracle has seen a contact"; no contact overflow, nothing unresolved; the free characters are never
    on the contact-resolving launch; some character leaves it again; the `now` bits of the plateau launch are the table's."""
    o = E.oracle_run()
    err_q, err_v = np.zeros(E.N_CHARACTERS), np.zeros(E.N_CHARACTERS)
    now = np.array([r["escalated.now"] for r in reference])
    ever = np.array([r["escalated.ever"] for r in reference])
    print("\n`now` per launch (characters 0..15):")
    for t in range(E.LAUNCHES):
        print(f"  {t:2d} {now[t].astype(int).tolist()}")
    seen = np.zeros(E.N_CHARACTERS, dtype=bool)
    for t, r in enumerate(reference):
        dq = np.maximum(np.abs(r["qpos"] - o["qpos"][t]).max(axis=1), np.abs(r["obs.joints"] - o["joints"][t]).max(axis=1))
        dq = np.maximum(dq, np.abs(r["obs.tquat"] - o["tquat"][t]).max(axis=1))
        err_q, err_v = np.maximum(err_q, dq), np.maximum(err_v, np.abs(r["qvel"] - o["qvel"][t]).max(axis=1))
        for k, ok in (("info.collision", "collision"), ("info.ik_success", "ik_success"), ("truncated", "truncated")):
            assert np.array_equal(r[k].astype(bool), o[ok][t]), (t, k, r[k], o[ok][t])
        assert np.array_equal(r["obs.gripper"].astype(np.float64), o["gripper"][t]), (t, r["obs.gripper"])
        seen |= o["contact"][t]
        assert np.array_equal(ever[t], seen), (t, ever[t].astype(int), seen.astype(int))
        assert not r["info.contact_overflow"].any() and not r["info.contact_unresolved"].any(), t
        assert not r["contact_overflow()"].any() and not r["contact_unresolved()"].any(), t
        assert (now[t] | ~o["contact"][t]).all(), (t, "a character in contact is on the contact-resolving launch")
        _check_remembered_directions(("reference", t), r["state.fields"][:, -SEP_WORDS:])
    print(f"largest |dq| per character {err_q.tolist()}\nlargest |dv| per character {err_v.tolist()}")
    assert err_q.max() <= 1e-9 and err_v.max() <= 1e-8, (err_q, err_v)
    assert not now[:, list(E.FREE)].any(), now[:, list(E.FREE)]
    assert (ever[-1] & ~now[-1]).any(), "somebody has left the contact-resolving launch again"
    assert np.array_equal(now[E.T_STAR], E.ESCALATED_AT_T_STAR), now[E.T_STAR].astype(int)


@pytest.mark.parametrize("name", list(E.arrangements()))
def test_every_environment_equals_its_character(name, reference):
    n, arr, count = E.arrangements()[name]
    counts, seconds = _compare(name, arr, reference, _env_rollout)
    per = sorted({E.per_of(n, c) for c in counts})
    print(f"\n{name}: n {n}, escalated per launch {counts}, environments per workgroup reached {per}, {seconds:.2f} s")
    assert counts[E.T_STAR] == count, (counts, count)
    assert E.per_of(n, count) in per


@pytest.mark.parametrize("mode", list(FINE_CALLS))
def test_fine_grained_api_at_a_mixed_layout(mode, fine_reference):
    """The same property through set_joint_position + Sim.step(17), and through step_until_convergence, whose pieces carry the substep
    count and the verdicts across the launches that are redone: the mixed 70-environment arrangement against a 16-environment batch
    driven the same way."""
    ref = fine_reference[mode]
    now = np.array([r["escalated.now"] for r in ref])
    ever = np.array([r["escalated.ever"] for r in ref])
    print(f"\n{mode}: `now` per call {[row.astype(int).tolist() for row in now]}")
    # the batch is split between the two launches in some call, somebody is newly flagged after the first call (a redo next to environments
    # that continue), and a contact has been resolved
    assert any(0 < row.sum() < len(row) for row in now) and (now[1:] & ~now[:-1]).any() and ever[-1].any()
    if mode == "converge":
        steps = np.array([r["convergence_steps"] for r in ref])
        print(f"convergence steps per call {steps.tolist()}")
        assert (steps[now] > 48).any(), "an escalated environment's convergence spans more than one piece"
    n, arr, _ = E.arrangements()[E.FINE_GRAINED]
    counts, seconds = _compare(f"{E.FINE_GRAINED} ({mode})", arr, ref, _fine_rollout, mode)
    per = sorted({E.per_of(n, c) for c in counts})
    print(f"escalated per call {counts}, environments per workgroup reached {per}, {seconds:.2f} s")
    # the arrangement's own counts: what its characters' bits add up to, split between the two launches, somebody newly flagged
    assert counts == [int(row[arr].sum()) for row in now], (counts, [int(row[arr].sum()) for row in now])
    assert any(0 < c < n for c in counts) and any(b > a for a, b in zip(counts, counts[1:]))
