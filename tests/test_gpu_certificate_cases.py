"""The lean launch's end-of-launch certificate (csrc/check_team.h, fed by chk_dend / chk_psum / chk_q0 in csrc/sim_kernels.h) on contacts
that begin and end inside one launch: the rows of tests/golden/certificate_cases.json, which tests/test_certificate_cases_cpu.py proves
to be such contacts on the oracle.

resolve_robot_contacts=7 (per-environment escalation), the fine-grained API (SimRobot.set_joint_position, then Sim.step(k) under
asynchronous control or Sim.step_until_convergence under synchronous control), hard starts; the "env" rows go through the env layer (the
fused env step under synchronous control, relative joint actions) against the oracle's env layer.  After EVERY launch, for EVERY environment:
  (a) qpos <= 1e-9 and qvel <= 1e-8 against the resolving oracle; step_until_convergence: the substep counts are equal too;
  (b) a launch in which the oracle's pen_seen exceeds 1e-8 (10 x kCheckTouch) leaves `ever` set, and `now` set: an environment in which a
      substep met a contact does not go back in the same launch (csrc/sim_kernels.h: the esc[2] "leave" bit is for an environment none of
      whose substeps met a contact).  step_until_convergence (direct or through the env) is the exception: the launcher cuts a call into pieces of 48 substeps, each
      a launch of its own, and a piece after the graze that passes the certificate takes the environment back -- there `ever` and parity
      are the assertion;
  (c) contact_overflow() is false;
  (d) the quiet characters never have `ever` set, and (stronger: they are a centimetre from everything) never `now`.
What the rows exercise is read from the escalation bits and partly ASSERTED (a row's `lean` / `returns` keys, set by the generator's rule):
  * a sweep nears its lowest point along a tangent, so the launch BEFORE its graze ends nearer to the contact than it travelled and fails
    the certificate itself: the swept characters are on the contact-resolving launch a launch early, and their graze launch tests that
    the contact-resolving launch's certificate does not take them back (printed: "graze launches begun on the lean launch");
  * `lean` rows must BEGIN their graze launch on the lean launch, so its certificate is what sends the launch to be redone: a graze in the
    first launch after the hard start (the `-launch0` characters, two shallow ones, every convergence one), and the `held` carried-slack
    characters, which rest 1, 3 and 8 launches on their start pose -- lean launches that write and charge the slack record -- and graze
    in their first moving launch;
  * `returns` rows (there and back, nine launches at rest between the grazes) must be back on the lean launch somewhere in between.
With a stage of the certificate switched off (the last test) both kinds go through the contact unresolved.
Every replica of a character in every arrangement equals the character's column of the batch that holds each character once, bit for bit
in qpos and qvel (the rule of tests/test_gpu_escalation_layouts.py)."""

import functools

import numpy as np
import pytest

import certificate_cases as CC

pytestmark = pytest.mark.gpu

SWITCH = "RCSH_CHECK_SKIP"
FORMS = tuple(CC.SUBSTEPS)
PIECES = ("converge", "env")  # step_until_convergence: a call is several launches of 48 substeps


def _launch(simu, form):
    if form == "converge":
        simu.step_until_convergence()
    else:
        simu.step(CC.SUBSTEPS[form])


def _run(rows, form, variant="plain"):
    """The batch on the kernels: per launch qpos, qvel, `now`, `ever`, overflow, convergence steps.  `variant`:
      "plain"   hard starts after the first substep at home;
      "writes"  the batch rests REST_LAUNCHES launches first -- the graze characters at a quiet pose, the quiet ones at their own starts --,
                then the graze characters' start states are written under a mask (set_joints_hard + set_qpos + set_qvel);
      "state"   the start states are snapshotted (get_state), everybody rests at a quiet pose, the snapshot is written back (set_state)."""
    from rcs_amd import sim as S
    from rcs_amd.envs import default_sim_gripper_cfg, default_sim_robot_cfg

    if form == "env":
        assert variant == "plain"
        return _run_env(rows)
    n = len(rows)
    cfg = default_sim_robot_cfg("fr3_empty_world")
    simu = S.Sim(cfg.mjcf_scene_path, S.SimConfig(async_control=form != "converge"), n_envs=n, resolve_robot_contacts=7)
    robot = S.SimRobot(simu, None, cfg)
    S.SimGripper(simu, default_sim_gripper_cfg())
    q0 = np.array([CC.start_state(r)[0] for r in rows])
    v0 = np.array([CC.start_state(r)[1] for r in rows])
    tg = np.array([CC.targets(r) for r in rows])  # [n, launches, 7]
    graze = np.array([r["family"] != "quiet" for r in rows])
    rest_pose = np.asarray(CC.quiet_rows(form)[0]["start"])

    def write(q, v, mask=None):
        robot.set_joints_hard(np.ascontiguousarray(q[:, :7]), mask)
        simu.set_qpos(np.ascontiguousarray(q), mask)
        simu.set_qvel(np.ascontiguousarray(v), mask)

    rec = []

    def record():
        now, ever = simu.contact_escalated()
        rec.append({"qpos": np.array(simu.qpos), "qvel": np.array(simu.qvel), "now": now.copy(), "ever": ever.copy(),
                    "overflow": np.array(simu.contact_overflow()), "steps": np.array(simu.convergence_steps()) if form == "converge" else None})

    try:
        simu.step(1)
        write(q0, v0)
        if variant != "plain":
            blob = simu.get_state()
            q_rest = q0.copy()
            q_rest[graze | (variant == "state")] = rest_pose
            write(q_rest, np.zeros_like(v0))
            for _ in range(CC.REST_LAUNCHES):
                robot.set_joint_position(np.ascontiguousarray(q_rest[:, :7]))
                _launch(simu, form)
                record()
            if variant == "state":
                simu.set_state(blob)
            else:
                write(q0, v0, graze)
        before = simu.contact_escalated()[0].copy()
        for t in range(tg.shape[1]):
            robot.set_joint_position(np.ascontiguousarray(tg[:, t]))
            _launch(simu, form)
            record()
            rec[-1]["before"] = before  # (`now` before the script's first launch)
    finally:
        simu.close()
    return rec


def _run_env(rows):
    """The batch through the env layer: the fused env step under synchronous control (JOINTS relative to the last step, the gripper commanded
    open), where the action is applied inside the kernel in the call's first piece and an environment escalated there is redone from the
    copy and applies it again."""
    from parity_util import make_vec_env

    n = len(rows)
    q0 = np.array([CC.start_state(r)[0] for r in rows])
    v0 = np.array([CC.start_state(r)[1] for r in rows])
    act = np.array([CC.actions(r) for r in rows])  # [n, calls, 7]
    venv = make_vec_env(n, False)
    assert venv.sim.resolve_robot_contacts == 7
    rec = []
    try:
        venv.reset()
        venv.robot.set_joints_hard(np.ascontiguousarray(q0[:, :7]))
        venv.sim.set_qpos(np.ascontiguousarray(q0))
        venv.sim.set_qvel(np.ascontiguousarray(v0))
        before = venv.sim.contact_escalated()[0].copy()
        for t in range(act.shape[1]):
            _, _, _, trunc, info = venv.step({"joints": np.ascontiguousarray(act[:, t]), "gripper": np.ones(n, dtype=np.float32)})
            now, ever = venv.sim.contact_escalated()
            rec.append({"qpos": np.array(venv.sim.qpos), "qvel": np.array(venv.sim.qvel), "now": now.copy(), "ever": ever.copy(), "before": before,
                        "overflow": np.array(venv.sim.contact_overflow()), "steps": np.array(venv.sim.convergence_steps()),
                        "truncated": np.asarray(trunc, dtype=bool).copy()})
    finally:
        venv.close()
    return rec


@functools.lru_cache(maxsize=None)
def _once(form, variant="plain"):
    rows = CC.arrangements(form)["once"]
    return rows, _run(rows, form, variant)


@functools.lru_cache(maxsize=None)
def _oracle(name, form, rested, written=False):
    """The resolving oracle's replay of a row; `rested`: a quiet row of the "writes" variant, whose script begins with its rest; `written`:
    a graze row of that variant, whose start state is written after a rest at the quiet pose (under synchronous control the rest moves
    the clock the convergence callbacks run by: tests/test_certificate_cases_cpu.py)."""
    row = next(r for r in CC.arrangements(form)["once"] if r["name"] == name)
    if rested:
        row = dict(row, ramp=[row["start"][row["joint"]]] * CC.REST_LAUNCHES + list(row["ramp"]))
    return CC.replay(row, rest=(CC.REST_LAUNCHES, np.asarray(CC.quiet_rows(form)[0]["start"])) if written else None)


def _hold_to_the_oracle(rows, rec, form, variant="plain"):
    """(a) .. (d) for every launch and environment; returns the per-row report: errors, and the quiet launches that were escalated anyway."""
    rest = 0 if variant == "plain" else CC.REST_LAUNCHES
    report, failures = [], []
    for e, row in enumerate(rows):
        quiet = row["family"] == "quiet"
        rested = quiet and variant == "writes"
        orc = _oracle(row["name"], form, rested, variant == "writes" and not quiet)
        first = 0 if rested else rest
        err_q = err_v = 0.0
        false_alarms = 0
        lean_before = []  # per graze launch: the environment began it on the lean launch, so the certificate is what sent it to be redone
        for t in range(first, len(rec)):
            r, k = rec[t], t - first
            dq = float(np.abs(r["qpos"][e] - orc["qpos"][k]).max())
            dv = float(np.abs(r["qvel"][e] - orc["qvel"][k]).max())
            err_q, err_v = max(err_q, dq), max(err_v, dv)
            if dq > 1e-9 or dv > 1e-8:
                failures.append((row["name"], t, "parity", dq, dv))
            if form in PIECES and int(r["steps"][e]) != int(orc["steps"][k]):
                failures.append((row["name"], t, "substeps", int(r["steps"][e]), int(orc["steps"][k])))
            if orc["pen"][k] > CC.SEEN:
                lean_before.append(not (r["before"][e] if t == rest else rec[t - 1]["now"][e]))
                if not r["ever"][e] or (form not in PIECES and not r["now"][e]):
                    failures.append((row["name"], t, "a graze launch that was not escalated", bool(r["now"][e]), bool(r["ever"][e])))
                if row.get("lean") and not lean_before[-1]:
                    failures.append((row["name"], t, "a graze launch that did not begin on the lean launch"))
            if form == "env" and bool(r["truncated"][e]) != bool(orc["truncated"][k]):
                failures.append((row["name"], t, "truncated", bool(r["truncated"][e])))
            elif orc["pen"][k] == 0.0 and not quiet:
                false_alarms += int(r["now"][e])
            if r["overflow"][e]:
                failures.append((row["name"], t, "overflow"))
            if quiet and (r["ever"][e] or r["now"][e]):
                failures.append((row["name"], t, "a quiet character was escalated"))
        if row.get("returns") and variant == "plain":  # there and back: between its two grazes the environment goes back to the lean launch
            g0, g1 = row["graze"]
            if all(rec[t]["now"][e] for t in range(g0 + 1, g1)):
                failures.append((row["name"], g1, "never back on the lean launch between its two grazes"))
        report.append({"name": row["name"], "family": row["family"], "dq": err_q, "dv": err_v, "false_alarms": false_alarms, "lean_before": lean_before,
                       "now": "".join(str(int(rec[t]["now"][e])) for t in range(first, len(rec))),
                       "quiet_launches": int((orc["pen"] == 0.0).sum())})
    return report, failures


def _print(tag, report):
    print(f"\n{tag}")
    for r in report:
        print(f"  {r['name']:28s} |dq| {r['dq']:.2e} |dv| {r['dv']:.2e}  on the contact-resolving launch in {r['false_alarms']} of {r['quiet_launches']} quiet launches"
              + (f", graze launches begun on the lean launch {[int(x) for x in r['lean_before']]}, `now` after each launch {r['now']}" if r["family"] != "quiet" else ""))
    fam = {}
    for r in report:
        a = fam.setdefault(r["family"], [0, 0])
        a[0] += r["false_alarms"]
        a[1] += r["quiet_launches"]
    print("  false alarms per family (measured, not asserted):", {k: f"{a}/{b}" for k, (a, b) in fam.items() if k != "quiet"})
    lean = {}
    for r in report:
        if r["family"] != "quiet":
            a = lean.setdefault(r["family"], [0, 0])
            a[0] += sum(r["lean_before"])
            a[1] += len(r["lean_before"])
    print("  graze launches begun on the lean launch, per family:", {k: f"{a}/{b}" for k, (a, b) in lean.items()})


@pytest.mark.parametrize("form", FORMS)
def test_every_character_once(form):
    rows, rec = _once(form)
    report, failures = _hold_to_the_oracle(rows, rec, form)
    _print(f"{form}: every character once ({len(rows)} environments, {len(rec)} launches)", report)
    assert not failures, failures


def _equal_to_its_character(name, rows, rec, ref_rows, ref_rec):
    col = {r["name"]: i for i, r in enumerate(ref_rows)}
    idx = np.array([col[r["name"]] for r in rows])
    for t, (a, b) in enumerate(zip(rec, ref_rec)):
        for k in ("qpos", "qvel"):
            if not np.array_equal(a[k], b[k][idx]):
                bad = np.flatnonzero((a[k] != b[k][idx]).any(axis=1))
                raise AssertionError(f"{name}, launch {t}, {k}: environments {bad.tolist()} ({[rows[i]['name'] for i in bad]}) differ from their character's column")


@pytest.mark.parametrize("form,name", [(f, n) for f in FORMS for n in CC.arrangements(f) if n != "once"])
def test_arrangements(form, name):
    """Every graze character at each of a wavefront's four team positions with three quiet neighbours, packed four to a wavefront, and in a
    batch whose size is no multiple of 4: (a) .. (d), and bit-equal to the character's column of the batch that holds each once."""
    rows = CC.arrangements(form)[name]
    rec = _run(rows, form)
    report, failures = _hold_to_the_oracle(rows, rec, form)
    _print(f"{form}, {name}: {len(rows)} environments", report)
    assert not failures, failures
    _equal_to_its_character(f"{form} {name}", rows, rec, *_once(form))


@pytest.mark.parametrize("variant", ["writes", "state"])
@pytest.mark.parametrize("form", [f for f in FORMS if f != "env"])
def test_after_a_state_write(form, variant):
    """The consumer side of void_remembered_gaps: the batch rests at quiet poses, where the slack records grow large, then the graze
    characters' start states are written (set_joints_hard + set_qpos + set_qvel under a mask that leaves the quiet neighbours alone; or
    get_state / set_state) and the scripts run.  A slack record that survived the write would certify the graze launch."""
    rows, rec = _once(form, variant)
    report, failures = _hold_to_the_oracle(rows, rec, form, variant)
    _print(f"{form}, after {variant}: {len(rows)} environments", report)
    assert not failures, failures


@pytest.mark.parametrize("switch,geom_types", [("1", (7, 7)), ("2", (6,))], ids=["no-narrow-phase", "no-boxes"])
def test_teeth_certificate_with_a_stage_switched_off_lets_a_graze_through(switch, geom_types, monkeypatch):
    """RCSH_CHECK_SKIP=1 takes the narrow phase out of the certificate, =2 the oriented boxes and everything after them: the self-deep
    characters then show what this file is for.  At least one hull-hull character (=1) / one character whose pair has a box geom (=2) must
    miss (a) by more than 1e-6 or miss (b); if none does, the family does not reach that stage and the table has to be redone.  (Wrong
    numbers, not faults: the switch only makes the certificate say "apart".)"""
    monkeypatch.setenv(SWITCH, switch)  # (read on every launch)
    rows = CC.arrangements("step17")["once"]
    rec = _run(rows, "step17")
    monkeypatch.delenv(SWITCH)
    cm = CC.compiled_model()
    types = {n: int(cm.arrays["geom_type"][g]) for g, n in enumerate(cm.geom_names)}
    report, failures = _hold_to_the_oracle(rows, rec, "step17")
    want = []
    for r in rows:
        if r["family"] != "self-deep":
            continue
        ta, tb = (types[n] for n in r["pair"])
        if (geom_types == (7, 7) and ta == tb == 7) or (geom_types == (6,) and 6 in (ta, tb)):
            want.append(r["name"])
    assert want
    missed = {}
    for f in failures:
        if f[0] in want and ((f[2] == "parity" and f[3] > 1e-6) or f[2].startswith("a graze launch")):
            missed.setdefault(f[0], f)
    print(f"\nRCSH_CHECK_SKIP={switch}: of {want}, let through: {list(missed.values())}")
    assert missed, (want, failures[:8])
    # the characters whose graze launch the lean launch's certificate decides are among them
    assert any(f[0] in want and next(r for r in rows if r["name"] == f[0]).get("lean") for f in missed.values()), missed
    assert not any(f[2] == "a quiet character was escalated" for f in failures)
