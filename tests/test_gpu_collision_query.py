"""Batched collision queries (SimRobot.check_collision / check_motion, csrc/query_team.h) against the oracle's collision pass.

The ground truth is what MuJoCo's collision pass reports at a given qpos (oracle orc_kinematics + orc_collide on a copy of an oracle
environment's data, as parity_util.oracle_contacts_at_current_qpos does), with the free box's pose written through box_qpos."""

import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "robot-control-stack_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

TOUCH = 1e-9
BAND = 1e-7  # rows whose oracle depth lies this close to the 1e-9 bar may differ (counted, < 1 %)


class OracleCollider:
    """The oracle's collision pass at arbitrary configurations of one oracle environment (a private copy of its data)."""

    def __init__(self, osim):
        import rcs_oracle as O

        self.O, self.L, self.osim = O, O.lib(), osim
        self.d = O.OrcData.from_buffer_copy(osim.s.d)
        m = osim.model
        self.ngeom = int(m.ngeom)
        self.gtype = [int(m.geom_type[g]) for g in range(self.ngeom)]

    def pairs(self, q, box=None):
        """{kind: {(g0, g1): depth}} of the penetrating pairs (kind 0 floor, 1 self, 2 free box) and the smallest distance of any
        reported depth from the 1e-9 bar."""
        d = self.d
        for i, x in enumerate(q):
            d.qpos[i] = float(x)
        if box is not None:
            b = np.asarray(box, dtype=np.float64)
            qn = b[3:] / np.linalg.norm(b[3:])
            d.box.qpos[:] = [float(x) for x in b]
            d.box.xpos[:] = [float(x) for x in b[:3]]
            d.box.xquat[:] = [float(x) for x in qn]
        self.L.orc_kinematics(C.byref(self.osim.model), C.byref(d))
        self.L.orc_collide(C.byref(self.osim.model), C.byref(d))
        out = {0: {}, 1: {}, 2: {}}
        near = np.inf
        gbox = self.ngeom
        for i in range(d.ncon):
            c = d.contact[i]
            g0, g1 = int(c.geom[0]), int(c.geom[1])
            plane = (g0 < gbox and self.gtype[g0] == 0) or (g1 < gbox and self.gtype[g1] == 0)
            if gbox in (g0, g1):
                if plane:
                    continue  # (the box on the floor: not a robot contact)
                kind = 2
            elif plane:
                kind = 0
            else:
                continue  # (self contacts: from the self list below)
            depth = -float(c.dist)
            near = min(near, abs(depth - TOUCH))
            if depth > TOUCH:
                out[kind][(g0, g1)] = max(depth, out[kind].get((g0, g1), 0.0))
        for i in range(d.nself):
            depth = float(d.self_depth[i])
            near = min(near, abs(depth - TOUCH))
            if depth > TOUCH:
                out[1][(int(d.self_geom[i][0]), int(d.self_geom[i][1]))] = depth
        return out, near

    def hit(self, q, box=None, kinds=7):
        p, _ = self.pairs(q, box)
        return any(p[k] for k in range(3) if kinds >> k & 1)


def _fr3(scene):
    from rcs_amd import sim as S
    from rcs_amd.envs import default_sim_gripper_cfg, default_sim_robot_cfg
    from rcs_amd.mjcf import compile_mjcf
    import rcs_oracle as O
    from rcs_env_oracle import FR3_Q_HOME

    cfg = default_sim_robot_cfg(scene)
    simu = S.Sim(cfg.mjcf_scene_path, S.SimConfig(), n_envs=2)
    robot = S.SimRobot(simu, None, cfg)
    S.SimGripper(simu, default_sim_gripper_cfg())
    cm = compile_mjcf(cfg.mjcf_scene_path)
    arm = [f"fr3_joint{i}_0" for i in range(1, 8)]
    osim = O.Sim(cm, arm, arm, "attachment_site_0", "base_0", FR3_Q_HOME, None, "finger_joint1_0", "actuator8_0")
    return simu, robot, OracleCollider(osim), cm, np.asarray(FR3_Q_HOME)


def _xarm7_pick():
    from rcs_amd import sim as S
    from rcs_amd.envs import xarm7_pick_sim_gripper_cfg, xarm7_pick_sim_robot_cfg
    from rcs_amd.mjcf import compile_mjcf
    import rcs_oracle as O
    from rcs_env_oracle import XARM7_PICK

    cfg = xarm7_pick_sim_robot_cfg()
    simu = S.Sim(cfg.mjcf_scene_path, S.SimConfig(), n_envs=2)
    robot = S.SimRobot(simu, None, cfg)
    S.SimGripper(simu, xarm7_pick_sim_gripper_cfg())
    cm = compile_mjcf(cfg.mjcf_scene_path)
    R = XARM7_PICK
    tcp = O.Pose(translation=np.array([0.0, 0.0, 0.1034]))
    osim = O.Sim(cm, R["joints"], R["actuators"], R["site"], R["base"], R["q_home"], tcp, R["gripper_joint"], R["gripper_actuator"],
                 arm_collision_geoms=[], gripper_cfg=R["gripper_cfg"])
    return simu, robot, OracleCollider(osim), cm, np.asarray(R["q_home"])


def _random_rows(cm, robot, m, rng, finger_hi=0.04):
    nl = int(cm.nq)
    lo, hi = cm.jnt_range[:nl, 0].copy(), cm.jnt_range[:nl, 1].copy()
    q = rng.uniform(lo, hi, size=(m, nl))
    if nl > robot.dof:
        f = rng.uniform(0.0, finger_hi, size=m)
        q[:, robot.dof:] = f[:, None]
    return q


def _compare(robot, orc, q, boxes=None, kinds=7):
    """Point query vs the oracle on rows q (boxes: [M, 7] or None): returns (mismatching rows, excluded rows near the bar)."""
    fq = None if boxes is None else np.ascontiguousarray(boxes)
    hit, kh, pair = robot.check_collision(q, free_qpos=fq, kinds=kinds)
    bad, excluded = [], 0
    for i in range(q.shape[0]):
        p, near = orc.pairs(q[i], None if boxes is None else boxes[i])
        okinds = sum(1 << k for k in range(3) if (kinds >> k & 1) and p[k])
        if near < BAND:
            excluded += 1
            continue
        if bool(hit[i]) != (okinds != 0) or int(kh[i]) != okinds:
            bad.append((i, int(kh[i]), okinds))
            continue
        if okinds:
            allp = {frozenset(k) for kk in range(3) if kinds >> kk & 1 for k in p[kk]}
            if frozenset(int(x) for x in pair[i]) not in allp:
                bad.append((i, "pair", tuple(pair[i]), sorted(tuple(sorted(a)) for a in allp)))
        elif tuple(pair[i]) != (-1, -1):
            bad.append((i, "pair without hit", tuple(pair[i])))
    return bad, excluded


def _hand_rows(orc, home, names):
    """Rows that must hit (found by deterministic scans against the oracle) and the reset pose that must not."""
    rows = []
    # the arm driven into the floor: shoulder forward, elbow folded down
    for j2 in np.linspace(0.6, 1.76, 30):
        q = np.concatenate([home, [0.04, 0.04]])
        q[1], q[3] = j2, -0.3
        p, _ = orc.pairs(q)
        if p[0]:
            rows.append(q)
            break
    # a folded arm with the hand against links 1-2
    link12 = {g for g, n in enumerate(names) if n and any(s in n for s in ("link1", "link2"))}
    found = False
    for j4 in np.linspace(-3.07, -2.5, 12):
        for j6 in np.linspace(0.0, 3.75, 40):
            for j2 in (-1.76, -1.2, 0.0, 1.0):
                q = np.concatenate([home, [0.04, 0.04]])
                q[1], q[3], q[5] = j2, j4, j6
                p, _ = orc.pairs(q)
                if any((a in link12) != (b in link12) for a, b in p[1]):
                    rows.append(q)
                    found = True
                    break
            if found:
                break
        if found:
            break
    # fingers pressed into each other (slides below their range)
    q = np.concatenate([home, [-0.002, -0.002]])
    rows.append(q)
    must_hit = len(rows)
    rows.append(np.concatenate([home, [0.0, 0.0]]))  # the reset pose: pads touching at a gap of exactly 0.0
    return np.array(rows), must_hit


def test_point_parity_fr3_empty_world():
    simu, robot, orc, cm, home = _fr3("fr3_empty_world")
    rng = np.random.default_rng(0)
    q = _random_rows(cm, robot, 4096, rng)
    bad, excluded = _compare(robot, orc, q)
    assert not bad, bad[:10]
    assert excluded < 0.01 * len(q), excluded
    print("fr3_empty_world: rows excluded near the bar:", excluded)
    hand, must_hit = _hand_rows(orc, home, cm.geom_names)
    assert must_hit >= 3, "a hand-made row could not be constructed"
    hit, kh, pair = robot.check_collision(hand)
    assert hit[:must_hit].all(), (hit, kh, pair)
    assert not hit[must_hit], "the reset pose (pads touching at 0.0) is no contact"
    assert kh[0] & 1 and kh[1] & 2 and kh[2] & 2
    bad, _ = _compare(robot, orc, hand)
    assert not bad, bad
    # [M, narm] + finger_qpos is the same query
    h2, k2, p2 = robot.check_collision(q[:64, :7], finger_qpos=q[:64, 7])
    h1, k1, p1 = robot.check_collision(q[:64])
    assert (h1 == h2).all() and (k1 == k2).all() and (p1 == p2).all()


def _boxes(rng, m, home_site=(0.45, 0.0)):
    b = np.zeros((m, 7))
    b[:, 0] = home_site[0] + rng.uniform(-0.25, 0.25, m)
    b[:, 1] = home_site[1] + rng.uniform(-0.25, 0.25, m)
    b[:, 2] = rng.uniform(0.0, 0.6, m)
    qu = rng.normal(size=(m, 4))
    b[:, 3:] = qu / np.linalg.norm(qu, axis=1, keepdims=True)
    return b


def test_point_parity_pick_up_every_kinds_mask():
    simu, robot, orc, cm, home = _fr3("fr3_simple_pick_up")
    rng = np.random.default_rng(1)
    m = 768
    q = _random_rows(cm, robot, m, rng)
    boxes = _boxes(rng, m)
    # boxes resting against the pads: the box placed where the fingertips are
    qp = np.tile(np.concatenate([home, [0.02, 0.02]]), (64, 1))
    qp[:, 7:] = rng.uniform(0.0, 0.04, (64, 1))
    pose = robot.get_ik().forward(np.tile(home, (simu.n_envs, 1)))[0]
    bp = np.zeros((64, 7))
    bp[:, :3] = pose[:3] + rng.uniform(-0.03, 0.03, (64, 3))
    bp[:, 3] = 1.0
    q = np.concatenate([q, qp])
    boxes = np.concatenate([boxes, bp])
    hits_box = 0
    for kinds in range(8):
        bad, excluded = _compare(robot, orc, q, boxes, kinds)
        assert not bad, (kinds, bad[:10])
        assert excluded < 0.01 * len(q), (kinds, excluded)
        if kinds == 4:
            hits_box = int(robot.check_collision(q, boxes, kinds=4)[0].sum())
    assert hits_box > 0, "no row touched the box"
    # without a pose the free body is not tested
    h_none, kh_none, _ = robot.check_collision(q, None)
    assert not (kh_none & 4).any()


def test_point_parity_xarm7_pick_world():
    simu, robot, orc, cm, home = _xarm7_pick()
    rng = np.random.default_rng(2)
    q = _random_rows(cm, robot, 1024, rng, finger_hi=0.85 if cm.jnt_range[robot.dof, 1] > 0.1 else 0.04)
    boxes = _boxes(rng, 1024, (0.4, 0.0))
    for kinds in (7, 3, 1, 2, 4):
        bad, excluded = _compare(robot, orc, q, boxes, kinds)
        assert not bad, (kinds, bad[:10])
        assert excluded < 0.01 * len(q), (kinds, excluded)


def _segments(cm, robot, home, rng, n):
    nl = int(cm.nq)
    lo, hi = cm.jnt_range[:nl, 0], cm.jnt_range[:nl, 1]
    a = np.zeros((n, nl))
    b = np.zeros((n, nl))
    k = n // 4
    base = np.concatenate([home, [0.04, 0.04]])
    # short, near home
    a[:k] = base + rng.uniform(-0.2, 0.2, (k, nl)) * np.r_[np.ones(7), 0, 0]
    b[:k] = a[:k] + rng.uniform(-0.1, 0.1, (k, nl)) * np.r_[np.ones(7), 0, 0]
    # long, anywhere
    a[k:2 * k] = rng.uniform(lo, hi, (k, nl))
    b[k:2 * k] = rng.uniform(lo, hi, (k, nl))
    # into the floor: shoulder forward, elbow down
    a[2 * k:3 * k] = base
    b[2 * k:3 * k] = base
    b[2 * k:3 * k, 1] = rng.uniform(1.2, 1.76, k)
    b[2 * k:3 * k, 3] = rng.uniform(-1.0, -0.07, k)
    # fingers closing onto each other (the pick-up test closes them onto the box too: _closing_onto_box)
    a[3 * k:] = base + rng.uniform(-0.3, 0.3, (n - 3 * k, nl)) * np.r_[np.ones(7), 0, 0]
    b[3 * k:] = a[3 * k:]
    b[3 * k:, 7:] = -0.003
    return np.clip(a, lo - 0.01, hi + 0.01), np.clip(b, lo - 0.01, hi + 0.01)


def _check_motion(robot, orc, a, b, boxes=None, res_q=1e-3):
    """check_motion vs the oracle sampled at 1001 evenly spaced points of every segment (the box, if any, at its row's pose):
    0 rows have no oracle contact; every t_contact is in contact; a contact lasting >= 5 % of a segment is never reported as
    undecided (2) and, on a contact row, is found no later than one resolution step after the oracle's first sample of it."""
    result, tc = robot.check_motion(a, b, resolution=res_q, free_qpos=boxes)
    assert set(np.unique(result)) <= {0, 1, 2}
    ts = np.linspace(0.0, 1.0, 1001)
    late = 0
    for i in range(len(a)):
        d = b[i] - a[i]
        box = None if boxes is None else boxes[i]
        hits = [orc.hit(a[i] + t * d if t < 1.0 else b[i], box) for t in ts]
        first = next((j for j, h in enumerate(hits) if h), None)
        longest, run = 0, 0
        for h in hits:
            run = run + 1 if h else 0
            longest = max(longest, run)
        if result[i] == 0:
            assert first is None, (i, "certified free, oracle contact at", ts[first])
        elif result[i] == 1:
            assert 0.0 <= tc[i] <= 1.0
            assert orc.hit(b[i] if tc[i] == 1.0 else a[i] + tc[i] * d, box), (i, tc[i])
            if first is not None:
                run = 0
                while first + run < len(hits) and hits[first + run]:
                    run += 1
                step = res_q / max(np.abs(d).max(), 1e-12)
                if run >= 50 and tc[i] > ts[first] + step + 1e-3:
                    late += 1
        else:
            assert longest < 50, (i, "undecided, oracle contact over", longest, "samples")
    assert late == 0, late
    print("motion results (free, contact, undecided):", np.bincount(result, minlength=3))
    return result, tc


def test_motion_soundness_fr3_empty_world():
    simu, robot, orc, cm, home = _fr3("fr3_empty_world")
    rng = np.random.default_rng(3)
    a, b = _segments(cm, robot, home, rng, 2048)
    _check_motion(robot, orc, a, b)


def _closing_onto_box(orc, cm, home, rng, n):
    """Segments that close the open hand onto a box held between its fingers (arm near home), and the boxes' poses: the box at the
    fingertips' centre, a few millimetres off, turned about the vertical by a random angle."""
    q = np.concatenate([home, [0.04, 0.04]])
    orc.pairs(q)
    d = orc.d
    lf, rf, hand = (cm.name2id("body", x) for x in ("left_finger_0", "right_finger_0", "hand_0"))
    mid = 0.5 * (np.array(d.xpos[lf][:]) + np.array(d.xpos[rf][:]))
    hz = np.array(d.xmat[hand][:]).reshape(3, 3)[:, 2]
    centre = mid + 0.045 * hz
    a = np.tile(q, (n, 1))
    a[:, :7] += rng.uniform(-0.01, 0.01, (n, 7))
    b = a.copy()
    b[:, 7:] = rng.uniform(-0.002, 0.01, (n, 1))
    boxes = np.zeros((n, 7))
    boxes[:, :3] = centre + rng.uniform(-0.005, 0.005, (n, 3))
    yaw = rng.uniform(0, np.pi, n)
    boxes[:, 3], boxes[:, 6] = np.cos(yaw / 2), np.sin(yaw / 2)
    return a, b, boxes


def test_motion_soundness_pick_up_with_box():
    simu, robot, orc, cm, home = _fr3("fr3_simple_pick_up")
    rng = np.random.default_rng(7)
    a1, b1 = _segments(cm, robot, home, rng, 1536)
    boxes1 = _boxes(rng, 1536)
    a2, b2, boxes2 = _closing_onto_box(orc, cm, home, rng, 512)
    a, b, boxes = np.concatenate([a1, a2]), np.concatenate([b1, b2]), np.concatenate([boxes1, boxes2])
    result, tc = _check_motion(robot, orc, a, b, boxes)
    # the hand closing onto the box: contacts with the box found (kind 2 at t_contact)
    closing = result[1536:]
    assert (closing == 1).sum() > 100, np.bincount(closing, minlength=3)
    q = a2 + tc[1536:, None] * (b2 - a2)
    _, kh, _ = robot.check_collision(q[closing == 1], boxes2[closing == 1])
    assert (kh & 4).any()


def test_motion_work_is_bounded():
    """Segments that can never be certified and never touch (the pads touching at exactly 0.0 all along) at a resolution far below
    what the budget of evaluations reaches: the call returns, undecided, in bounded time."""
    import time

    simu, robot, orc, cm, home = _fr3("fr3_empty_world")
    rng = np.random.default_rng(8)
    n = 256
    a = np.tile(np.concatenate([home, [0.0, 0.0]]), (n, 1))
    a[:, :7] += rng.uniform(-0.2, 0.2, (n, 7))
    b = a.copy()
    b[:, :7] += rng.uniform(-0.5, 0.5, (n, 7))
    t0 = time.perf_counter()
    result, tc = robot.check_motion(a, b, resolution=1e-12)
    dt = time.perf_counter() - t0
    print("uncertifiable segments at resolution 1e-12:", np.bincount(result, minlength=3), f"{dt:.3f} s")
    assert dt < 60.0
    for i in np.flatnonzero(result == 1):
        assert orc.hit(a[i] + tc[i] * (b[i] - a[i]))
    assert (result != 0).all()


def test_motion_slides_beyond_their_stroke_are_not_certified():
    """The levers hold while the finger slides stay within the stroke they were built for: fingers opened past it are never
    reported free (the same segments with the fingers inside it are)."""
    simu, robot, orc, cm, home = _fr3("fr3_empty_world")
    rng = np.random.default_rng(9)
    n = 256
    a = np.tile(np.concatenate([home, [0.04, 0.04]]), (n, 1))
    a[:, :7] += rng.uniform(-0.1, 0.1, (n, 7))
    b = a.copy()
    b[:, :7] += rng.uniform(-0.1, 0.1, (n, 7))
    r_in, _ = robot.check_motion(a, b)
    assert (r_in == 0).mean() > 0.5
    a[:, 7:] = b[:, 7:] = 0.06
    r_out, _ = robot.check_motion(a, b)
    assert (r_out != 0).all(), np.bincount(r_out, minlength=3)


def test_zero_free_body_quaternion_is_the_identity():
    """mju_normalize4: a quaternion of (near) zero norm becomes the identity."""
    simu, robot, orc, cm, home = _fr3("fr3_simple_pick_up")
    rng = np.random.default_rng(10)
    q = _random_rows(cm, robot, 256, rng)
    boxes = _boxes(rng, 256)
    boxes[:, 3:] = [1.0, 0.0, 0.0, 0.0]
    zero = boxes.copy()
    zero[:, 3:] = 0.0
    for x, y in zip(robot.check_collision(q, boxes), robot.check_collision(q, zero)):
        assert np.array_equal(x, y)


def test_scene_with_an_untested_geom_type_is_refused():
    """A colliding sphere on the hand: the collision queries could not be exact -- refused (RCSH_ERR_MODEL -> RuntimeError)."""
    import shutil
    import xml.etree.ElementTree as ET

    from parity_util import SCENE, scratch_dir
    from rcs_amd import sim as S
    from rcs_amd.envs import default_sim_gripper_cfg, default_sim_robot_cfg

    path = os.path.join(scratch_dir(), "rcs_amd_fr3_sphere", "scene.xml")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    tree = ET.parse(SCENE)
    hand = next(bd for bd in tree.getroot().iter("body") if bd.get("name") == "hand_0")
    ET.SubElement(hand, "geom", {"name": "extra_sphere", "type": "sphere", "size": "0.02", "pos": "0 0 0.05"})
    tree.write(path)
    for extra in ("collision_vertices.npz", "render_hulls.npz"):
        if os.path.exists(os.path.join(os.path.dirname(SCENE), extra)):
            shutil.copy(os.path.join(os.path.dirname(SCENE), extra), os.path.dirname(path))
    cfg = default_sim_robot_cfg("fr3_empty_world")
    cfg.mjcf_scene_path = cfg.kinematic_model_path = path
    try:
        simu = S.Sim(path, S.SimConfig(), n_envs=1)
    except RuntimeError:
        return  # (refused at creation already)
    robot = S.SimRobot(simu, None, cfg)
    S.SimGripper(simu, default_sim_gripper_cfg())
    with pytest.raises(RuntimeError):
        robot.check_collision(np.zeros((4, 9)))
    with pytest.raises(RuntimeError):
        robot.check_motion(np.zeros((4, 9)), np.zeros((4, 9)))


def test_motion_certificate_does_work():
    simu, robot, orc, cm, home = _fr3("fr3_empty_world")
    rng = np.random.default_rng(4)
    n = 1024
    base = np.concatenate([home, [0.04, 0.04]])
    a = np.tile(base, (n, 1))
    a[:, :7] += rng.uniform(-0.15, 0.15, (n, 7))
    b = a.copy()
    b[:, :7] += rng.uniform(-0.3, 0.3, (n, 7))
    result, _ = robot.check_motion(a, b, resolution=1e-3)
    frac = float((result == 0).mean())
    print("certified free near home:", frac, np.bincount(result, minlength=3))
    assert frac >= 0.9, np.bincount(result, minlength=3)


def test_queries_leave_the_simulation_untouched():
    simu, robot, orc, cm, home = _fr3("fr3_simple_pick_up")
    rng = np.random.default_rng(5)
    simu.step(20)
    q = _random_rows(cm, robot, 256, rng)
    boxes = _boxes(rng, 256)
    s0 = simu.get_state().copy()
    r1 = robot.check_collision(q, boxes)
    m1 = robot.check_motion(q[:128], q[128:], free_qpos=boxes[:128])
    assert (simu.get_state() == s0).all()
    r2 = robot.check_collision(q, boxes)
    m2 = robot.check_motion(q[:128], q[128:], free_qpos=boxes[:128])
    for x, y in zip(r1 + m1, r2 + m2):
        assert np.array_equal(x, y)
    assert (simu.get_state() == s0).all()


def test_headline_rollout_bit_identical_with_queries_between_steps():
    from parity_util import make_vec_env, synthetic_actions

    runs = []
    for with_queries in (False, True):
        venv = make_vec_env(64, True)
        robot = venv.robot
        joints, grip = synthetic_actions(64, 100, 0)
        venv.reset()
        rng = np.random.default_rng(6)
        out = []
        for t in range(100):
            if with_queries:
                q = np.concatenate([rng.uniform(-1, 1, (32, 7)), np.full((32, 2), 0.02)], axis=1)
                robot.check_collision(q)
                robot.check_motion(q[:16], q[16:])
            obs, rew, term, trunc, info = venv.step({"joints": joints[t], "gripper": grip[t]})
            out.append((venv.sim.qpos.copy(), venv.sim.qvel.copy(), {k: np.asarray(v).copy() for k, v in info.items()}))
        runs.append(out)
    for (qa, va, ia), (qb, vb, ib) in zip(*runs):
        assert np.array_equal(qa, qb) and np.array_equal(va, vb)
        for k in ia:
            assert np.array_equal(ia[k], ib[k]), k


def test_errors_leave_state_untouched():
    simu, robot, orc, cm, home = _fr3("fr3_simple_pick_up")
    L, h = simu._L, simu._h
    s0 = simu.get_state().copy()
    q = np.tile(np.concatenate([home, [0.02, 0.02]]), (4, 1))
    hit = np.zeros(4, dtype=np.uint8)
    res = np.zeros(4, dtype=np.int32)
    tc = np.zeros(4)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.rcsh_collision_query(h, None, None, 4, 7, P(hit), None, None) != 0
    assert L.rcsh_collision_query(h, P(q), None, 4, 7, None, None, None) != 0
    assert L.rcsh_collision_query(h, P(q), None, -1, 7, P(hit), None, None) != 0
    assert L.rcsh_collision_query(h, P(q), None, 4, 8, P(hit), None, None) != 0
    bad = q.copy()
    bad[2, 3] = np.nan
    assert L.rcsh_collision_query(h, P(bad), None, 4, 7, P(hit), None, None) != 0
    assert L.rcsh_motion_query(h, P(q), P(q), None, 4, 7, 0.0, P(res), P(tc)) != 0
    assert L.rcsh_motion_query(h, P(q), P(q), None, 4, 7, -1.0, P(res), P(tc)) != 0
    assert L.rcsh_motion_query(h, P(q), None, None, 4, 7, 1e-3, P(res), P(tc)) != 0
    assert L.rcsh_motion_query(h, P(q), P(bad), None, 4, 7, 1e-3, P(res), P(tc)) != 0
    assert L.rcsh_collision_query(h, P(q), None, 0, 7, P(hit), None, None) == 0
    assert L.rcsh_motion_query(h, P(q), P(q), None, 0, 7, 1e-3, P(res), P(tc)) == 0
    with pytest.raises(ValueError):
        robot.check_collision(bad)
    with pytest.raises(ValueError):
        robot.check_motion(q, q, resolution=0.0)
    assert (simu.get_state() == s0).all()
    hit0, kh0, pair0 = robot.check_collision(np.zeros((0, 9)))
    assert hit0.shape == (0,)
