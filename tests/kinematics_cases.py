"""Edge cases of the Cartesian path (csrc/ik_team.h, csrc/pose.h, cart_prepare in csrc/sim_kernels.h), built from the oracle alone.

Inverse-kinematics rows (`inverse_cases`), per robot and seeded:
  * wide     -- targets `forward(q)` with q uniform over the middle 90 % of every joint's range, half of them started from home and half
                from an equally drawn configuration: long runs, runs to the iteration cap, large arguments of the sine;
  * near_pi  -- the start frame turned by angles inside [pi - 1e-2, pi) and just below that band about seven axes, five of them with zero
                components: the near-pi branch of the SO(3) log, whose signs come from off-diagonal comparisons.  There a component
                of the rotation vector is the square root of a difference that is zero but for round-off: 0 or 2e-8, as the last bits
                fall, in any implementation.  The 5- and 6-dof arms contract that away; a 7-dof arm keeps it in its null space for good
                (measured on the FR3, rotation about x by pi - 9.9e-3: the kernel's solution 2.2e-8 from the oracle's, whose twins
                agree with each other -- a nudge of 1e-13 moves the axis' zero components by 1e-13 and their squares by 1e-26, far below
                the round-off).  These rows (`q_exempt`) run on every robot and are held to everything but q on the 7-dof arms;
  * small    -- rotation errors of 0, around kTaylor (the series branch of log6 / Jlog6) and 1e-3 with a translation of 3 cm;
  * far      -- targets out of reach: 1000 iterations, no success;
  * edge     -- targets on rays from the start pose, bisected (by the oracle's own success) onto the edge of what the iteration reaches:
                the last rows inside it converge slowly, in 150 to 500 iterations, the first rows outside it run to the cap with an error
                just above the threshold.  (Wide rows that take this long wander before they converge, and no twin follows them.)

The CLIK is an iteration whose result can depend on the last bit of its input (a target at the edge of the workspace converges or does not;
a 7-dof arm's solution keeps the path's null-space component).  A row is therefore KEPT for the comparison at the project's 1e-9 only if
the oracle reproduces itself on it: three runs, from q0 and from q0 +- 1e-13 on every joint, agree on success, on the iteration count and
on q within 1e-11 (the solution, or the iterate a failed run stopped at) -- the "twin nudged by 1e-13, 100 x" convention of parity_util's many-contact test.  Dropped rows
are still sent to the kernel; tests/test_kinematics_cases_cpu.py bounds how many the filter may drop and which classes must survive it.

Env-level cases (`limit_case`): Cartesian env-steps whose actions exceed the step limits (0.2 m / 45 deg), equal them, stay below them,
and whose accumulated offset crosses the workspace clamp, each environment mirrored by an oracle environment and an oracle twin.
"""

from __future__ import annotations

import functools
import math

import numpy as np

ROBOTS = ("fr3", "xarm7", "arm6", "so101")
K_TAYLOR = 1.220703125e-4   # kTaylor (csrc/ik.h): eps^(1/4), the series branches of log6 / Jlog6 lie below it
NEAR_PI = 1e-2              # the near-pi branch of the SO(3) log: angle >= pi - 1e-2
TWIN_NUDGE = 1e-13          # rad on every arm joint: the twins of an oracle run
TWIN_TOL = 1e-11            # 100 x the nudge: twins further apart than this have parted
N_WIDE = 200
SEED = 4                    # of the drawn rows; chosen so that every condition of tests/test_kinematics_cases_cpu.py holds on every robot
QUICK_ITERATIONS = 60       # a "quick" row: converges within this many iterations (the small class takes 55 on the 6- and 7-dof arms)

_AXES = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 1.0, 0.0], [0.0, 1.0, -1.0], [1.0, -2.0, 3.0], [-1.0, 1.0, 1.0]])
_AXES /= np.linalg.norm(_AXES, axis=1, keepdims=True)
# inside the band (at least 1e-6 away from pi, where round-off decides the signs in any implementation) and just below it
_NEAR_PI_GAPS = (NEAR_PI - 1e-4, 3e-3, 1e-3, 1e-4, 1e-5, NEAR_PI + 1e-4, 2 * NEAR_PI)
_SMALL_ANGLES = (0.5 * K_TAYLOR, (1 - 1e-4) * K_TAYLOR, (1 + 1e-4) * K_TAYLOR, 2 * K_TAYLOR, 1e-3)
_SMALL_SHIFTS = np.array([[0.03, 0.0, 0.0], [0.0, -0.03, 0.0], [0.0, 0.0, 0.03], [0.02, 0.02, -0.01], [-0.02, 0.01, 0.02]])
_EDGE_RAYS = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, -1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0]])
_EDGE_LEVELS = 26           # bisection steps from a bracket of 1.5 m: the last rows lie 2e-8 m from the edge, far above round-off
_FAR = np.array([[3.0, 0.0, 0.5], [0.0, -2.5, 0.3], [0.5, 0.5, 2.5], [-1.5, 1.5, -1.0], [1.2, -1.2, 0.2], [0.0, 0.0, -1.5]])


# ---------------------------------------------------------------------------------------------------------------- the oracle side
@functools.lru_cache(maxsize=None)
def oracle_env(robot: str):
    """One oracle environment of the robot, reset: its `sim.ik_forward` / `sim.ik_inverse` are Pin::forward / Pin::inverse."""
    from parity_util import make_oracle_envs

    o = make_oracle_envs(1, True, gripper=False, relative=False, robot=robot)[0]
    o.reset()
    return o


def tcp_offset(robot: str):
    """The tool offset the Kinematics calls are given: the Franka hand's on the FR3, none on the others (oracle Pose)."""
    import rcs_oracle as O

    return O.franka_hand_tcp_offset() if robot == "fr3" else O.Pose()


def vec7(pose) -> np.ndarray:
    return np.concatenate([pose.translation(), pose.rotation_q()])


def _axis_angle_pose(axis, angle, shift=(0.0, 0.0, 0.0)):
    import rcs_oracle as O

    a = np.asarray(axis, dtype=np.float64)
    return O.Pose(translation=np.asarray(shift, dtype=np.float64), quaternion=np.concatenate([a * math.sin(0.5 * angle), [math.cos(0.5 * angle)]]))


def _draw_q(rng, low, high, share=0.9):
    mid, half = 0.5 * (low + high), 0.5 * (high - low)
    return mid + share * half * rng.uniform(-1.0, 1.0, size=low.shape)


@functools.lru_cache(maxsize=None)
def inverse_cases(robot: str) -> dict:
    """The rows of one robot: `target` [N, 7] (TCP targets of Kinematics.inverse), `q0` [N, dof], `cls` [N] and `angle0` [N], the
    angle of the rotation error the iteration starts from (frame(q0)^-1 * target * tcp^-1); `q_exempt` [N]: the near-pi rows about an
    axis with zero components on a 7-dof arm, whose q no two implementations share (module docstring)."""
    import rcs_oracle as O

    o, tcp = oracle_env(robot), tcp_offset(robot)
    low, high, home = np.asarray(o.robot["low"], float), np.asarray(o.robot["high"], float), np.asarray(o.robot["q_home"], float)
    rng = np.random.default_rng(1000 * SEED + ROBOTS.index(robot))
    target, q0, cls, q_exempt = [], [], [], []

    def add(t7, start, name, exempt=False):
        target.append(np.asarray(t7, dtype=np.float64)); q0.append(np.asarray(start, dtype=np.float64)); cls.append(name)
        q_exempt.append(exempt)

    for i in range(N_WIDE):
        add(vec7(o.sim.ik_forward(_draw_q(rng, low, high), tcp)), home if i % 2 == 0 else _draw_q(rng, low, high), "wide")
    frame0 = o.sim.ik_forward(home, None)  # the IK frame at home; inverse() aims the frame at target * tcp^-1 (quirk Q7)
    for a, axis in enumerate(_AXES):
        for gap in _NEAR_PI_GAPS:
            shift = (0.0, 0.0, 0.0) if a % 2 == 0 else (0.02, -0.03, 0.01)
            add(vec7(frame0 * _axis_angle_pose(axis, math.pi - gap, shift) * tcp), home, "near_pi",
                exempt=len(home) == 7 and bool(np.any(axis == 0.0)) and gap <= NEAR_PI)
    start = vec7(frame0 * tcp)
    for s, shift in enumerate(_SMALL_SHIFTS):
        # a pure translation: the target's quaternion is the start pose's, bit for bit
        add(np.concatenate([start[:3] + shift, start[3:]]), home, "small")
        for angle in _SMALL_ANGLES:
            add(vec7(frame0 * _axis_angle_pose(_AXES[(s + 2) % len(_AXES)], angle, shift) * tcp), home, "small")
    for f, far in enumerate(_FAR):
        add(np.concatenate([far, start[3:] if f % 2 == 0 else vec7(_axis_angle_pose(_AXES[f], 1.0))[3:]]), home, "far")
    for r, ray in enumerate(_EDGE_RAYS):
        # (the 5-dof arm holds the start's orientation only in its own plane: up and down)
        ray = ray if robot != "so101" else _EDGE_RAYS[r % 2]
        q_start = home if r >= 5 else _draw_q(rng, low, high)
        inside, outside, lo, hi = [], [], 0.0, 1.5
        for _ in range(_EDGE_LEVELS):
            mid = 0.5 * (lo + hi)
            t7 = np.concatenate([start[:3] + mid * ray, start[3:]])
            if o.sim.ik_inverse(O.Pose(translation=t7[:3], quaternion=t7[3:]), q_start, tcp)[0] is not None:
                lo = mid; inside.append(t7)
            else:
                hi = mid; outside.append(t7)
        for t7 in inside[-6:] + outside[-2:]:
            add(t7, q_start, "edge")
    target, q0, cls = np.array(target), np.array(q0), np.array(cls)
    inv_tcp = tcp.inverse()
    angle0 = np.array([(o.sim.ik_forward(q, None).inverse() * O.Pose(translation=t[:3], quaternion=t[3:]) * inv_tcp).total_angle()
                       for t, q in zip(target, q0)])
    return {"target": target, "q0": q0, "cls": cls, "angle0": angle0, "q_exempt": np.array(q_exempt)}


@functools.lru_cache(maxsize=None)
def classified_cases(robot: str) -> dict:
    """`inverse_cases` with the oracle's answer (`ok`, `iters`, `q` [N, nq], zero on failed rows), `kept`: the twin rule, and
    `kept_counts`: `kept`, plus the `q_exempt` rows whose three runs agree on success and on the iteration count."""
    import rcs_oracle as O

    c = dict(inverse_cases(robot))
    o, tcp = oracle_env(robot), tcp_offset(robot)
    n = len(c["cls"])
    ok, iters, kept, counts = np.zeros(n, dtype=bool), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    q = np.zeros((n, o.sim.model.njnt))
    for r in range(n):
        pose = O.Pose(translation=c["target"][r, :3], quaternion=c["target"][r, 3:])
        runs = [o.sim.ik_inverse_last(pose, c["q0"][r] + d, tcp) for d in (0.0, TWIN_NUDGE, -TWIN_NUDGE)]
        ok[r], q_r, iters[r] = runs[0]
        if ok[r]:
            q[r] = q_r
        # (a failed run's last iterate counts too: three runs that wander for 1000 iterations agree on "failed, 1000" without
        # following each other, and a fourth implementation may well converge -- the oracle keeps the iterate for this)
        # (... except out of reach, where nothing can converge and the iterates run off by hundreds of radians)
        settled = c["cls"][r] != "far" or ok[r]
        kept[r] = all(ok_t == ok[r] and it_t == iters[r] and (not settled or np.abs(q_t - q_r).max() <= TWIN_TOL) for ok_t, q_t, it_t in runs[1:])
        counts[r] = all(ok_t == ok[r] and it_t == iters[r] for ok_t, _, it_t in runs[1:])
    c.update(ok=ok, iters=iters, q=q, kept=kept & ~c["q_exempt"], kept_counts=kept | (c["q_exempt"] & counts))
    return c


def wavefront_layout(robot: str) -> np.ndarray:
    """Row indices into `classified_cases`, 4 k + 3 of them, so that the kernel's last wavefront has a team without a target.  A
    wavefront is four consecutive rows; it iterates until its four teams are done.  Every row appears; every wavefront but one begins
    with a kept row that FAILS (1000 iterations) and a kept row that converges quickly (the small class: 55 iterations on the 6- and
    7-dof arms), which have to stay put for the hundreds of iterations their neighbours go on; the failing and quick rows repeat
    (the oracle ran each once).  The last full wavefront consists of failing rows only."""
    c = classified_cases(robot)
    n = len(c["cls"])
    fail = np.flatnonzero(c["kept"] & ~c["ok"])
    quick = np.flatnonzero(c["kept"] & c["ok"] & (c["iters"] <= QUICK_ITERATIONS))
    if len(quick) == 0:  # (the 5-dof arm reaches none of the small targets: its kept rows with the fewest iterations)
        good = np.flatnonzero(c["kept"] & c["ok"])
        quick = good[np.argsort(c["iters"][good], kind="stable")[:8]]
    assert len(fail) >= 4 and len(quick) >= 1, (robot, len(fail), len(quick))
    rows = []
    for w, first in enumerate(range(0, n - n % 2, 2)):
        rows += [fail[w % len(fail)], quick[w % len(quick)], first, first + 1]
    if n % 2:
        rows += [fail[0], quick[0], n - 1, fail[1]]
    rows += list(fail[-4:])
    rows += [fail[2 % len(fail)], quick[-1], int(np.flatnonzero(c["cls"] == "wide")[0])]
    return np.array(rows, dtype=np.int64)


# ------------------------------------------------------------------------------------------------------------- forward kinematics
N_FK = 128


@functools.lru_cache(maxsize=None)
def fk_configs(robot: str) -> np.ndarray:
    """[N_FK, dof] joint configurations over each joint's WHOLE range (the xArm7's reach +- 2 pi), home and both corners first."""
    o = oracle_env(robot)
    low, high, home = np.asarray(o.robot["low"], float), np.asarray(o.robot["high"], float), np.asarray(o.robot["q_home"], float)
    rng = np.random.default_rng(2000 + ROBOTS.index(robot))
    return np.vstack([home, low, high, rng.uniform(low, high, size=(N_FK - 3, len(low)))])


def mat_to_quat_branch(R) -> int:
    """Which branch of mat_to_quat (csrc/pose.h; Eigen's Quaternion(Matrix3)) a rotation matrix takes: 0 the trace branch, else 1 + the
    index of the largest diagonal entry in the same comparison order (1 against 0, then 2 against the winner)."""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    if R[0, 0] + R[1, 1] + R[2, 2] > 0:
        return 0
    i = 1 if R[1, 1] > R[0, 0] else 0
    if R[2, 2] > R[i, i]:
        i = 2
    return 1 + i


def fk_branch_counts(robot: str) -> np.ndarray:
    o = oracle_env(robot)
    return np.bincount([mat_to_quat_branch(o.sim.ik_forward(q, None).rotation_m()) for q in fk_configs(robot)], minlength=4)


# ------------------------------------------------------------------------------------------- an independent anchor: log6 in numpy
def log6_norm(pose) -> float:
    """|log6| of an rcs_amd.common.Pose, from the quaternion's axis and angle and the closed form of V^-1 -- nothing of the oracle's
    matrix-based log3 / log6 is used."""
    q, p = pose.rotation_q(), pose.translation()
    if q[3] < 0:
        q = -q
    s = float(np.linalg.norm(q[:3]))
    theta = 2.0 * math.atan2(s, q[3])
    if theta < 1e-7:
        return float(np.linalg.norm(np.concatenate([p, 2.0 * q[:3]])))
    w = q[:3] / s * theta
    coef = 1.0 / theta**2 - (1.0 + math.cos(theta)) / (2.0 * theta * math.sin(theta))
    v = p - 0.5 * np.cross(w, p) + coef * np.cross(w, np.cross(w, p))
    return float(np.linalg.norm(np.concatenate([v, w])))


def residual_of_solution(robot: str, q, target7) -> float:
    """|log6(frame(q)^-1 * target * tcp^-1)| with rcs_amd.common.Pose: what Pin::inverse drives below 1e-4."""
    from rcs_amd.common import Pose

    o, tcp_o = oracle_env(robot), tcp_offset(robot)
    tcp = Pose(translation=tcp_o.translation(), quaternion=tcp_o.rotation_q())
    f = o.sim.ik_forward(np.asarray(q)[: len(o.robot["low"])], tcp_o)  # frame * tcp^-1: composed back to the frame below
    frame = Pose(translation=f.translation(), quaternion=f.rotation_q()) * tcp
    goal = Pose(translation=target7[:3], quaternion=target7[3:]) * tcp.inverse()
    return log6_norm(frame.inverse() * goal)


# ------------------------------------------------------------------------------ env steps where the limits and the clamp bind
LIMIT_ENVS, LIMIT_STEPS = 48, 12
MAX_MOV = (0.2, float(np.deg2rad(45)))
LIMIT_CONFIGS = (("fr3", "xyzrpy", "last_step"), ("fr3", "xyzrpy", "configured_origin"), ("fr3", "tquat", "last_step"),
                 ("fr3", "tquat", "configured_origin"), ("arm6", "tquat", "last_step"), ("xarm7", "xyzrpy", "configured_origin"))


def limit_actions(mode: str, relative_to: str) -> np.ndarray:
    """[LIMIT_STEPS, LIMIT_ENVS, 6 or 7] relative actions.  By class e % 6 a step's increment (translation length, rotation angle)
    0: exceeds both limits; 1: neither; 2: the translation's only; 3: the rotation's only; 4: EQUALS both limits (the comparisons are
    strict, nothing is cut); 5: exceeds both, and in tquat mode the action's quaternion is negated (w < 0: slerp's d < 0 branch).  An
    environment keeps one translation direction with z >= 0 (nobody is driven into the floor), axis-aligned in class 4 so that the
    length is 0.2 exactly.
    last_step: the increment is the action; the arm follows until the target leaves its reach, and the IK fails from then on.
    configured_origin: the action is the accumulated offset from the origin fixed at reset, and the limits apply to its CHANGE.  The
    offset goes out along the environment's direction and comes back the same way: six steps out and six back where e % 12 < 6, which
    carries the offset across the workspace clamp, two out and two back elsewhere."""
    from rcs_amd.common import Pose

    act = np.zeros((LIMIT_STEPS, LIMIT_ENVS, 6 if mode == "xyzrpy" else 7))
    for e in range(LIMIT_ENVS):
        rng = np.random.default_rng(7000 + e)
        k = e % 6
        d = rng.normal(size=3)
        d[2] = abs(d[2])
        d /= np.linalg.norm(d)
        if k == 4:
            d = np.eye(3)[(e // 6) % 3] * (-1.0 if (e // 18) % 2 and (e // 6) % 3 != 2 else 1.0)
        big_t, big_r = k in (0, 2, 5), k in (0, 3, 5)
        lengths = rng.uniform(0.25, 0.5, size=LIMIT_STEPS) if big_t else rng.uniform(0.02, 0.15, size=LIMIT_STEPS)
        if k == 4:
            lengths[:] = MAX_MOV[0]
        run = 6 if e % 12 < 6 else 2
        total, out = Pose(), []
        for t in range(LIMIT_STEPS):
            angle = rng.uniform(1.0, 1.5) if big_r else rng.uniform(0.05, 0.6)
            axis = rng.normal(size=3)
            axis /= np.linalg.norm(axis)
            if k == 4:
                angle, axis = MAX_MOV[1], np.eye(3)[t % 3]
            quat = np.concatenate([axis * math.sin(0.5 * angle), [math.cos(0.5 * angle)]])
            step = Pose(translation=d * lengths[t], quaternion=quat)
            if relative_to == "configured_origin":
                if (t // run) % 2 == 0:
                    out.append(lengths[t])
                    reach = float(np.sum(out))
                else:
                    reach = float(np.sum(out[:-1]))
                    out.pop()
                total = Pose(translation=d * reach, quaternion=(step * total).rotation_q())
                step = total
            if mode == "xyzrpy":
                act[t, e] = step.xyzrpy()
            else:
                act[t, e] = np.concatenate([step.translation(), -step.rotation_q() if k == 5 else step.rotation_q()])
    return act


_FLAGS = ("ik_success", "collision", "truncated")


def _oracle_record(oe, obs, info, truncated, dof):
    return {"qpos": np.array(oe.sim.qpos[:dof]), "target": np.array(oe.sim.s.target_angles[:dof]), "tquat": np.array(obs["tquat"]),
            "xyzrpy": np.array(obs["xyzrpy"]), "ik_success": bool(info["ik_success"]), "collision": bool(info["collision"]),
            "truncated": bool(truncated)}


@functools.lru_cache(maxsize=None)
def limit_case(robot: str, mode: str, relative_to: str) -> dict:
    """The oracle's side of one configuration: per step and environment the record of the oracle environment (`rec[t][e]`), whether its
    twin -- arm qpos moved by 1e-13 after reset -- agrees on the flags (`flags_agree` [T, E]), `split` [E]: the first step at which
    the twin differs in a flag or by more than 1e-11 (LIMIT_STEPS: never), and the counts the CPU test asserts."""
    import rcs_oracle as O
    from parity_util import make_oracle_envs, robot_dof, rpy_error

    dof = robot_dof(robot)
    act = limit_actions(mode, relative_to)
    rec = [[None] * LIMIT_ENVS for _ in range(LIMIT_STEPS)]
    flags_agree = np.zeros((LIMIT_STEPS, LIMIT_ENVS), dtype=bool)
    split = np.full(LIMIT_ENVS, LIMIT_STEPS, dtype=np.int64)
    clamped = np.zeros(LIMIT_ENVS, dtype=bool)
    cut = np.zeros((LIMIT_STEPS, LIMIT_ENVS, 2), dtype=bool)
    ik_fail = slerp_negative = 0
    from rcs_env_oracle import TRPY_HIGH, TRPY_LOW

    for e in range(LIMIT_ENVS):
        pair = make_oracle_envs(2, True, gripper=False, mode=mode, max_relative_movement=MAX_MOV, robot=robot, relative_to=relative_to)
        for oe in pair:
            oe.reset()
        for j in range(dof):  # (written into the oracle's mjData: `sim.qpos` is a copy)
            pair[1].sim.s.d.qpos[pair[1].sim.s.arm_jnt[j]] += TWIN_NUDGE
        for t in range(LIMIT_STEPS):
            last = pair[0]._last_action
            out = []
            for oe in pair:
                obs, _, _, trunc, info = oe.step({mode: act[t, e]})
                out.append(_oracle_record(oe, obs, info, trunc, dof))
            a, b = out
            rec[t][e] = a
            # which limits cut this step's change of the offset (from the wrapper's own state)
            back = last.inverse() if last is not None and relative_to == "configured_origin" else O.Pose()
            asked, applied = _action_pose(mode, act[t, e]) * back, pair[0]._last_action * back
            cut[t, e] = (np.linalg.norm(asked.translation()) > np.linalg.norm(applied.translation()) + 1e-9,
                         asked.total_angle() > applied.total_angle() + 1e-9)
            slerp_negative += int(cut[t, e, 1] and asked.rotation_q()[3] < 0)  # (slerp from the identity: d is the quaternion's w)
            unclipped = pair[0]._origin.translation() + pair[0]._last_action.translation()
            clamped[e] |= bool(np.any(unclipped < TRPY_LOW) or np.any(unclipped > TRPY_HIGH))
            ik_fail += int(not a["ik_success"])
            flags_agree[t, e] = all(a[k] == b[k] for k in _FLAGS)
            apart = max(np.abs(a["qpos"] - b["qpos"]).max(), np.abs(a["target"] - b["target"]).max(), np.abs(a["tquat"] - b["tquat"]).max(),
                        np.abs(a["xyzrpy"][:3] - b["xyzrpy"][:3]).max(), rpy_error(a["xyzrpy"][3:], b["xyzrpy"][3:]))
            if split[e] == LIMIT_STEPS and (not flags_agree[t, e] or apart > TWIN_TOL):
                split[e] = t
    return {"actions": act, "rec": rec, "flags_agree": flags_agree, "split": split, "clamped": clamped, "cut": cut, "ik_fail": ik_fail,
            "slerp_negative": slerp_negative, "dof": dof}


def _action_pose(mode, action):
    import rcs_oracle as O

    return O.Pose(translation=action[:3], rpy_vector=action[3:]) if mode == "xyzrpy" else O.Pose(translation=action[:3], quaternion=action[3:])


def limit_case_summary(case: dict) -> str:
    n = LIMIT_ENVS * LIMIT_STEPS
    cut = case["cut"]
    return (f"ik_success False in {case['ik_fail']} of {n} env-steps; clamp bound in {int(case['clamped'].sum())} environments; translation cut in "
            f"{int(cut[..., 0].sum())}, rotation cut in {int(cut[..., 1].sum())} env-steps, {case['slerp_negative']} of them from a quaternion with w < 0; twins together to the end in "
            f"{int((case['split'] == LIMIT_STEPS).sum())} of {LIMIT_ENVS} environments")


def run_limit_parity(robot: str, mode: str, relative_to: str) -> dict:
    """The HIP env against `limit_case`: largest differences over the env-steps before an environment's twins part, flag mismatches
    there, and flag mismatches after it on the steps whose twin agrees with the oracle on the flags."""
    from parity_util import make_vec_env, rpy_error
    from rcs_amd.envs import ControlMode

    case = limit_case(robot, mode, relative_to)
    dof, act = case["dof"], case["actions"]
    cm = ControlMode.CARTESIAN_TRPY if mode == "xyzrpy" else ControlMode.CARTESIAN_TQuat
    venv = make_vec_env(LIMIT_ENVS, True, gripper=False, control_mode=cm, max_relative_movement=MAX_MOV, relative_to=relative_to, robot=robot)
    rep = {"max_abs_qpos": 0.0, "max_abs_target": 0.0, "max_abs_tquat": 0.0, "max_abs_xyzrpy": 0.0, "flag_mismatches": 0,
           "late_flag_mismatches": 0, "compared": 0, "late_compared": 0}
    venv.reset()
    for t in range(LIMIT_STEPS):
        obs, _, _, trunc, info = venv.step({mode: act[t]})
        st, q = venv.robot.get_state(), venv.sim.qpos
        for e in range(LIMIT_ENVS):
            o = case["rec"][t][e]
            wrong = int(bool(info["ik_success"][e]) != o["ik_success"]) + int(bool(info["collision"][e]) != o["collision"]) + int(bool(trunc[e]) != o["truncated"])
            if t < case["split"][e]:
                rep["compared"] += 1
                rep["flag_mismatches"] += wrong
                rep["max_abs_qpos"] = max(rep["max_abs_qpos"], float(np.abs(q[e][:dof] - o["qpos"]).max()))
                rep["max_abs_target"] = max(rep["max_abs_target"], float(np.abs(st.target_angles[e] - o["target"]).max()))
                rep["max_abs_tquat"] = max(rep["max_abs_tquat"], float(np.abs(obs["tquat"][e] - o["tquat"]).max()))
                rep["max_abs_xyzrpy"] = max(rep["max_abs_xyzrpy"], float(np.abs(obs["xyzrpy"][e][:3] - o["xyzrpy"][:3]).max()),
                                            rpy_error(obs["xyzrpy"][e][3:], o["xyzrpy"][3:]))
            elif case["flags_agree"][t, e]:
                rep["late_compared"] += 1
                rep["late_flag_mismatches"] += wrong
    venv.close()
    return rep
