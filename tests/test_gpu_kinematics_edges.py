"""The Cartesian path at its edges, HIP against the oracle: the CLIK kernels (csrc/ik_team.h) on wide, near-pi, small-angle, out-of-reach
and edge-of-reach targets with failing and converging rows in one wavefront; forward kinematics over the joints' whole range;
set_cartesian_position with a mask; env-steps whose actions bind the step limits and the workspace clamp (csrc/pose.h, cart_prepare).

The cases and the rule that says which rows the oracle itself reproduces are in tests/kinematics_cases.py; what that rule may drop is
bounded in tests/test_kinematics_cases_cpu.py.  The bars are the project's: 1e-9 on joint solutions and targets, 1e-12 on poses, flags
and iteration counts exact."""

import numpy as np
import pytest

import kinematics_cases as K

pytestmark = pytest.mark.gpu

TOL = 1e-9
POSE_TOL = 1e-12


@pytest.fixture(autouse=True, params=["team"])
def kernel(request):
    """The kernel variant every test pins (rcsh_sim_set_kernel), as in test_gpu_parity.py."""
    import parity_util

    parity_util.KERNEL = request.param
    yield request.param
    parity_util.KERNEL = "auto"


@pytest.mark.parametrize("robot", K.ROBOTS)
def test_inverse_edges_match_oracle_in_mixed_wavefronts(robot):
    """Kinematics.inverse on every row of kinematics_cases, four rows to a wavefront: a row that runs to the cap, a row that is done after
    55 iterations and two others.  On the rows the oracle reproduces, success and the iteration count are the oracle's, q within 1e-9,
    the finger entries zero.  The other rows run too and are only exempt from that comparison -- but wherever the kernel reports
    success, on whatever row, its q must solve the problem: the numpy residual of kinematics_cases is below Pin's 1e-4.  Then the same
    rows in reverse order: every row's q, success and iteration count are bit for bit those of the first run, whoever its neighbours are.

    Not held to 1e-9 on q, for a reason that is no kernel bug: near-pi rotations about an axis with exactly zero components on the
    7-dof arms (`q_exempt`; measured 2.2e-8 on the FR3, argument in kinematics_cases' docstring).  They are held to everything else."""
    from parity_util import make_vec_env, robot_dof

    c, rows = K.classified_cases(robot), K.wavefront_layout(robot)
    n, dof = len(rows), robot_dof(robot)
    assert n % 4 == 3
    target, q0 = c["target"][rows], c["q0"][rows]
    kept, o_ok, o_it, o_q = c["kept_counts"][rows], c["ok"][rows], c["iters"][rows], c["q"][rows]
    q_kept = c["kept"][rows]
    tcp7 = K.vec7(K.tcp_offset(robot))
    venv = make_vec_env(n, True, gripper=False, relative=False, robot=robot)
    venv.reset()
    ik = venv.robot.get_ik()
    q, ok, it = ik.inverse(target, q0, tcp7)
    q_r, ok_r, it_r = ik.inverse(target[::-1], q0[::-1], tcp7)
    venv.close()
    good = q_kept & o_ok
    exempt_q = c["q_exempt"][rows] & ok & o_ok
    diff = np.abs(q[good][:, :dof] - o_q[good][:, :dof]).max(axis=1)
    # every success the kernel reports solves the problem (each distinct row once)
    first = np.unique(rows, return_index=True)[1]
    solved = first[ok[first]]
    residual = np.array([K.residual_of_solution(robot, q[r], target[r]) for r in solved])
    exempt_diff = np.abs(q[exempt_q][:, :dof] - o_q[exempt_q][:, :dof]).max() if exempt_q.any() else 0.0
    print(f"\n{robot}: kernel successes {len(solved)} of {len(first)} distinct rows, {int((ok & ~o_ok)[first].sum())} of them where the oracle failed "
          f"(none on a kept row), largest residual {residual.max():.9e}; q-exempt near-pi rows {int(c['q_exempt'].sum())}, their largest "
          f"|q - q_oracle| {exempt_diff:.3e}")
    print(f"{robot}: {n} rows, {int((~kept).sum())} exempt ({int((~c['kept_counts']).sum())} of {len(c['kept'])} distinct rows); on kept rows: "
          f"success mismatches {int((ok != o_ok)[kept].sum())}, iteration mismatches {int((it != o_it)[kept].sum())}, "
          f"largest |q - q_oracle| {diff.max():.3e}; failing rows {int((kept & ~o_ok).sum())}, longest success {int(o_it[good].max())}")
    assert np.array_equal(ok[kept], o_ok[kept]), np.flatnonzero(kept & (ok != o_ok))
    assert np.array_equal(it[kept], o_it[kept]), [(int(r), int(it[r]), int(o_it[r])) for r in np.flatnonzero(kept & (it != o_it))]
    assert (it[kept & ~o_ok] == 1000).all()
    assert diff.max() < TOL, (np.flatnonzero(good)[diff.argmax()], diff.max())
    assert np.all(q[:, dof:] == 0.0)
    assert residual.max() <= 1e-4 * (1 + 1e-6), (solved[residual.argmax()], residual.max())  # (1e-6: see test_kept_solutions_solve_the_problem)
    # a row's result may not depend on its neighbours
    assert np.array_equal(ok_r[::-1], ok) and np.array_equal(it_r[::-1], it)
    assert np.array_equal(q_r[::-1], q, equal_nan=True), np.flatnonzero((q_r[::-1] != q).any(axis=1))


@pytest.mark.parametrize("robot", K.ROBOTS)
def test_forward_over_the_whole_joint_range(robot):
    """Kinematics.forward with and without a tool offset at configurations over every joint's whole range -- all four branches of
    mat_to_quat, sines and cosines of angles up to 2 pi -- within 1e-12 of the oracle, the quaternion compared raw (its sign is part of the
    API).  get_cartesian_position reports the same poses once the configurations are written with set_joints_hard and the kinematics
    refreshed by a substep (as in the reference, the site's placement is the last position stage's, i.e. of the joints before the
    substep's integration) -- also at the configurations in which the arm touches itself or the floor."""
    import rcs_oracle as O
    from parity_util import make_oracle_envs, make_vec_env

    cfgs = K.fk_configs(robot)
    n = len(cfgs) + 3
    qs = np.resize(cfgs, (n, cfgs.shape[1]))
    o = K.oracle_env(robot)
    venv = make_vec_env(n, True, gripper=False, relative=False, robot=robot)
    venv.reset()
    ik = venv.robot.get_ik()
    worst = 0.0
    hand = O.franka_hand_tcp_offset()  # (a real offset on every robot: a rotation about z and 0.1 m)
    for tcp in (hand, O.Pose()):
        fwd = ik.forward(qs, K.vec7(tcp))
        ref = np.array([K.vec7(o.sim.ik_forward(q, tcp)) for q in qs])
        worst = max(worst, float(np.abs(fwd - ref).max()))
    # the same configurations as the robots' state
    oe = make_oracle_envs(1, True, gripper=False, relative=False, robot=robot)[0]
    free, ref = np.zeros(n, dtype=bool), np.zeros((n, 7))
    for e, q in enumerate(qs):
        oe.reset()
        oe.sim.set_joints_hard(q)
        oe.sim.step(1)
        free[e] = oe.sim.s.d.ncon == 0
        ref[e] = K.vec7(oe.sim.get_cartesian_position())
        assert np.abs(ref[e] - K.vec7(o.sim.ik_forward(q, None))).max() < POSE_TOL
    venv.robot.set_joints_hard(qs)
    venv.sim.step(1)
    got = venv.robot.get_cartesian_position()
    venv.close()
    state_worst = float(np.abs(got - ref).max())
    print(f"\n{robot}: largest forward-pose difference {worst:.3e}; get_cartesian_position at {n} configurations, {int((~free).sum())} "
          f"of them in contact: {state_worst:.3e}; mat_to_quat branches {K.fk_branch_counts(robot).tolist()}")
    assert worst < POSE_TOL and state_worst < POSE_TOL


def test_set_cartesian_position_with_mask_failures_and_successes():
    """SimRobot.set_cartesian_position on 19 FR3 environments, every wavefront holding a reachable target, a target out of reach and a
    masked row: masked rows keep their state bit for bit, failed rows lose ik_success and nothing else, successful rows get the oracle's
    joint targets and are moving, no longer arrived."""
    import rcs_oracle as O
    from parity_util import make_oracle_envs, make_vec_env
    from rcs_env_oracle import FR3_Q_HOME

    n = 19
    venv = make_vec_env(n, True, gripper=False, relative=False)
    oenvs = make_oracle_envs(n, True, gripper=False, relative=False)
    venv.reset()
    robot, sim = venv.robot, venv.sim
    # everybody arrives at a joint target first, so that is_arrived is set and is_moving cleared
    rng = np.random.default_rng(17)
    first = np.tile(FR3_Q_HOME, (n, 1)) + rng.uniform(-0.05, 0.05, size=(n, 7))
    robot.set_joint_position(first)
    sim.step_until_convergence()
    for e, oe in enumerate(oenvs):
        oe.reset()
        oe.sim.set_joint_position(first[e])
        oe.sim.step_until_convergence()
    before, q_before, ctrl_before = robot.get_state(), sim.qpos.copy(), sim.ctrl.copy()
    assert before.is_arrived.all() and not before.is_moving.any() and before.ik_success.all()
    kind = np.arange(n) % 3  # 0 reachable, 1 out of reach, 2 masked (given a reachable or an unreachable target alternately)
    pose = robot.get_cartesian_position()
    shift = rng.uniform(-0.08, 0.08, size=(n, 3))
    target = np.zeros((n, 7))
    for e in range(n):
        near = O.Pose(translation=pose[e, :3] + shift[e], quaternion=pose[e, 3:]) * O.Pose(rpy_vector=rng.uniform(-0.3, 0.3, size=3))
        far = O.Pose(translation=[2.5, (-1.0) ** e, 0.5], quaternion=pose[e, 3:])
        target[e] = K.vec7(near if kind[e] == 0 or (kind[e] == 2 and e % 2 == 0) else far)
    robot.set_cartesian_position(target, mask=kind != 2)
    after, q_after, ctrl_after = robot.get_state(), sim.qpos, sim.ctrl
    venv.close()
    worst = 0.0
    for e, oe in enumerate(oenvs):
        if kind[e] == 2:
            continue
        oe.sim.set_cartesian_position(O.Pose(translation=target[e, :3], quaternion=target[e, 3:]))
        assert bool(oe.sim.s.ik_success) == (kind[e] == 0), e
        if kind[e] == 0:
            worst = max(worst, float(np.abs(after.target_angles[e] - np.asarray(oe.sim.s.target_angles[:7])).max()))
            assert np.abs(ctrl_after[e][:7] - np.asarray(oe.sim.ctrl)[:7]).max() < TOL
            assert np.abs(after.previous_angles[e] - np.asarray(oe.sim.s.previous_angles[:7])).max() < TOL
    print(f"\nset_cartesian_position: largest |target_angles - oracle| {worst:.3e}")
    ok, failed, masked = kind == 0, kind == 1, kind == 2
    assert np.array_equal(q_after, q_before)  # (a command moves nobody before the next substep)
    for name in ("previous_angles", "target_angles", "ik_success", "collision", "is_moving", "is_arrived"):
        assert np.array_equal(getattr(after, name)[masked], getattr(before, name)[masked]), name
    assert np.array_equal(ctrl_after[masked], ctrl_before[masked])
    assert not after.ik_success[failed].any()
    for name in ("previous_angles", "target_angles", "collision", "is_moving", "is_arrived"):
        assert np.array_equal(getattr(after, name)[failed], getattr(before, name)[failed]), name
    assert np.array_equal(ctrl_after[failed], ctrl_before[failed])
    assert after.ik_success[ok].all() and after.is_moving[ok].all() and not after.is_arrived[ok].any()
    assert worst < TOL
    assert (np.abs(after.target_angles[ok] - before.target_angles[ok]).max(axis=1) > 1e-3).all()


@pytest.mark.parametrize("robot,mode,relative_to", K.LIMIT_CONFIGS)
def test_env_steps_where_the_limits_and_the_clamp_bind(robot, mode, relative_to):
    """48 environments, 12 asynchronous env-steps with a step limit of 0.2 m / 45 deg and actions that exceed it, equal it and stay below it
    (kinematics_cases.limit_actions); in configured_origin the offset crosses the workspace clamp; the IK of some environments fails while
    their neighbours go on.  Up to the step at which an environment's oracle twin (joints moved by 1e-13 after reset) parts from it the
    environment is compared at 1e-9 and on its flags; after it on the flags alone, wherever the twin still agrees on them."""
    rep = K.run_limit_parity(robot, mode, relative_to)
    print(f"\n{robot} {mode} {relative_to}: {K.limit_case_summary(K.limit_case(robot, mode, relative_to))}\n   {rep}")
    assert rep["compared"] >= 0.9 * K.LIMIT_ENVS * K.LIMIT_STEPS
    assert rep["flag_mismatches"] == 0 and rep["late_flag_mismatches"] == 0, rep
    assert rep["max_abs_qpos"] < TOL and rep["max_abs_target"] < TOL and rep["max_abs_tquat"] < TOL and rep["max_abs_xyzrpy"] < TOL, rep
