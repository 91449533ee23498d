"""A handle's resources over its life (csrc/rcs_hip.hip: the owners of rcsh_sim and CopyCarrier, csrc/owned.h): what an entry point
replaces -- a render scene, the buffers of per-environment contact resolution, a render schedule -- and what rcsh_sim_destroy gives back
leave no trace in what the next call, or the next handle, computes.  Everything is compared bit for bit against a handle that took the
short way.  Nothing here asserts on free device memory: the device is shared."""

import ctypes as C
import gc
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "robot-control-stack_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k, np.argwhere(np.asarray(a[k]) != np.asarray(b[k]))[:8].tolist())


def _sim_with_hand(n):
    from rcs_amd import sim as S
    from rcs_amd.envs import default_sim_gripper_cfg, default_sim_robot_cfg

    cfg = default_sim_robot_cfg("fr3_empty_world")
    simu = S.Sim(cfg.mjcf_scene_path, S.SimConfig(max_convergence_steps=40), n_envs=n)
    robot = S.SimRobot(simu, None, cfg)
    S.SimGripper(simu, default_sim_gripper_cfg())
    return simu, robot


def _camera(simu, name="wrist_0", frame_rate=0, width=32, height=24, **kw):
    from rcs_amd.camera import SimCameraConfig, SimCameraSet

    cams = {name: SimCameraConfig(identifier=name, frame_rate=frame_rate, resolution_width=width, resolution_height=height)}
    return SimCameraSet(simu, cams, physical_units=True, **kw)


def test_a_second_render_scene_replaces_the_first():
    """A SimCameraSet attaches its render scene on construction; a second set on the same Sim attaches a second one, whose buffers replace
    the first's.  Its 32 x 24 depth frame of 4 environments equals the frame of a fresh handle that only ever had that scene, and
    still does once the first set is gone."""
    n = 4
    rng = np.random.default_rng(11)
    dq = rng.uniform(-0.3, 0.3, (n, 7))

    def posed():
        simu, robot = _sim_with_hand(n)
        first = _camera(simu, "bird_eye_cam")
        robot.set_joint_position(robot.get_joint_position() + dq)
        simu.step(25)
        return simu, first

    simu, first = posed()
    second = _camera(simu, "bird_eye_cam")
    fresh_sim, fresh = posed()

    def frame(cs):
        depth, xmat, xpos = cs.render_raw("bird_eye_cam")
        return {"depth": depth, "xmat": xmat, "xpos": xpos}

    want = frame(fresh)
    assert want["depth"].shape == (n, 24, 32) and want["depth"].min() < 1.0  # (something is in view)
    assert len({want["depth"][e].tobytes() for e in range(n)}) == n  # (every environment has its own pose)
    _same(frame(second), want, "the second scene's frame")
    del first
    gc.collect()
    _same(frame(second), want, "the same frame after the first camera set is gone")
    simu.close(), fresh_sim.close()


def _rollout(venv, steps, seed):
    from parity_util import synthetic_actions

    joints, grip = synthetic_actions(venv.n_envs, steps, seed=seed, dof=venv.dof)
    venv.sim.reset()
    venv.reset()
    out = {}
    for t in range(steps):
        o, _, term, trunc, i = venv.step({"joints": joints[t], "gripper": grip[t]})
        out.update({f"obs{t}.{k}": v for k, v in o.items()})
        out.update({f"info{t}.{k}": np.asarray(v) for k, v in i.items()})
        out[f"terminated{t}"], out[f"truncated{t}"] = term, trunc
    st = venv.robot.get_state()
    out.update({"qpos": venv.sim.qpos, "qvel": venv.sim.qvel, "converged": venv.sim.is_converged(), "state": venv.sim.get_state(),
                "ik_success": np.asarray(st.ik_success), "collision": np.asarray(st.collision), "is_moving": np.asarray(st.is_moving),
                "is_arrived": np.asarray(st.is_arrived)})
    now, ever = venv.sim.contact_escalated()
    out.update({"escalated_now": now, "escalated_ever": ever, "unresolved": venv.sim.contact_unresolved(), "overflow": venv.sim.contact_overflow()})
    return out


def test_contact_resolution_switched_on_off_and_on_again():
    """Contacts resolved per environment (rcsh_contact_options, mode 7) switched on, off and on again on one handle: the buffers of the
    first switch are kept and cleared, the option is set anew.  After Sim.reset, 20 env-steps of the suite's synthetic actions on 8
    environments give the positions, velocities and flags of a fresh handle that switched it on once -- and the same state blob."""
    from parity_util import make_vec_env
    from rcs_amd import _lib

    n, steps = 8, 20
    venv = make_vec_env(n, True)  # (the default of a scene without a free body: switched on at creation)
    assert venv.sim.resolve_robot_contacts == 7
    for mode in (0, 7):
        opts = _lib.make_contact_options(venv.sim.model, mode)
        _lib.check(venv._L.rcsh_sim_set_contact_options(venv.sim._h, C.byref(opts)))
    got = _rollout(venv, steps, seed=3)
    fresh = make_vec_env(n, True)
    want = _rollout(fresh, steps, seed=3)
    assert np.abs(want["qpos"] - want["qpos"][0]).max() > 1e-3  # (the environments went their own ways)
    _same(got, want, "on, off, on against on")
    venv.close(), fresh.close()


def _everything_once(n, joints, grip):
    """One handle that configures every kind of resource a handle can own, steps twice and is destroyed; what it computed."""
    from parity_util import make_vec_env
    from rcs_amd import _lib

    venv = make_vec_env(n, True)
    L, h = venv._L, venv.sim._h
    out = {}
    _lib.check(L.rcsh_prof_enable(h, 1))  # profiling events around every stepping launch
    venv.configure_guard(enabled=True)
    venv.configure_autoreset(enabled=True, max_episode_steps=1)
    venv.reset()
    # query staging, grown once: 3 rows, then 300
    home = venv.sim.qpos
    for m in (3, 300):
        rows = np.ascontiguousarray(np.tile(home[0], (m, 1)) + np.linspace(-0.3, 0.3, m)[:, None] * (np.arange(home.shape[1]) < venv.dof))
        rows[::2, 1], rows[::2, 3] = 1.7, -0.4  # every other row: the arm folded forward and down
        hit, kinds, pair = np.zeros(m, dtype=np.uint8), np.zeros(m, dtype=np.uint8), np.zeros((m, 2), dtype=np.int32)
        _lib.check(L.rcsh_collision_query(h, _lib.ptr(rows), None, m, 7, _lib.ptr(hit), _lib.ptr(kinds), _lib.ptr(pair)))
        out.update({f"query{m}.hit": hit, f"query{m}.kinds": kinds, f"query{m}.pair": pair})
    assert out["query300.hit"].any() and not out["query300.hit"].all()
    # the copy carrier of a world of one: created, connected to itself, destroyed
    blob = C.create_string_buffer(256)
    _lib.check(L.rcsh_comm_copy_create(h, 0, 1, 8 * n * venv.obs_width, blob))
    _lib.check(L.rcsh_comm_copy_connect(h, blob.raw))
    recv = C.c_void_p()
    _lib.check(L.rcsh_comm_copy_recv_buffer(h, 0, C.byref(recv)))
    assert recv.value
    _lib.check(L.rcsh_comm_destroy(h))
    with pytest.raises(RuntimeError, match="no copy carrier"):
        _lib.check(L.rcsh_comm_copy_recv_buffer(h, 0, C.byref(recv)))
    # step one: guarded, under autoreset (a time limit of one step: every episode ends and is reset on the device)
    o, _, term, trunc, i = venv.step({"joints": joints[0], "gripper": grip[0]})
    out.update({f"obs0.{k}": v for k, v in o.items()})
    out.update({f"info0.{k}": np.asarray(v) for k, v in i.items() if not isinstance(v, dict)})
    out.update({f"final_obs0.{k}": v for k, v in i["final_obs"].items()})
    out["terminated0"], out["truncated0"] = term, trunc
    assert i["autoreset"].all() and not i["guard_blocked"].any()
    # step two: a render scene with a schedule instead of autoreset (the two exclude each other)
    venv.configure_autoreset(enabled=False)
    cs = _camera(venv.sim, "wrist_0", frame_rate=30, width=8, height=6, render_on_demand=False, max_framesets=16)
    o, _, term, trunc, i = venv.step({"joints": joints[1], "gripper": grip[1]})
    out.update({f"obs1.{k}": v for k, v in o.items()})
    out.update({f"info1.{k}": np.asarray(v) for k, v in i.items()})
    out["terminated1"], out["truncated1"] = term, trunc
    assert cs.buffer_size() >= 1  # (a camera is due at once: the step's launch recorded a frame and the host rendered it)
    out["frames"] = np.asarray(cs.buffer_size())
    out["depth"] = cs._buffer[0]["depth"]["wrist_0"]
    out["frame_time"] = cs._buffer[0]["timestamp"]
    ms, launches = C.c_double(0), C.c_int64(0)
    _lib.check(L.rcsh_prof_read(h, C.byref(ms), C.byref(launches)))
    assert launches.value == 2 and ms.value > 0  # (the two env-steps' stepping launches were timed)
    out.update({"qpos": venv.sim.qpos, "qvel": venv.sim.qvel, "state": venv.sim.get_state()})
    venv.close()
    return out


def test_six_handles_created_and_destroyed_in_one_process():
    """Six handles one after the other in this process, each with a guard, autoreset, a render scene with a schedule, query staging
    grown once, profiling events and a copy-carrier communicator of world size 1 that is created and destroyed; each steps twice and is
    destroyed.  What the last one computed equals what the first one did, bit for bit (and so does every one in between)."""
    from parity_util import synthetic_actions

    n = 8
    joints, grip = synthetic_actions(n, 2, seed=5)
    first = _everything_once(n, joints, grip)
    for k in range(1, 6):
        _same(_everything_once(n, joints, grip), first, ("handle", k))


def test_render_schedule_grown_removed_and_set_again():
    """The render schedule grown (same cameras, larger capacity), removed (ncam = 0) and set again.  Growing keeps the cameras' clocks:
    no frame becomes due by it (tests/test_gpu_parity.py::test_render_schedule_grows_with_the_launch_and_rejects_a_second_set holds
    the pending records to that).  Without a schedule there is nothing to collect; a schedule set after the removal starts every
    camera as due, as the first one did."""
    from rcs_amd import _lib

    n = 3
    simu, _ = _sim_with_hand(n)
    cs = _camera(simu, "wrist_0", frame_rate=30, width=8, height=6, render_on_demand=False, max_framesets=100)
    L, h = simu._L, simu._h

    def pending():
        count = np.zeros(n, dtype=np.int32)
        _lib.check(L.rcsh_render_pending(h, _lib.ptr(count)))
        return count

    simu.step(3)
    assert cs.buffer_size() == 1  # due at once, after the first substep
    t_first = cs._buffer[0]["timestamp"].copy()
    assert np.allclose(t_first, simu.model.timestep, rtol=0, atol=1e-12)
    small = cs._capacity
    cs.ensure_capacity(4000)  # grows: the same cameras and periods, a larger capacity
    assert cs._capacity > small
    simu.step(3)
    assert cs.buffer_size() == 1 and (pending() == 0).all()  # the clocks survived: 6 substeps of 2 ms are short of a 30 Hz period
    _lib.check(L.rcsh_sim_set_render_schedule(h, None, None, 0, 0))  # removed
    with pytest.raises(RuntimeError, match="no render schedule"):
        pending()
    simu._rate_camera_sets = []
    simu.step(3)  # (steps without a schedule: nothing is recorded, nothing is collected)
    assert cs.buffer_size() == 1
    cs._capacity = 0
    cs.ensure_capacity(40)  # set again
    simu._rate_camera_sets = [cs]
    assert (pending() == 0).all()
    simu.step(3)
    assert cs.buffer_size() == 2  # every camera started as due: one frame, after the launch's first substep
    ev = cs._buffer[1]
    assert ev["have"]["wrist_0"].all()
    assert np.allclose(ev["timestamp"], 10 * simu.model.timestep, rtol=0, atol=1e-12)
    simu.close()
