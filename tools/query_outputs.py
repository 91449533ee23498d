"""dev tool (GPU): every output array of the query family -- point, motion, clearance, swept clearance, dynamics, their env forms, guard
peek -- through the host-pointer forms from seeded inputs, for comparing two builds of the library bit for bit (RCSH_LIB selects the build).

    RCSH_LIB=<lib.so> python tools/query_outputs.py OUT_DIR          one .npy per array
    python tools/query_outputs.py --compare DIR_A DIR_B              array_equal on every array; exit 1 on a difference

Scenes: fr3_empty_world (kinds 3), fr3_simple_pick_up (kinds 7, boxes near the hand: the free body's narrow phase runs),
xarm7_pick_world (the second archetype).  Rows: M = 259 (a dead team in the last wavefront) -- the contact rows the tests construct
(tests/test_gpu_clearance.py) and random rows within the joint limits, so that sphere-settled, box-settled, Gilbert, MPR, box-box, open
and beyond all occur -- and M = 4096 random rows.  The env forms: 259 environments after three steps of a seeded rollout."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("robot-control-stack_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

M_SMALL, M_LARGE, N_ENVS = 259, 4096, 259


def compare(a, b):
    names = sorted(f for f in os.listdir(a) if f.endswith(".npy"))
    assert names and names == sorted(f for f in os.listdir(b) if f.endswith(".npy")), "the two directories hold different arrays"
    bad = 0
    for f in names:
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        same = x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()  # (bit for bit: NaN payloads and zero signs included)
        nan = int(np.isnan(x).sum()) if x.dtype.kind == "f" else 0
        if same:
            diff = 0.0
        else:
            bad += 1
            diff = float(np.nanmax(np.abs(x.astype(np.float64) - y.astype(np.float64)))) if x.shape == y.shape else float("inf")
        print(f"{f}: shape {x.shape} dtype {x.dtype} {'bit-equal' if same else 'DIFFERENT'} (max abs difference {diff:.3e}{', %d NaN' % nan if nan else ''})")
    print("all arrays bit-equal" if not bad else f"{bad} of {len(names)} arrays differ")
    return 1 if bad else 0


def rows_for(name, m):
    """(robot, q [m, nl], q_to [m, nl], boxes [m, 7] or None, kinds)"""
    import test_gpu_clearance as TC
    from test_gpu_collision_query import _boxes, _random_rows

    simu, robot, orc, cm, home, sc = TC.scene(name)
    rng = np.random.default_rng(20 + m)
    finger_hi = 0.85 if cm.jnt_range[robot.dof, 1] > 0.1 else 0.04
    q = _random_rows(cm, robot, m, rng, finger_hi=finger_hi)
    boxes, kinds = None, 3
    if name == "fr3_simple_pick_up":
        kinds = 7
        boxes = _boxes(rng, m)
        if m == M_SMALL:
            # the tests' rows around the home pose with the cube at the fingertips: the pads' contact rows, then rows a hand's breadth off
            k = 48
            q[:k] = np.concatenate([home, [0.04, 0.04]])
            q[:k, :7] += rng.uniform(-0.01, 0.01, (k, 7))
            q[:k, 7:] = rng.uniform(0.0, 0.02, (k, 1))
            boxes[:k] = TC._boxes_near_hand(orc, cm, q[:k], rng, 0.005)
            boxes[:k, 3:] = 0.0
            yaw = rng.uniform(0, np.pi, k)
            boxes[:k, 3], boxes[:k, 6] = np.cos(yaw / 2), np.sin(yaw / 2)
            q[k:2 * k] = np.concatenate([home, [0.04, 0.04]])
            q[k:2 * k, :7] += rng.uniform(-0.3, 0.3, (k, 7))
            q[k:2 * k, 7:] = rng.uniform(0.0, 0.04, (k, 1))
            boxes[k:2 * k] = TC._boxes_near_hand(orc, cm, q[k:2 * k], rng, 0.10)
            boxes[2 * k:3 * k] = TC._boxes_near_hand(orc, cm, q[2 * k:3 * k], rng, 0.10)
    elif name == "xarm7_pick_world":
        kinds = 7
        boxes = _boxes(rng, m, (0.4, 0.0))
    elif m == M_SMALL:
        c = TC._contact_rows_empty(orc, home, rng)
        q[:len(c)] = c
    lo, hi = cm.jnt_range[:q.shape[1], 0], cm.jnt_range[:q.shape[1], 1]
    q_to = np.clip(q + rng.uniform(-0.2, 0.2, q.shape), lo, hi)
    q_to[:, robot.dof:] = q[:, robot.dof:]
    return robot, q, q_to, boxes, kinds


def dump(out):
    os.makedirs(out, exist_ok=True)

    def save(tag, names, arrays):
        for n, a in zip(names, arrays):
            np.save(os.path.join(out, f"{tag}_{n}.npy"), np.asarray(a))

    clear_names = ("distance", "status", "pair", "witness", "grad")

    def save_dict(tag, arrays):
        save(tag, sorted(arrays), [arrays[k] for k in sorted(arrays)])
    for name in ("fr3_empty_world", "fr3_simple_pick_up", "xarm7_pick_world"):
        for m in (M_SMALL, M_LARGE):
            robot, q, q_to, boxes, kinds = rows_for(name, m)
            tag = f"{name}_M{m}"
            save(f"{tag}_point", ("hit", "kinds_hit", "pair"), robot.check_collision(q, free_qpos=boxes, kinds=kinds))
            save(f"{tag}_motion", ("result", "t_contact"), robot.check_motion(q, q_to, resolution=1e-3, free_qpos=boxes, kinds=kinds))
            mask = np.ones(len(robot.clearance_pairs(kinds)), dtype=np.uint8)
            mask[::3] = 0
            near = {"d_max": 0.002, "pair_mask": robot.clearance_mask(kinds)}  # (without the finger pads' pairs most rows are beyond 2 mm)
            for ctag, kw in (("inf", {}), ("dmax005", {"d_max": 0.05}), ("masked", {"pair_mask": mask}), ("dmax0002_no_finger_pairs", near)):
                res = robot.check_clearance(q, free_qpos=boxes, kinds=kinds, **kw)
                save(f"{tag}_clearance_{ctag}", clear_names, res)
                print(tag, ctag, "status apart/beyond/contact/open", np.bincount(res[1], minlength=4).tolist(), flush=True)
            # swept clearance (1 cm brackets and samples: the large batch stays a matter of seconds) and dynamics, every output and a few
            for stag, kw in (("all", {}), ("masked_dmax005_no_grad", {"pair_mask": mask, "d_max": 0.05, "want_grad": False})):
                res = robot.swept_clearance(q, q_to, tolerance=1e-2, resolution=1e-2, free_qpos=boxes, kinds=kinds, **kw)
                save_dict(f"{tag}_swept_{stag}", res)
                print(tag, "swept", stag, "status bracketed/beyond/contact/open", np.bincount(res["status"], minlength=4).tolist(), flush=True)
            rng = np.random.default_rng(40 + m)
            v, a, f = (rng.uniform(-1, 1, q.shape) for _ in range(3))
            save_dict(f"{tag}_dynamics_all", robot.dynamics_query(q, v, a, f, tcp_offset=None))
            save_dict(f"{tag}_dynamics_jac_inverse", robot.dynamics_query(q, v, qacc=a, want=("jac", "qfrc_inverse")))
    # the env forms: the environments' own rows after three steps
    from parity_util import make_vec_env, synthetic_actions
    from test_gpu_clearance import _pick_env

    joints, grip = synthetic_actions(N_ENVS, 4, 3)
    for tag, venv, kinds in (("env_fr3_empty_world", make_vec_env(N_ENVS, True), 3), ("env_fr3_simple_pick_up", _pick_env(N_ENVS), 7)):
        venv.reset()
        for t in range(3):
            venv.step({"joints": joints[t], "gripper": grip[t]})
        mask = np.ones(len(venv.robot.clearance_pairs(kinds)), dtype=np.uint8)
        mask[::3] = 0
        for ctag, kw in (("inf", {}), ("dmax005", {"d_max": 0.05}), ("masked", {"pair_mask": mask})):
            save(f"{tag}_clearance_{ctag}", clear_names, venv.clearance(kinds=kinds, **kw))
        nl = int(venv.sim.model.nq)
        q_to = venv.sim.qpos[:, :nl] + np.random.default_rng(50).uniform(-0.2, 0.2, (N_ENVS, nl)) * np.array([1.0] * venv.robot.dof + [0.0] * (nl - venv.robot.dof))
        save_dict(f"{tag}_swept_all", venv.swept_clearance(q_to, tolerance=1e-2, resolution=1e-2, kinds=kinds))
        save_dict(f"{tag}_swept_masked_dmax005", venv.swept_clearance(q_to, tolerance=1e-2, resolution=1e-2, kinds=kinds, pair_mask=mask, d_max=0.05))
        f = np.random.default_rng(51).uniform(-1, 1, (N_ENVS, nl))
        save_dict(f"{tag}_dynamics_all", venv.dynamics(qacc=f[::-1], qfrc=f))
        save_dict(f"{tag}_dynamics_bias_gravity", venv.dynamics(want=("qfrc_bias", "gravity")))
        venv.configure_guard(enabled=False, kinds=kinds)
        for scale in (1.0, 8.0):  # (the second: actions large enough to be clamped, some into contact)
            save(f"{tag}_guard_x{scale:g}", ("blocked", "result", "t_contact"), venv.check_action({"joints": scale * joints[3]}))
        venv.close()
    print("wrote", len(os.listdir(out)), "arrays to", out)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    dump(sys.argv[1])
