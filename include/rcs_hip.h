/*
 * rcs_hip.h -- C-ABI of the MI355X batched simulation backend (librcs_hip.so).
 *
 * Drop-in boundary for the RCS simulation hot path.  Each entry point is the
 * N-environment form of one method the reference exposes through its pybind11
 * module `rcs._core.sim` / `rcs._core.common` (reference src/pybind/rcs.cpp);
 * the reference method it replaces is cited on every declaration.  A reference
 * maintainer binds these exactly like the existing C++ classes (INTEGRATION.md
 * shows the pybind11 and ctypes stubs).
 *
 * Conventions
 *  - plain C: opaque handle, caller-owned buffers, no exceptions.  Every call
 *    returns RCSH_OK or an error code; rcsh_last_error() gives the message of the
 *    last failure on the calling thread.  The Python shim maps
 *    RCSH_ERR_NAME -> RuntimeError and RCSH_ERR_ARG -> ValueError, the exception
 *    types the reference raises (SimRobot.cpp:57-93, SimGripper.cpp:80-83).
 *  - arrays are row-major, environment-major: q[N][dof], pose[N][7] = x y z qx qy qz qw
 *    (Eigen coeff order, reference Pose.cpp:115), flags uint8 (0/1).
 *  - `mask` (uint8[N], may be NULL = all) selects the environments a call acts on.
 *  - entry points without a suffix take HOST pointers and synchronise; `_dev`
 *    entry points take DEVICE pointers, enqueue on the handle's HIP stream and
 *    return immediately (rcsh_sim_synchronize() or a stream wait orders them).
 *  - the library never falls back to the CPU: without a usable gfx950 device
 *    rcsh_sim_create fails with RCSH_ERR_DEVICE.
 */
#ifndef RCS_HIP_H
#define RCS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RCSH_ABI_VERSION 2

enum {
  RCSH_OK = 0,
  RCSH_ERR_ARG = 1,       /* std::invalid_argument in the reference */
  RCSH_ERR_NAME = 2,      /* std::runtime_error("No joint named ...") in the reference */
  RCSH_ERR_MODEL = 3,     /* scene outside the compiled archetypes / MJCF subset */
  RCSH_ERR_DEVICE = 4,    /* no gfx950 device, HIP failure */
  RCSH_ERR_STATE = 5      /* call order violated (e.g. robot not added) */
};

/* Flat scene tables; field names follow mjModel.  Stands where the reference hands
 * `mjModel*` to `Sim(mjmdl, mjdata)` (reference src/pybind/rcs.cpp:493-497). */
typedef struct rcsh_model_desc {
  int32_t nbody, njnt, nu, ntendon, nwrap, neq, nsite;
  double timestep;
  double gravity[3];
  const int32_t* body_parentid;   /* [nbody] */
  const int32_t* body_jntadr;     /* [nbody] joint id or -1 */
  const int32_t* body_jntnum;     /* [nbody] */
  const double* body_pos;         /* [nbody][3] */
  const double* body_quat;        /* [nbody][4] wxyz */
  const double* body_ipos;        /* [nbody][3] */
  const double* body_iquat;       /* [nbody][4] */
  const double* body_mass;        /* [nbody] */
  const double* body_inertia;     /* [nbody][3] principal */
  const double* body_gravcomp;    /* [nbody] */
  const int32_t* jnt_type;        /* [njnt] 2 slide, 3 hinge */
  const int32_t* jnt_bodyid;      /* [njnt] */
  const double* jnt_pos;          /* [njnt][3] */
  const double* jnt_axis;         /* [njnt][3] */
  const int32_t* jnt_limited;     /* [njnt] */
  const double* jnt_range;        /* [njnt][2] */
  const double* jnt_margin;       /* [njnt] */
  const double* jnt_solref;       /* [njnt][2] */
  const double* jnt_solimp;       /* [njnt][5] */
  const int32_t* jnt_actfrclimited;
  const double* jnt_actfrcrange;  /* [njnt][2] */
  const int32_t* jnt_actgravcomp;
  const double* dof_armature;     /* [njnt] */
  const double* dof_damping;      /* [njnt] */
  const double* dof_frictionloss; /* [njnt] dry joint friction (soft row per dof, team kernel only) */
  const double* qpos0;            /* [njnt] */
  const int32_t* tendon_adr;      /* [ntendon] */
  const int32_t* tendon_num;      /* [ntendon] */
  const int32_t* wrap_objid;      /* [nwrap] joint ids */
  const double* wrap_prm;         /* [nwrap] coefficients */
  const int32_t* eq_obj1id;       /* [neq] joint ids */
  const int32_t* eq_obj2id;
  const int32_t* eq_active0;
  const double* eq_data;          /* [neq][5] polycoef */
  const double* eq_solref;        /* [neq][2] */
  const double* eq_solimp;        /* [neq][5] */
  const int32_t* actuator_trntype;   /* [nu] 0 joint, 3 tendon */
  const int32_t* actuator_trnid;
  const double* actuator_gear;       /* [nu] */
  const double* actuator_gainprm;    /* [nu][3] */
  const double* actuator_biasprm;    /* [nu][3] */
  const int32_t* actuator_biastype;  /* [nu] 0 none, 1 affine */
  const int32_t* actuator_ctrllimited;
  const double* actuator_ctrlrange;  /* [nu][2] */
  const int32_t* actuator_forcelimited;
  const double* actuator_forcerange; /* [nu][2] */
  const int32_t* site_bodyid;        /* [nsite] */
  const double* site_pos;            /* [nsite][3] */
  const double* site_quat;           /* [nsite][4] */
  /* collision geoms: detected against the static plane geom everywhere (collision flags); in scenes with a free box
   * (rcsh_sim_add_free_box) their contacts with the floor and the box are resolved */
  int32_t ngeom, nmeshvert;
  const int32_t* geom_type;          /* [ngeom] mjtGeom: 0 plane, 2 sphere, 3 capsule, 6 box, 7 mesh */
  const int32_t* geom_bodyid;        /* [ngeom] */
  const int32_t* geom_contype;       /* [ngeom] */
  const int32_t* geom_conaffinity;   /* [ngeom] */
  const double* geom_pos;            /* [ngeom][3] */
  const double* geom_quat;           /* [ngeom][4] */
  const double* geom_size;           /* [ngeom][3] */
  const int32_t* geom_vertadr;       /* [ngeom] first row of mesh_vert */
  const int32_t* geom_vertnum;       /* [ngeom] 0: no vertex set (geom never reports contacts) */
  const double* mesh_vert;           /* [nmeshvert][3] convex-hull vertices, geom frame */
  const double* dof_solref;          /* [njnt][2] solreffriction */
  const double* dof_solimp;          /* [njnt][5] solimpfriction */
  const double* geom_friction;       /* [ngeom][3] sliding, torsional, rolling (contacts are condim 3: only [0] is used) */
} rcsh_model_desc;

/* SimRobotConfig after name -> id lookup (reference src/sim/SimRobot.h:14-47, SimRobot.cpp:52-94). */
typedef struct rcsh_robot_desc {
  int32_t dof;
  const int32_t* joint_ids;     /* [dof] */
  const int32_t* actuator_ids;  /* [dof] */
  int32_t attachment_site;
  int32_t base_body;
  const double* q_home;         /* [dof] robots_meta_config.q_home, reference include/rcs/Robot.h:24-95 */
  double tcp_offset[7];         /* pose, xyzw quaternion */
  double joint_rotational_tolerance; /* SimRobot.h:15 */
  double seconds_between_callbacks;  /* SimRobot.h:17 */
  int32_t register_convergence_callback;
  int32_t n_collision_geoms;         /* SimRobotConfig.arm_collision_geoms after name lookup (SimRobot.cpp:55-62) */
  const int32_t* collision_geom_ids;
} rcsh_robot_desc;

/* SimGripperConfig after name -> id lookup (reference src/sim/SimGripper.h:15-45). */
typedef struct rcsh_gripper_desc {
  int32_t joint_id;
  int32_t actuator_id;
  double epsilon_inner, epsilon_outer;
  double seconds_between_callbacks;
  double max_actuator_width, min_actuator_width;
  double max_joint_width, min_joint_width;
  /* SimGripperConfig.collision_geoms / collision_geoms_fingers / ignored_collision_geoms (SimGripper.cpp:31-33,57-63) */
  int32_t n_collision_geoms, n_finger_geoms, n_ignored_geoms;
  const int32_t* collision_geom_ids;
  const int32_t* finger_geom_ids;
  const int32_t* ignored_geom_ids;
} rcsh_gripper_desc;

/* Gymnasium-loop configuration of the fused env-step (reference python/rcs/envs/creators.py:43-128). */
enum { RCSH_MODE_JOINTS = 0, RCSH_MODE_CARTESIAN_TRPY = 1, RCSH_MODE_CARTESIAN_TQUAT = 2,
       /* torque-actuated robots (csrc/env_torque_team.h; "torque and impedance control modes" below) */
       RCSH_MODE_TORQUE = 3, RCSH_MODE_JOINT_IMPEDANCE = 4, RCSH_MODE_CARTESIAN_IMPEDANCE_TRPY = 5,
       RCSH_MODE_CARTESIAN_IMPEDANCE_TQUAT = 6 };
enum { RCSH_REL_NONE = 0, RCSH_REL_LAST_STEP = 1, RCSH_REL_CONFIGURED_ORIGIN = 2 };
typedef struct rcsh_env_desc {
  int32_t control_mode;
  int32_t relative_to;
  double max_mov[2];            /* joints: [0]; cartesian: translation, rotation */
  int32_t binary_gripper;       /* GripperWrapper(binary=True) */
  const double* joint_low;      /* [dof] robots_meta_config.joint_limits */
  const double* joint_high;
} rcsh_env_desc;

typedef struct rcsh_sim rcsh_sim;

const char* rcsh_last_error(void);
int rcsh_abi_version(void);
int rcsh_device_count(void);

/* rcs._core.sim.Sim(mjmdl, mjdata)  -- rcs.cpp:493-497; one handle = n_envs independent mjData */
int rcsh_sim_create(const rcsh_model_desc* model, int32_t n_envs, int32_t device, rcsh_sim** out);
void rcsh_sim_destroy(rcsh_sim* sim);
int rcsh_sim_num_envs(const rcsh_sim* sim);
int rcsh_sim_synchronize(rcsh_sim* sim);
/* the HIP stream (hipStream_t) all work of this handle is enqueued on; set_stream adopts a caller-owned
 * stream (e.g. the host framework's current stream, so its collectives order after the env-step kernel) */
void* rcsh_sim_stream(rcsh_sim* sim);
int rcsh_sim_set_stream(rcsh_sim* sim, void* hip_stream);
/* Stream ordering between handles (no reference counterpart): everything enqueued on `sim`'s stream after this call runs after
 * what `producer`'s stream holds now (an event on the producer's stream, a stream-side wait on the other: no host blocking).
 * A host that runs several handles side by side -- sub-batches of different robot types on one GPU -- orders the places where
 * they meet (a shared observation block, an exchange slot) with it, without a HIP binding of its own. */
int rcsh_sim_wait_for(rcsh_sim* sim, rcsh_sim* producer);
/* Kernel selection (no reference counterpart).  Every scene runs on the team kernel (16 lanes per environment);
 * RCSH_KERNEL_AUTO and RCSH_KERNEL_TEAM both name it.  RCSH_KERNEL_LANE, the one-lane-per-environment kernel of ABI 1, was
 * removed (it lost at every batch size and stepped neither dry friction nor free bodies): selecting it is RCSH_ERR_ARG.
 * RCSH_KERNEL_TEAM_OCC2 is the same team kernel compiled for two resident wavefronts per SIMD (<= 256 registers); it exists
 * for the launches without free box / resolved contacts / collision callbacks and falls back to TEAM elsewhere.  AUTO picks
 * by batch size; the results of the two are bit-identical. */
enum { RCSH_KERNEL_AUTO = 0, RCSH_KERNEL_TEAM = 1, RCSH_KERNEL_LANE = 2, RCSH_KERNEL_TEAM_OCC2 = 3 };
int rcsh_sim_set_kernel(rcsh_sim* sim, int32_t variant);

/* Sim.set_config / get_config -- rcs.cpp:501-502, sim.cpp:27-32; SimConfig sim.h:29-34 */
int rcsh_sim_set_config(rcsh_sim* sim, int32_t async_control, int32_t realtime, int32_t frequency,
                        int32_t max_convergence_steps);
int rcsh_sim_get_config(const rcsh_sim* sim, int32_t* async_control, int32_t* realtime, int32_t* frequency,
                        int32_t* max_convergence_steps);
/* Sim.step(k) -- rcs.cpp:503, sim.cpp:108-115 */
int rcsh_sim_step(rcsh_sim* sim, int64_t k);
/* Sim.step_until_convergence() -- rcs.cpp:498-499, sim.cpp:84-106 */
int rcsh_sim_step_until_convergence(rcsh_sim* sim);
/* Sim.is_converged() -- rcs.cpp:500, sim.cpp:83; also the substeps the last call took per env */
int rcsh_sim_is_converged(rcsh_sim* sim, uint8_t* converged, int32_t* convergence_steps);
/* Sim.reset() -- rcs.cpp:504, sim.cpp:117-138 */
int rcsh_sim_reset(rcsh_sim* sim, const uint8_t* mask);

/* SimRobot(sim, ik, cfg, register_convergence_callback) -- rcs.cpp:516-527, SimRobot.cpp:27-43 */
int rcsh_sim_add_robot(rcsh_sim* sim, const rcsh_robot_desc* robot);
/* Robot.set_joint_position -- rcs.cpp:358-359, SimRobot.cpp:123-131 */
int rcsh_robot_set_joint_position(rcsh_sim* sim, const double* q, const uint8_t* mask);
/* Robot.get_joint_position -- rcs.cpp:360, SimRobot.cpp:133-139 */
int rcsh_robot_get_joint_position(rcsh_sim* sim, double* q);
/* Robot.get_cartesian_position -- rcs.cpp:356-357, SimRobot.cpp:114-121 */
int rcsh_robot_get_cartesian_position(rcsh_sim* sim, double* pose);
/* Robot.get_base_pose_in_world_coordinates -- rcs.cpp:369-370, SimRobot.cpp:207-213 */
int rcsh_robot_get_base_pose(rcsh_sim* sim, double* pose);
/* Robot.set_cartesian_position -- rcs.cpp:365-367, SimRobot.cpp:145-155 (Pin CLIK, Kinematics.cpp:28-68) */
int rcsh_robot_set_cartesian_position(rcsh_sim* sim, const double* pose, const uint8_t* mask);
/* SimRobot.set_joints_hard -- rcs.cpp:525, SimRobot.cpp:198-205 */
int rcsh_robot_set_joints_hard(rcsh_sim* sim, const double* q, const uint8_t* mask);
/* Robot.reset / move_home -- rcs.cpp:361-363, SimRobot.cpp:47-50,193-196 */
int rcsh_robot_reset(rcsh_sim* sim, const uint8_t* mask);
int rcsh_robot_move_home(rcsh_sim* sim, const uint8_t* mask);
/* SimRobot.get_state -- rcs.cpp:527, SimRobotState SimRobot.h:49-57; any pointer may be NULL */
int rcsh_robot_get_state(rcsh_sim* sim, uint8_t* ik_success, uint8_t* collision, uint8_t* is_moving,
                         uint8_t* is_arrived, double* previous_angles, double* target_angles);
/* Kinematics.inverse / forward on the robot's own chain -- rcs.cpp:289-300, Kinematics.cpp:28-82.
 * q0 [N][dof] -> q [N][nq] (nq = model dofs, quirk Q7), success [N], iterations [N] (may be NULL) */
int rcsh_ik_inverse(rcsh_sim* sim, const double* pose, const double* q0, const double* tcp_offset7, double* q,
                    uint8_t* success, int32_t* iterations);
int rcsh_ik_forward(rcsh_sim* sim, const double* q0, const double* tcp_offset7, double* pose);

/* ---- collision queries on caller-supplied configurations (no reference method: MjORobot.check_collision of the reference's
 * OMPL layer, python/rcs/ompl/mj_ompl.py, writes q into mjData, runs mj_fwdPosition + mj_collision and looks at the contacts).
 * Evaluated against the handle's scene -- the floor plane, the robot's own collision geoms (its world-welded base included) and,
 * in a scene with a free body, that body at the pose `free_qpos` [M][7] (x y z qw qx qy qz; NULL: the body is not tested) -- and
 * independent of n_envs: they read and write NO per-environment state, and run on the handle's stream.
 * q rows are [M][nl]: the robot chain's joints including the finger slides (the width rcsh_ik_inverse returns).  `kinds`: bit 0
 * robot geom <-> floor, bit 1 robot geom <-> robot geom (MuJoCo's pair filters), bit 2 robot geom <-> free body.  A pair is in
 * contact when it penetrates by more than 1e-9 m; joint limits are not collisions (q outside the range is evaluated as given).
 * Robots without collision geometry (the ur5e, so101 and arm6 scenes) answer "no contact" for every row.  RCSH_ERR_MODEL: the
 * scene has geoms or geom pairs beyond the contact tables' capacity (rcsh_sim_contact_table_dropped,
 * rcsh_sim_contact_check_unchecked_pairs), so the answer could not be exact.  RCSH_ERR_ARG: M < 0, an unknown kinds bit, a null
 * pointer where M > 0, free_qpos in a scene without a free body, a non-finite entry (host forms only: the _dev forms do not read
 * the values on the host), resolution <= 0.  M = 0 does nothing.
 * Point query: hit [M] (any selected kind in contact), kinds_hit [M] (the kinds found, complete; may be NULL), pair [M][2] (MuJoCo
 * geom ids of one penetrating pair, in MuJoCo's order within a contact, the same from run to run; -1 -1 for none; may be NULL). */
int rcsh_collision_query(rcsh_sim* sim, const double* q, const double* free_qpos, int32_t m, int32_t kinds, uint8_t* hit,
                         uint8_t* kinds_hit, int32_t* pair);
int rcsh_collision_query_dev(rcsh_sim* sim, const double* q_dev, const double* free_qpos_dev, int32_t m, int32_t kinds, uint8_t* hit_dev,
                             uint8_t* kinds_hit_dev, int32_t* pair_dev);
/* Motion query: the straight joint-space segment q(s) = q_from + s (q_to - q_from), s in [0, 1], per row.  result [M]: 0 free -- no
 * configuration of the segment is in contact, PROVEN by the lever certificate (never inferred from samples); 1 contact -- t_contact
 * [M] is the smallest sampled s whose configuration the point query reports in contact; 2 undecided -- every piece that could not
 * be certified was bisected down to `resolution` (its largest joint travel, rad or m) and no sampled point was in contact.
 * t_contact is -1 where result != 1.  One launch per call.  The work per row is bounded whatever the resolution: after 2048
 * evaluated configurations without a contact a row samples s = k / 32 beyond what it settled and reports 1 at the first contact,
 * else 2 (a contact lasting over 1/32 of the segment is never reported as 2; a row that runs out after a contact reports it, though
 * an earlier one may have gone unsampled).  A row whose finger slides leave qpos0 -+ the stroke the levers were built for is never
 * reported 0.  A free-body quaternion of zero norm is the identity (as mju_normalize4 makes it); a scene with a colliding geom of a
 * type other than plane, capsule, box or mesh is refused (RCSH_ERR_MODEL). */
int rcsh_motion_query(rcsh_sim* sim, const double* q_from, const double* q_to, const double* free_qpos, int32_t m, int32_t kinds,
                      double resolution, int32_t* result, double* t_contact);
int rcsh_motion_query_dev(rcsh_sim* sim, const double* q_from_dev, const double* q_to_dev, const double* free_qpos_dev, int32_t m,
                          int32_t kinds, double resolution, int32_t* result_dev, double* t_contact_dev);

/* ---- clearance queries: how far, between which geoms, and which way to move (csrc/clearance_team.h).
 * rcsh_clearance_pairs lists the pairs a clearance query covers for `kinds`, as mjModel geom ids, each pair in MuJoCo's order within
 * a contact, in a fixed order: (1) the floor pairs, in geom order; (2) the self pairs, in the order of the end-of-launch check's
 * table; (3) the free body's pairs, in geom order.  That is exactly the set the point query tests: pairs the tables drop (a
 * parent-child pair across the first hinge) are not in it.  geom_ids [capacity][2]; capacity may be 0 to read *count alone; a robot
 * without collision geoms has count 0.
 * rcsh_clearance_query: q, free_qpos, kinds, RCSH_ERR_MODEL and RCSH_ERR_ARG as rcsh_collision_query; no per-environment state is read
 * or written; the handle's stream.  pair_mask [count] bytes, indexed by the list for the same `kinds`: 0 skips the pair; NULL: every
 * pair.  d_max > 0 (+inf allowed; NaN or <= 0: RCSH_ERR_ARG): pairs farther apart than d_max are not looked for.  Every output but
 * `distance` may be NULL.  Per row:
 *   status [M]  0 apart: distance [M] is the smallest Euclidean distance over the selected pairs, within 1e-9 m;
 *               1 nothing within d_max: distance == d_max, pair -1 -1, witness and grad zeros;
 *               2 in contact (some selected pair penetrates by more than 1e-9 m, the point query's predicate): distance is minus the
 *                 depth of the deepest penetrating pair -- the depth of the contact pass's narrow phase (MPR; the lowest point against
 *                 the floor; the box-box collider's depth for two boxes);
 *               3 not converged (the distance iteration met its cap of 64 support queries): distance is the proven lower bound, never
 *                 more than the truth; pair and witness are the iteration's last;
 *   pair [M][2]     the pair that attains `distance` (ties: the lowest list index);
 *   witness [M][6]  world points wa on the first geom and wb on the second, in the list's order (a capsule's is the point of its
 *                   core segment: |wb - wa| minus the capsules' radii is the distance); status 2: the contact position
 *                   +- half the depth along the contact normal (wa = pos + n depth / 2, wb = pos - n depth / 2);
 *   grad [M][nl]    d(distance)/dq_j with the witnesses held fixed on their geoms: n . (v_b,j - v_a,j), n = (wb - wa) / |wb - wa|
 *                   (status 2: the contact normal, from the first geom to the second), v_x,j = axis_j x (w_x - anchor_j) for a hinge
 *                   among the ancestors of x's link, axis_j for a slide, 0 otherwise (geoms welded to the world, the floor and the
 *                   free body do not move).
 * rcsh_env_clearance asks the same once per environment (M = n_envs): the row is the environment's own chain configuration (arm
 * joints and finger slides, what the collision guard reads) and, with bit 2 of `kinds` in a scene with a free body, the body at the
 * environment's own pose.  It writes nothing but its outputs. */
int rcsh_clearance_pairs(rcsh_sim* sim, int32_t kinds, int32_t* geom_ids, int32_t capacity, int32_t* count);
int rcsh_clearance_query(rcsh_sim* sim, const double* q, const double* free_qpos, int32_t m, int32_t kinds, const uint8_t* pair_mask,
                         double d_max, double* distance, uint8_t* status, int32_t* pair, double* witness, double* grad);
int rcsh_clearance_query_dev(rcsh_sim* sim, const double* q_dev, const double* free_qpos_dev, int32_t m, int32_t kinds,
                             const uint8_t* pair_mask_dev, double d_max, double* distance_dev, uint8_t* status_dev, int32_t* pair_dev,
                             double* witness_dev, double* grad_dev);
int rcsh_env_clearance(rcsh_sim* sim, int32_t kinds, const uint8_t* pair_mask, double d_max, double* distance, uint8_t* status,
                       int32_t* pair, double* witness, double* grad);
int rcsh_env_clearance_dev(rcsh_sim* sim, int32_t kinds, const uint8_t* pair_mask_dev, double d_max, double* distance_dev,
                           uint8_t* status_dev, int32_t* pair_dev, double* witness_dev, double* grad_dev);

/* ---- swept clearance: the smallest distance along a joint-space motion, bracketed (csrc/swept_team.h).
 * A row is the straight segment q(s) = q_from + s (q_to - q_from), s in [0, 1], over the nl chain joints (finger slides included), as
 * rcsh_motion_query takes it.  kinds, free_qpos (the body stands still at that pose for the whole segment), pair_mask (indexed by
 * rcsh_clearance_pairs) and d_max mean what they mean for rcsh_clearance_query; `tolerance` (> 0, m) is the bracket width asked for;
 * `resolution` (> 0, rad or m) is rcsh_motion_query's: a piece whose largest joint travel is at most this is not split further.
 * The bracket rests on the motion certificate's levers: over a piece of width w in s a pair's distance changes by at most w L_p, so
 *   min over [a, b] of d_p >= (d_p(a) + d_p(b) - w L_p) / 2.
 * `distance` is the smallest exact clearance among the sampled configurations (an upper bound of the minimum, attained at `s`);
 * `lower` is the smallest bound of any piece of the segment (a PROVEN lower bound of the clearance over the whole segment).
 * Every output pointer of rcsh_swept_out but `distance` may be NULL.  Per row:
 *   distance [M]   the clearance at q(s): what rcsh_clearance_query answers for that configuration;
 *   lower [M]      lower <= distance; never more than the true minimum where it is finite;
 *   s [M]          the parameter at which `distance` is attained;
 *   pair [M][2], witness [M][6], grad [M][nl]   rcsh_clearance_query's outputs at q(s): the same conventions, tie rule and capsule-core
 *                  witnesses;
 *   evals [M]      configurations evaluated for the row: at most 2048 while it minimises, at most 256 more once a contact was sampled;
 *   status [M]     0 bracketed: distance - lower <= tolerance;
 *                  1 beyond: proven -- no selected pair comes within d_max anywhere on the segment: distance == lower == d_max, s = -1,
 *                    pair -1 -1, witness and grad zeros;
 *                  2 contact: a sampled configuration penetrates by more than 1e-9 m (the point query's predicate).  s is the smallest
 *                    sampled parameter in contact, after the part of the segment before it has been searched as rcsh_motion_query
 *                    searches it (pieces certified free, or bisected down to `resolution`); distance, pair, witness and grad are
 *                    rcsh_clearance_query's status-2 answer there; lower = -inf.  The minimisation stops: the deepest penetration along
 *                    the path is not looked for;
 *                  3 open: the bracket is valid but wider than `tolerance` -- the evaluation budget or the piece stack ran out,
 *                    `resolution` stopped the splitting, the distance iteration of the best sample met its cap, or a finger slide
 *                    leaves the stroke the levers were built for (then nothing can be proven: lower = -inf, and the segment is sampled
 *                    at s = k / 32).  Where no sampled configuration came within d_max but that could not be proven for the whole
 *                    segment, distance == d_max, s = -1, pair -1 -1 and lower < d_max.
 * For every status but 1, `distance` is a value the clearance really takes on the segment, at `s`; a q_from == q_to row gives s = 0
 * and the point query's answer.  Results depend on the row alone.  The bound is Lipschitz only: a distance that stays flat while the
 * levers are large (joint 1 turning the arm about the vertical above the floor) converges slowly and ends as status 3 with a valid
 * bracket.  One mask per call; no per-pair output.
 * RCSH_ERR_MODEL and RCSH_ERR_ARG as rcsh_clearance_query, plus tolerance or resolution that is not finite or is <= 0.  M = 0 does
 * nothing; an error leaves outputs and state untouched.  Robots without collision geometry answer status 1 for every row.
 * rcsh_env_swept_clearance asks the same once per environment (M = n_envs): the start is the environment's own chain configuration,
 * the end is q_to [N][nl], the free body is at the environment's own pose.  It writes nothing but its outputs. */
typedef struct rcsh_swept_out {
  double* distance;  /* [M] (required) */
  double* lower;     /* [M] */
  double* s;         /* [M] */
  int32_t* pair;     /* [M][2] */
  double* witness;   /* [M][6] */
  double* grad;      /* [M][nl] */
  int32_t* evals;    /* [M] */
  uint8_t* status;   /* [M] */
} rcsh_swept_out;
int rcsh_swept_clearance(rcsh_sim* sim, const double* q_from, const double* q_to, const double* free_qpos, int32_t m, int32_t kinds,
                         const uint8_t* pair_mask, double d_max, double tolerance, double resolution, const rcsh_swept_out* out);
int rcsh_swept_clearance_dev(rcsh_sim* sim, const double* q_from_dev, const double* q_to_dev, const double* free_qpos_dev, int32_t m,
                             int32_t kinds, const uint8_t* pair_mask_dev, double d_max, double tolerance, double resolution,
                             const rcsh_swept_out* out_dev);
int rcsh_env_swept_clearance(rcsh_sim* sim, const double* q_to, int32_t kinds, const uint8_t* pair_mask, double d_max, double tolerance,
                             double resolution, const rcsh_swept_out* out);
int rcsh_env_swept_clearance_dev(rcsh_sim* sim, const double* q_to_dev, int32_t kinds, const uint8_t* pair_mask_dev, double d_max,
                                 double tolerance, double resolution, const rcsh_swept_out* out_dev);

/* ---- dynamics queries: the joint-space inertia, the bias forces and the TCP Jacobian at caller-supplied states
 * (csrc/dynamics_team.h).  What a model-based controller reads off the reference's `sim.data` -- qM (mj_fullM), qfrc_bias,
 * qfrc_gravcomp, mj_jac of the TCP -- and what the reference's hardware driver takes from libfranka every cycle (model.mass, coriolis,
 * gravity, zeroJacobian; extensions/rcs_fr3/src/hw/FR3.cpp:241-340), for M rows at once.  Like the collision queries
 * rcsh_dynamics_query reads and writes NO per-environment state, is independent of n_envs and runs on the handle's stream.
 * Rows are [M][nl], the robot chain's joints including the finger slides (rad, m): q; qvel (rad/s, m/s; NULL: zero); qacc_in
 * (rad/s^2, m/s^2; read only when qfrc_inverse is asked for); qfrc_in (N m, N; read only when qacc is asked for).  In a scene with a
 * free body the query covers the chain's nl degrees of freedom: the body's block of the inertia is decoupled from them.
 * Every output pointer of rcsh_dynamics_out may be NULL (not wanted); an output's bits do not depend on which others are asked for.
 * Per row, SI units, MuJoCo's signs:
 *   qM [M][nl][nl]       the full symmetric joint-space inertia, armature on the diagonal (mj_fullM of mjData.qM);
 *   qfrc_bias [M][nl]    Coriolis, centrifugal and gravity forces C(q, qvel) qvel + g(q): inverse dynamics at zero acceleration
 *                        (mjData.qfrc_bias; the equation of motion is M qacc + qfrc_bias = applied forces);
 *   gravity [M][nl]      qfrc_bias at qvel = 0, i.e. g(q); the Coriolis / centrifugal part is qfrc_bias - gravity;
 *   qfrc_gravcomp [M][nl] the gravity-compensation force of the bodies' `gravcomp` (mjData.qfrc_gravcomp: a passive or, with
 *                        actuatorgravcomp, an actuator-side force that the stepping kernels ADD to the applied forces; it equals
 *                        `gravity` where every body has gravcomp = 1);
 *   jac [M][6][nl]       the geometric Jacobian of the TCP: rows 0-2 d(position)/dq_j, rows 3-5 the angular velocity per unit joint
 *                        rate, expressed in the robot-base frame -- the frame rcsh_ik_forward reports its pose in, so central
 *                        differences of rcsh_ik_forward reproduce it.  The TCP is the pose rcsh_ik_forward returns for the same
 *                        tcp_offset7 (x y z qx qy qz qw): the attachment site composed with the INVERSE offset (reference quirk Q7);
 *                        tcp_offset7 NULL: the site itself (not the robot config's offset).  Columns of joints that are not
 *                        ancestors of the site's link (the finger slides) are zero;
 *   qfrc_inverse [M][nl] M qacc_in + qfrc_bias: rigid-body inverse dynamics of the chain;
 *   qacc [M][nl]         M^-1 (qfrc_in - qfrc_bias) by the LDL^T factorisation the stepping kernels use: forward dynamics of the
 *                        UNCONSTRAINED chain.
 * NOT included in any output: actuator forces, joint damping, dry friction (frictionloss), joint-limit, equality (the fingers'
 * coupling) and contact forces; the caller adds what it models to qfrc_in.
 * RCSH_ERR_STATE: no robot attached.  RCSH_ERR_ARG: M < 0; a null q or a null `out` where M > 0; qfrc_inverse asked for without
 * qacc_in, or qacc without qfrc_in; a non-finite input entry (host forms only: the _dev forms do not read the values on the host); a
 * tcp_offset7 quaternion of zero norm.  M = 0 does nothing.  tcp_offset7 is a host pointer in both forms.
 * rcsh_env_dynamics asks the same once per environment (M = n_envs): the row is the environment's own chain qpos and qvel; qacc_in
 * and qfrc_in are [N][nl] as above.  It writes nothing but its outputs. */
typedef struct rcsh_dynamics_out {
  double* qM;             /* [M][nl][nl] */
  double* qfrc_bias;      /* [M][nl] */
  double* gravity;        /* [M][nl] */
  double* qfrc_gravcomp;  /* [M][nl] */
  double* jac;            /* [M][6][nl] */
  double* qfrc_inverse;   /* [M][nl]; needs qacc_in */
  double* qacc;           /* [M][nl]; needs qfrc_in */
} rcsh_dynamics_out;
int rcsh_dynamics_query(rcsh_sim* sim, const double* q, const double* qvel, const double* qacc_in, const double* qfrc_in, int32_t m,
                        const double* tcp_offset7, const rcsh_dynamics_out* out);
int rcsh_dynamics_query_dev(rcsh_sim* sim, const double* q_dev, const double* qvel_dev, const double* qacc_in_dev,
                            const double* qfrc_in_dev, int32_t m, const double* tcp_offset7, const rcsh_dynamics_out* out_dev);
int rcsh_env_dynamics(rcsh_sim* sim, const double* qacc_in, const double* qfrc_in, const double* tcp_offset7,
                      const rcsh_dynamics_out* out);
int rcsh_env_dynamics_dev(rcsh_sim* sim, const double* qacc_in_dev, const double* qfrc_in_dev, const double* tcp_offset7,
                          const rcsh_dynamics_out* out_dev);

/* ---- dynamics derivatives: how qfrc_inverse and qacc of the dynamics queries change with the state (csrc/dynamics_grad_team.h).
 * What iLQR / DDP, SQP-style MPC and linearised feedback need of the chain, analytically (the differentiated recursive Newton-Euler
 * pass; no finite difference on the device), for M rows at once.  Rows q, qvel (NULL: zero), qacc_in, qfrc_in are [M][nl] as in
 * rcsh_dynamics_query; like it the call reads and writes NO per-environment state and runs on the handle's stream.
 * Every output is [M][nl][nl] row-major, element [i][k] the derivative of component i by variable k; every pointer of
 * rcsh_dynamics_grad_out may be NULL (not wanted), and an output's bits do not depend on which others are asked for:
 *   dqfrc_inverse_dq     d(M(q) qacc_in + qfrc_bias(q, qvel)) / dq at the row's (q, qvel, qacc_in);
 *   dqfrc_inverse_dqvel  d qfrc_bias / d qvel (does not depend on qacc_in);
 *   dqacc_dq             d(M^-1 (qfrc_in - qfrc_bias)) / dq = -M^-1 d(qfrc_inverse)/dq taken at the row's own qacc;
 *   dqacc_dqvel          -M^-1 d qfrc_bias / d qvel;
 *   qM_inv               M^-1, full symmetric: d qacc / d qfrc_in.
 * They differentiate exactly what rcsh_dynamics_query returns: armature is part of M, the finger slides are part of the chain, and no
 * actuator, damping, gravity-compensation, limit, equality, friction or contact term enters.
 * RCSH_ERR_STATE: no robot attached.  RCSH_ERR_ARG: M < 0; a null q or a null `out` where M > 0; dqfrc_inverse_dq asked for without
 * qacc_in; dqacc_dq or dqacc_dqvel without qfrc_in; a non-finite input entry (host forms only).  M = 0 does nothing.
 * rcsh_env_dynamics_derivatives asks the same once per environment (M = n_envs) at the environment's own chain qpos and qvel;
 * qacc_in and qfrc_in are [N][nl].  It writes nothing but its outputs. */
typedef struct rcsh_dynamics_grad_out {
  double* dqfrc_inverse_dq;     /* [M][nl][nl]; needs qacc_in */
  double* dqfrc_inverse_dqvel;  /* [M][nl][nl] */
  double* dqacc_dq;             /* [M][nl][nl]; needs qfrc_in */
  double* dqacc_dqvel;          /* [M][nl][nl]; needs qfrc_in */
  double* qM_inv;               /* [M][nl][nl] */
} rcsh_dynamics_grad_out;
int rcsh_dynamics_derivatives(rcsh_sim* sim, const double* q, const double* qvel, const double* qacc_in, const double* qfrc_in,
                              int32_t m, const rcsh_dynamics_grad_out* out);
int rcsh_dynamics_derivatives_dev(rcsh_sim* sim, const double* q_dev, const double* qvel_dev, const double* qacc_in_dev,
                                  const double* qfrc_in_dev, int32_t m, const rcsh_dynamics_grad_out* out_dev);
int rcsh_env_dynamics_derivatives(rcsh_sim* sim, const double* qacc_in, const double* qfrc_in, const rcsh_dynamics_grad_out* out);
int rcsh_env_dynamics_derivatives_dev(rcsh_sim* sim, const double* qacc_in_dev, const double* qfrc_in_dev,
                                      const rcsh_dynamics_grad_out* out_dev);

/* ---- operational-space dynamics of the TCP (csrc/opspace_team.h): what a task-space controller forms from qM, qfrc_bias and jac,
 * formed on the device for M rows at once, plus the TCP's velocity-product acceleration.  Rows q, qvel (NULL: zero) are [M][nl] as
 * in rcsh_dynamics_query; like it the call reads and writes NO per-environment state and runs on the handle's stream.
 * Definitions, per row, everything in the robot-base frame of `jac`, the TCP that of rcsh_dynamics_query for the same tcp_offset7:
 *   J      `jac` [6][nl] with the rows NOT selected by task_mask set to zero (bit r selects row r; rows 0-2 linear, 3-5 angular);
 *   Minv   the full chain's M^-1, the matrix rcsh_dynamics_derivatives returns as qM_inv: armature and the finger slides included;
 *   b      qfrc_bias;
 *   A      J Minv J^T + damping * I_sel, I_sel the identity on the selected rows; damping >= 0 is in the units of A's diagonal.
 * Outputs (every pointer of rcsh_opspace_out may be NULL: not wanted; an output's bits do not depend on which others are asked for):
 *   twist       [M][6]       J qvel;
 *   jdot_qvel   [M][6]       the TCP's acceleration at qacc = 0: linear part the classical acceleration of the TCP point, d^2 p/dt^2,
 *                            angular part d omega/dt, so that d(twist)/dt = J qacc + jdot_qvel.  Masked rows are zero.  Analytic.
 *   lambda_inv  [M][6][6]    A.  Always defined.
 *   lambda      [M][6][6]    A^-1 on the selected rows and columns, zero elsewhere;
 *   jbar        [M][nl][6]   Minv J^T lambda, the dynamically consistent inverse of J;
 *   op_bias     [M][6]       jbar^T b - lambda jdot_qvel: the task force for a task acceleration xacc is lambda xacc + op_bias;
 *   null_proj   [M][nl][nl]  I - J^T jbar^T, used as tau = J^T F + null_proj tau0;
 *   qfrc        [M][nl]      J^T (lambda xacc_des + op_bias) + null_proj qfrc_null.  Needs xacc_des [M][6]; qfrc_null [M][nl], NULL: zero;
 *   status      [M] int32    0: fine.  1: A is not positive definite to working precision.
 * The status rule: A restricted to the selected rows is factored L D L^T without pivoting; a row gets status 1 when some
 * d_i <= RCSH_OPSPACE_REL_PIVOT * A_ii, when d_i is not finite, or when A_ii <= 0.  In a status-1 row every entry of lambda, jbar,
 * op_bias, null_proj and qfrc is NaN; twist, jdot_qvel and lambda_inv are always written.
 * Forces NOT included: as with the other dynamics queries no actuator, damping, gravity-compensation, limit, equality, friction or
 * contact force enters.  qfrc cancels b in the task space only: the caller puts gravity compensation (or -qfrc_gravcomp, where the
 * scene compensates already) into qfrc_null or adds it afterwards.
 * rcsh_opspace_opts is a host struct in every form; NULL means the site itself, task_mask 0x3F and damping 0.
 * RCSH_ERR_STATE: no robot attached.  RCSH_ERR_ARG: M < 0; a null q or a null `out` where M > 0; qfrc asked for without xacc_des;
 * task_mask 0 or above 0x3F; a negative or non-finite damping; a zero-norm offset quaternion; a non-finite input entry (host forms
 * only).  M = 0 does nothing.
 * rcsh_env_opspace asks the same once per environment (M = n_envs) at the environment's own chain qpos and qvel; xacc_des is [N][6],
 * qfrc_null [N][nl].  It writes nothing but its outputs. */
#define RCSH_OPSPACE_REL_PIVOT 1e-10 /* the status rule's bound on d_i / A_ii: a specification, not a measurement */
typedef struct rcsh_opspace_opts {
  const double* tcp_offset7; /* x y z qx qy qz qw as in rcsh_dynamics_query; NULL: the site itself */
  uint32_t task_mask;        /* bit r: row r of J is part of the task; 0x3F: all six */
  double damping;            /* >= 0, added to A's selected diagonal */
} rcsh_opspace_opts;
typedef struct rcsh_opspace_out {
  double* twist;      /* [M][6] */
  double* jdot_qvel;  /* [M][6] */
  double* lambda_inv; /* [M][6][6] */
  double* lambda;     /* [M][6][6] */
  double* jbar;       /* [M][nl][6] */
  double* op_bias;    /* [M][6] */
  double* null_proj;  /* [M][nl][nl] */
  double* qfrc;       /* [M][nl]; needs xacc_des */
  int32_t* status;    /* [M] */
} rcsh_opspace_out;
int rcsh_opspace_query(rcsh_sim* sim, const double* q, const double* qvel, const double* xacc_des, const double* qfrc_null, int32_t m,
                       const rcsh_opspace_opts* opts, const rcsh_opspace_out* out);
int rcsh_opspace_query_dev(rcsh_sim* sim, const double* q_dev, const double* qvel_dev, const double* xacc_des_dev,
                           const double* qfrc_null_dev, int32_t m, const rcsh_opspace_opts* opts, const rcsh_opspace_out* out_dev);
int rcsh_env_opspace(rcsh_sim* sim, const double* xacc_des, const double* qfrc_null, const rcsh_opspace_opts* opts,
                     const rcsh_opspace_out* out);
int rcsh_env_opspace_dev(rcsh_sim* sim, const double* xacc_des_dev, const double* qfrc_null_dev, const rcsh_opspace_opts* opts,
                         const rcsh_opspace_out* out_dev);

/* ---- torque control (csrc/torque_team.h).  A robot is TORQUE-ACTUATED when every arm actuator has biastype none and a zero biasprm
 * (MJCF <motor>; rcs_amd.mjcf.torque_actuated_scene writes such a variant of a shipped scene): its ctrl is a joint torque, clamped by
 * ctrlrange and the joint's actuatorfrcrange like any ctrl.  A mixed arm is not torque-actuated.
 * rcsh_robot_set_joint_torque writes the arm's ctrl ([N][dof]) of the masked environments and nothing else: target, previous angles,
 * the moving / arrived flags and the gripper's ctrl stay.  RCSH_ERR_ARG on a robot that is not torque-actuated.
 * On a torque-actuated robot rcsh_sim_step holds ctrl over the launch as ever; rcsh_sim_step_until_convergence and
 * rcsh_robot_set_cartesian_position return RCSH_ERR_ARG (the predicates and the CLIK assume position servos);
 * rcsh_robot_set_joint_position, rcsh_robot_move_home, rcsh_robot_reset and rcsh_robot_set_joints_hard write target / previous
 * angles / qpos as before but ZERO to the arm's ctrl, and set the law's targets to that configuration and its TCP pose.
 *
 * The law at substep rate.  rcsh_sim_step_torque(k) runs k substeps in one launch and evaluates, before each, at the state the substep
 * starts on (robot-base frame; TCP, Jacobian and every term as rcsh_dynamics_query / rcsh_opspace_query define them for tcp_offset7,
 * task_mask and damping):
 *   x_err     = [p_des - p ; rotvec(R_des R^T)]                 rotvec: the rotation vector on the shorter arc
 *   xacc      = task_k * x_err - task_d * twist                 (diagonal gains, on the task acceleration)
 *   qfrc_null = joint_k * (q_des - q) - joint_d * qvel  (+ qfrc_bias if compensate_bias)       finger entries: 0 (+ qfrc_bias)
 *   tau       = J^T (lambda xacc + op_bias) + null_proj qfrc_null - qfrc_gravcomp
 *   ctrl[arm] = tau[arm]                                        (the finger entries are dropped; the gripper's ctrl is the caller's)
 * task_mask = 0 is the pure joint law: tau = qfrc_null - qfrc_gravcomp.  enabled = 0: no law, ctrl is the caller's.
 * Where the opspace status would be 1 the substep keeps the torque of the substep before and the environment's `singular` byte is
 * raised (rcsh_torque_status; sticky until rcsh_sim_reset / rcsh_robot_reset of that environment); no NaN reaches ctrl: a torque
 * that comes out non-finite (a NaN or zero-quaternion target written through the _dev form, which validates nothing) is held back
 * the same way.  The pose targets that the resets and set_joint_position leave are formed with the tcp_offset7 configured at that
 * moment (before any rcsh_torque_configure: the site itself): after configuring another offset, set the targets again.
 * rcsh_sim_step_torque runs no position-servo bookkeeping: the is_moving / is_arrived callbacks and their timestamps stay as they
 * were while `time` advances, so a later rcsh_sim_step fires them against the old timestamps.
 * After the launch ctrl holds the last torque applied (rcsh_sim_get_ctrl), and the launch ends with the handle's check for contacts
 * nobody resolves, as rcsh_sim_step does.
 * rcsh_torque_set_target: pose7 [N][7] (x y z qx qy qz qw, base frame) and / or q_des [N][dof]; NULL keeps; masked.
 * RCSH_ERR_ARG from rcsh_torque_configure and rcsh_sim_step_torque: the robot is not torque-actuated, the scene has a free body,
 * robot contacts are resolved, rate-driven cameras are scheduled, the site is static; a task_mask above 0x3F, a negative or
 * non-finite damping or gain, a zero-norm offset quaternion; k < 0.  RCSH_ERR_STATE: no robot.  RCSH_ERR_MODEL: no kernel for the
 * archetype (dry joint friction other than on the 7-dof arm without gripper). */
#define RCSH_MAX_ARM 8
typedef struct rcsh_torque_law {
  int32_t enabled;        /* 0: ctrl is the caller's (rcsh_robot_set_joint_torque) */
  uint32_t task_mask;     /* as rcsh_opspace_opts; 0: pure joint law */
  double damping;         /* as rcsh_opspace_opts */
  double tcp_offset7[7];  /* x y z qx qy qz qw as in rcsh_dynamics_query; all zero: the site itself */
  double task_k[6], task_d[6];                       /* diagonal, on the task acceleration, robot-base frame */
  double joint_k[RCSH_MAX_ARM], joint_d[RCSH_MAX_ARM]; /* null-space / joint impedance */
  int32_t compensate_bias; /* add qfrc_bias to the null-space torque */
} rcsh_torque_law;
int rcsh_robot_is_torque_actuated(rcsh_sim* sim, int32_t* yes);
int rcsh_robot_set_joint_torque(rcsh_sim* sim, const double* tau /*[N][dof]*/, const uint8_t* mask);
int rcsh_robot_set_joint_torque_dev(rcsh_sim* sim, const double* tau_dev, const uint8_t* mask_dev);
int rcsh_torque_configure(rcsh_sim* sim, const rcsh_torque_law* law);
int rcsh_torque_set_target(rcsh_sim* sim, const double* pose7, const double* q_des, const uint8_t* mask);
int rcsh_torque_set_target_dev(rcsh_sim* sim, const double* pose7_dev, const double* q_des_dev, const uint8_t* mask_dev);
int rcsh_torque_get_target(rcsh_sim* sim, double* pose7 /*[N][7]*/, double* q_des /*[N][dof]*/); /* either may be NULL */
int rcsh_sim_step_torque(rcsh_sim* sim, int64_t k);
int rcsh_torque_status(rcsh_sim* sim, uint8_t* singular /*[N]*/);

/* SimGripper(sim, cfg) -- rcs.cpp:508-515, SimGripper.cpp:13-39 */
int rcsh_sim_add_gripper(rcsh_sim* sim, const rcsh_gripper_desc* gripper);
/* Gripper.set_normalized_width -- rcs.cpp:383-384, SimGripper.cpp:79-92 (RCSH_ERR_ARG outside [0,1] / force<0) */
int rcsh_gripper_set_normalized_width(rcsh_sim* sim, const double* width, double force, const uint8_t* mask);
/* Gripper.get_normalized_width -- rcs.cpp:385, SimGripper.cpp:93-106 */
int rcsh_gripper_get_normalized_width(rcsh_sim* sim, double* width);
/* Gripper.is_grasped -- rcs.cpp:388, SimGripper.cpp:132-141 */
int rcsh_gripper_is_grasped(rcsh_sim* sim, uint8_t* grasped);
/* Gripper.reset -- rcs.cpp:395, SimGripper.cpp:158-165 */
int rcsh_gripper_reset(rcsh_sim* sim, const uint8_t* mask);
/* SimGripper.get_state -- rcs.cpp:514, SimGripperState SimGripper.h:47-52 */
int rcsh_gripper_get_state(rcsh_sim* sim, double* last_commanded_width, uint8_t* is_moving, double* last_width,
                           uint8_t* collision);

/* mjData views the reference reads directly (python/rcs/envs/sim.py:343-411): qpos, qvel, ctrl, time */
int rcsh_sim_get_qpos(rcsh_sim* sim, double* qpos);  /* [N][nq] */
int rcsh_sim_get_qvel(rcsh_sim* sim, double* qvel);
int rcsh_sim_get_ctrl(rcsh_sim* sim, double* ctrl);  /* [N][nu] */
int rcsh_sim_get_time(rcsh_sim* sim, double* time);  /* [N] */
int rcsh_sim_set_qpos(rcsh_sim* sim, const double* qpos, const uint8_t* mask);
int rcsh_sim_set_qvel(rcsh_sim* sim, const double* qvel, const uint8_t* mask);
int rcsh_sim_nq(const rcsh_sim* sim);
int rcsh_sim_nu(const rcsh_sim* sim);

/* One free-floating box on the floor plane -- the `box_geom` body of the reference's pick-up scene
 * (assets/scenes/fr3_simple_pick_up/scene.xml:30-33), whose free joint the task wrappers write and read through
 * mjData: RandomCubePos `sim.data.joint("box_joint").qpos = [...]` (python/rcs/envs/sim.py:379-383),
 * PickCubeSuccessWrapper `sim.data.joint("box_joint").qpos[2]` / `[:3]` (sim.py:399-412).  The description carries
 * the mjModel constants of that body and of its contact pair with the floor (mj_contactParam already applied:
 * friction = element-wise max, solref / solimp mixed) plus the solver options the contact solve reads
 * (assets/fr3/mjcf/fr3_common.xml:3).  qpos is [x y z qw qx qy qz], qvel [linear (world), angular (body frame)].
 * With `resolve_robot_contacts` the robot's collision geoms (finger pads, finger / hand / link hulls, the camera capsule)
 * collide with the box and with the floor, and one constraint problem couples the robot's joints with the box's 6 dofs
 * (FR3 + hand archetype); without it the box touches the floor only. */
typedef struct rcsh_free_box_desc {
  double qpos0[7];
  double mass, inertia[3];   /* centre of mass at the body origin, principal axes = body axes */
  double size[3];            /* half extents of the box geom */
  double friction[3];        /* of the floor / box pair */
  double solref[2], solimp[5];
  double plane_z;            /* floor: z = plane_z, normal +z */
  double impratio;           /* mjOption.impratio */
  double noslip_tolerance;   /* mjOption.noslip_tolerance */
  int32_t noslip_iterations; /* mjOption.noslip_iterations */
  int32_t cone_elliptic;     /* mjOption.cone == mjCONE_ELLIPTIC (the only cone type built) */
  double geom_friction[3];   /* the box geom's own coefficients (mixed with a robot geom's per contact: element-wise max) */
  double floor_friction[3];  /* the floor geom's */
  int32_t resolve_robot_contacts;
  int32_t reserved;
} rcsh_free_box_desc;
int rcsh_sim_add_free_box(rcsh_sim* sim, const rcsh_free_box_desc* box);
/* Scenes WITHOUT a free body: the solver options mjModel.opt carries (reference assets/fr3/mjcf/fr3_common.xml:3) and the
 * default contact parameters, so that contacts of the robot's collision geoms with the floor are resolved (the arm stops
 * on the floor instead of only raising SimRobot's collision flag).  FR3 + hand archetype; elsewhere and with
 * resolve_robot_contacts = 0 robot contacts are detected only. */
typedef struct rcsh_contact_options {
  double impratio, noslip_tolerance;
  int32_t noslip_iterations, cone_elliptic;
  double solref[2], solimp[5];
  /* bit 0: contacts of the robot's geoms with the floor enter the constraint solve (0: detected only).  Bit 1 (round 5): so do
   * contacts between two geoms of the robot -- mj_step2 resolves every entry of mjData.contact (reference src/sim/sim.cpp:108-115).
   * Bit 2 (round 5): environment by environment -- a step is the lean launch over the environments that touch nothing plus the
   * contact-resolving launch over the others; an environment whose geoms are found in contact at the end of a lean launch has
   * that launch redone with its contacts resolved from their first substep (csrc/sim_kernels.h: RunOp::esc_role).  Without bit 2
   * the whole batch runs on the contact-resolving kernel. */
  int32_t resolve_robot_contacts, reserved;
} rcsh_contact_options;
int rcsh_sim_set_contact_options(rcsh_sim* sim, const rcsh_contact_options* options);
/* Per-environment escalation (rcsh_contact_options.resolve_robot_contacts bit 2), [N] flags each, either may be null:
 * `now`: the environment is stepped by the contact-resolving kernel at present; `ever`: a contact of its robot geoms has been
 * resolved since its last rcsh_sim_reset.  All zero where escalation is off. */
int rcsh_sim_contact_escalated(rcsh_sim* sim, uint8_t* now, uint8_t* ever);
/* [N] flags: a contact phase of the environment ran out of contact or link slots since its last rcsh_sim_reset (the tail of MuJoCo's
 * contact order was dropped, so from that substep on the trajectory is not the reference's); the same bit is byte 6 of an env-step's
 * info row. */
int rcsh_sim_contact_overflow(rcsh_sim* sim, uint8_t* overflow);
/* [N] flags: the environment's geoms were found in a contact this configuration does not resolve -- robot <-> floor in scenes
 * that only detect contacts (the default without a free body), robot <-> robot everywhere -- at the end of a stepping launch,
 * since its last rcsh_sim_reset.  MuJoCo resolves every contact of d->contact in every mj_step2 (reference src/sim/sim.cpp:
 * 108-115), so from that launch on the environment's trajectory is not the reference's; the same bit is byte 7 of an
 * env-step's info row.  Checked once per launch on the position the next position stage will see (csrc/check_team.h). */
int rcsh_sim_contact_unresolved(rcsh_sim* sim, uint8_t* unresolved);
/* How often the check runs: at the end of every `every`-th stepping launch (default 1: every launch, the flag comes on in the
 * env-step the contact begins in; 0: never).  The check costs a launch about as much as four physics substeps (~25 us at 4096 environments); a resident
 * rollout that prefers throughput sets a larger cadence -- a contact is then found with a lag of up to `every` - 1 launches, one
 * that comes and goes between two checks is missed -- and rcsh_sim_contact_unresolved() always checks the present state first. */
int rcsh_sim_set_contact_check(rcsh_sim* sim, int32_t every);
/* Admitted geom pairs beyond the 192 the end-of-launch check (and the self-contact stage of the contact-resolving kernels) keeps
 * entries for: they are neither checked nor resolved; the handle is created all the same and the Python host warns.  0 for every
 * shipped scene (fr3_empty_world: 137 pairs).  No reference counterpart: MuJoCo has no such capacity. */
int rcsh_sim_contact_check_unchecked_pairs(rcsh_sim* sim, int32_t* count);
/* Collision geoms of the scene that exceed the contact table's capacity (28 geoms -- 32 until round 4, when the end-of-launch
 * check took LDS for the geoms' world boxes --, 10 boxes, 152 hull vertices) are left out of
 * GEOM-GEOM detection (the floor test still sees them): their mjModel ids (up to `capacity`), how many there are, and why.
 * rcsh_sim_add_robot / rcsh_sim_add_gripper refuse a collision geom that is on this list; the Python host warns about the
 * rest (a world-welded obstacle no callback list names would still count for SimRobot::collision_callback,
 * reference src/sim/SimRobot.cpp:172-182).  No reference counterpart: MuJoCo has no such capacity. */
int rcsh_sim_contact_table_dropped(rcsh_sim* sim, int32_t* geom_ids, int32_t capacity, int32_t* count, char* reason, size_t reason_capacity);
int rcsh_sim_reset_free_box(rcsh_sim* sim);
int rcsh_sim_get_free_qpos(rcsh_sim* sim, double* qpos);  /* [N][7] */
int rcsh_sim_get_free_qvel(rcsh_sim* sim, double* qvel);  /* [N][6] */
int rcsh_sim_set_free_qpos(rcsh_sim* sim, const double* qpos, const uint8_t* mask);
int rcsh_sim_set_free_qvel(rcsh_sim* sim, const double* qvel, const uint8_t* mask);

/* Snapshot / restore of EVERYTHING that evolves (the mjData fields above, the callback scheduler's timestamps and
 * return values, SimRobot / SimGripper state, the wrappers' prev_action / origin / last_action, flags): the reference's
 * closest facility is the GUI bridge's mjSTATE_FULLPHYSICS copy (src/sim/gui_server.cpp:49-60).  The blob is opaque,
 * `rcsh_sim_state_bytes` long, and valid for handles created from the same scene with the same n_envs (it begins with a
 * 16-byte header -- layout version, n_envs, number of state fields -- and rcsh_sim_set_state refuses a blob whose header says
 * otherwise: RCSH_ERR_ARG); restoring and re-running the same calls reproduces the continuation bit for bit. */
size_t rcsh_sim_state_bytes(const rcsh_sim* sim);
int rcsh_sim_get_state(rcsh_sim* sim, void* blob);
int rcsh_sim_set_state(rcsh_sim* sim, const void* blob);

/* ---- fused Gymnasium loop: SimEnvCreator()(...).reset() / .step(action) for N environments in one launch.
 * Wrapper stack restated in the kernel (reference python/rcs/envs/base.py:246-304,469-565,680-735;
 * envs/sim.py:49-76,119-131).  Observation row: tquat[7] joints[dof] xyzrpy[6] gripper[1]
 * (obs_width = 14 + dof); info row (uint8[8]): collision, ik_success, is_sim_converged, is_grasped,
 * truncated, gripper_collision, contact_overflow, contact_unresolved (the last two: no reference counterpart -- a contact
 * phase ran out of slots / the environment was found in a contact this configuration does not resolve, sticky until reset,
 * see rcsh_sim_contact_unresolved) -- `info` rows are written as one 8-byte word each: the buffer must be 8-byte aligned --;
 * gripper_width[N] (double).
 *
 * Torque and impedance control modes (RCSH_MODE_TORQUE .. RCSH_MODE_CARTESIAN_IMPEDANCE_TQUAT; csrc/env_torque_team.h), for
 * torque-actuated robots (rcsh_robot_is_torque_actuated).  Action row: TORQUE [dof] joint torques (N m); JOINT_IMPEDANCE [dof]
 * joint positions; CARTESIAN_IMPEDANCE_TRPY [6] xyzrpy; CARTESIAN_IMPEDANCE_TQUAT [7] xyz + xyzw.  One step is ONE stepping launch
 * -- the wrappers' action(), the target write and round(1 / frequency / timestep) substeps -- and the handle's observing pass:
 *   gripper           GripperWrapper.action as in the position modes;
 *   TORQUE            ctrl[arm] = action, held over the substeps (clamped by ctrlrange in the substep like any ctrl); no law, no
 *                     relative action space, no 1e-3 gate;
 *   JOINT_IMPEDANCE   the JOINTS mode's RelativeActionSpace arithmetic and RobotEnv.step's gate; a commanded action becomes the
 *                     law's q_des, a gated-out one leaves the target; nothing of the position servo's bookkeeping (ctrl, target /
 *                     previous angles, is_moving / is_arrived) is written;
 *   CARTESIAN_*       the Cartesian modes' wrapper arithmetic and gate; a commanded pose becomes the law's pose target.  The env
 *                     layer's poses are those of rcsh_robot_get_cartesian_position: the site composed with the robot's tcp_offset.
 *                     The law's TCP is the site composed with the INVERSE of its tcp_offset7 (quirk Q7): step and reset return
 *                     RCSH_ERR_ARG unless both are the same TCP, i.e. unless the law's tcp_offset7 is the inverse of the robot's
 *                     tcp_offset (all-zero counts as the identity, quaternions are compared up to sign);
 *   the impedance modes evaluate the law before every substep exactly as rcsh_sim_step_torque does, the singular / non-finite
 *   hold-back and the sticky `singular` byte included.
 * rcsh_env_reset in these modes: gripper reset, qpos := qpos0, arm := q_home, qvel := 0, ALL of ctrl := 0 (never q_home: ctrl is a
 * torque), time and callback timestamps := 0, the sticky contact flags and the `singular` byte cleared, the law's q_des := q_home and
 * its pose target := the TCP pose there; one substep (under the law; with zero torque in TORQUE mode); the relative-action origin :=
 * the state after it; the observing pass.  Autoreset uses this reset.  `substeps` reports the substeps of the stepping launch.
 * `collision` in the info row stays what the flags word holds: no collision detection runs in these modes, contact_unresolved is
 * the signal.
 * Refused, changing nothing -- RCSH_ERR_ARG: a robot that is not torque-actuated; a scene rcsh_sim_step_torque refuses (free body,
 * resolved robot contacts, scheduled cameras, static site -- at configure time and again at every step and reset); async_control = 0;
 * TORQUE with relative_to != RCSH_REL_NONE; the TCP mismatch; an env step of round(1 / frequency / timestep) < 1 substeps (step and
 * reset).  RCSH_ERR_STATE: an impedance mode without an enabled law (step and reset); together with the collision guard or the
 * pick task, in either order.  RCSH_ERR_MODEL: no kernel instance (dry friction on another archetype than rcsh_sim_step_torque's). */
int rcsh_env_configure(rcsh_sim* sim, const rcsh_env_desc* env);
int rcsh_env_obs_width(const rcsh_sim* sim);
int rcsh_env_action_width(const rcsh_sim* sim);
int rcsh_env_reset(rcsh_sim* sim, const uint8_t* mask, double* obs, uint8_t* info, double* gripper_width);
int rcsh_env_step(rcsh_sim* sim, const double* action, const float* gripper, double* obs, uint8_t* info,
                  double* gripper_width, int32_t* substeps);
/* device-pointer forms used by the rollout loop (nothing crosses PCIe) */
int rcsh_env_reset_dev(rcsh_sim* sim, const uint8_t* mask_dev, double* obs_dev, uint8_t* info_dev,
                       double* gripper_width_dev);
int rcsh_env_step_dev(rcsh_sim* sim, const double* action_dev, const float* gripper_dev, double* obs_dev,
                      uint8_t* info_dev, double* gripper_width_dev, int32_t* substeps_dev);

/* Task layer of the pick-up scene: SimTaskEnvCreator()(...) = SimEnvCreator with RandomCubePos under the
 * RobotSimWrapper and PickCubeSuccessWrapper on top (python/rcs/envs/creators.py:131-187; the registered gym id
 * rcs/FR3SimplePickUpSim-v0, python/rcs/__init__.py:67-70).
 *  - reset: RandomCubePos.reset (python/rcs/envs/sim.py:365-383) runs the inner reset, steps once, writes the box
 *    pose and the RobotSimWrapper steps once more; `box_qpos` [N][7] is the pose each environment writes (the
 *    reference draws x, y and the quaternion's w from numpy's global generator; the caller draws them here).
 *  - step: PickCubeSuccessWrapper.step (sim.py:396-431); `task` [N][9] receives the box pose (7), the reward and
 *    success (0/1 -- the wrapper returns it as `terminated` and info["success"]).
 * ee_home / success_height are the wrapper's constants EE_HOME and 0.15 + 0.852. */
typedef struct rcsh_pick_task_desc {
  double ee_home[3];
  double success_height;
} rcsh_pick_task_desc;
int rcsh_env_configure_pick_task(rcsh_sim* sim, const rcsh_pick_task_desc* task);
int rcsh_env_reset_task(rcsh_sim* sim, const uint8_t* mask, const double* box_qpos, double* obs, uint8_t* info, double* gripper_width);
int rcsh_env_step_task(rcsh_sim* sim, const double* action, const float* gripper, double* obs, uint8_t* info, double* gripper_width,
                       int32_t* substeps, double* task);
int rcsh_env_reset_task_dev(rcsh_sim* sim, const uint8_t* mask_dev, const double* box_qpos_dev, double* obs_dev, uint8_t* info_dev,
                            double* gripper_width_dev);
int rcsh_env_step_task_dev(rcsh_sim* sim, const double* action_dev, const float* gripper_dev, double* obs_dev, uint8_t* info_dev,
                           double* gripper_width_dev, int32_t* substeps_dev, double* task_dev);

/* Collision guard of the fused loop: the reference's CollisionGuard wrapper (python/rcs/envs/sim.py:156-287), which sits between
 * RelativeActionSpace and RobotEnv.step, for N environments and decided on the device.  Before a guarded step one launch asks, per
 * environment, the motion query's question about the environment's OWN segment: from its current chain configuration (arm joints
 * and finger slides) to the absolute joint command this action would hand to RobotEnv.step (the relative action space's arithmetic,
 * recomputed without touching what it remembers), finger slides kept, the free body -- kinds bit 2, scenes that have one -- at the
 * environment's own current pose.  result / t_contact are the motion query's (0 free: PROVEN by the lever certificate, 1 contact,
 * 2 undecided), with two differences that the guard's fixed finger slides allow:
 *  - a pair of geoms none of whose separating joints travels over the segment (finger against finger, finger against hand) keeps
 *    its relative pose and is decided by the sample at the segment's start alone -- the closed hand's pads touch at a gap of
 *    exactly 0, which passes no certificate: the motion query reports such a row 2, the guard does not;
 *  - a finger slide up to 0.5 mm past the stroke the levers were built for is still certified (an open finger rests on its joint
 *    limit and the soft limit lets it through by micrometres; the levers carry a millimetre of additive slack), where the motion
 *    query reports such a row 2.
 * blocked = result 1, or result 2 with block_undecided.  A blocked environment steps like every other one, but RobotEnv.step
 * receives its current joint position instead of the action's command (the relative action space advances on the original action,
 * the gripper command applies unchanged); with `truncate` its info row reports truncated.  An environment in contact at the start
 * of its segment is blocked (result 1, t_contact 0) until it is reset.
 * Two deviations from the reference, on purpose: the decision is the kinematic certificate, not a shadow simulation; and a blocked
 * environment is stepped with the hold command and observed afresh, where the reference returns its previous observation.
 * Joint-space control only: RCSH_ERR_STATE in a Cartesian control mode (configuring, and peeking; rcsh_env_configure refuses a
 * Cartesian mode while a guard is enabled) or before rcsh_env_configure; RCSH_ERR_ARG for kinds outside 1..7 or resolution <= 0;
 * RCSH_ERR_MODEL where the motion query refuses the scene.  A refused call changes nothing.  The guard keeps no state that outlives
 * a step. */
typedef struct rcsh_guard_desc {
  int32_t enabled;         /* 0: the steps run unguarded (rcsh_env_guard_peek still answers) */
  int32_t kinds;           /* as rcsh_motion_query: bit 0 floor, 1 self, 2 free body (ignored in a scene without one) */
  double resolution;       /* as rcsh_motion_query, > 0 */
  int32_t block_undecided; /* result 2 blocks too */
  int32_t truncate;        /* blocked environments report truncated (info row, byte 4) */
} rcsh_guard_desc;
int rcsh_env_configure_guard(rcsh_sim* sim, const rcsh_guard_desc* guard);
/* The guard's decision for an action batch [N][dof], without stepping and without writing any state. */
int rcsh_env_guard_peek(rcsh_sim* sim, const double* action, int32_t* result, double* t_contact, uint8_t* blocked);
int rcsh_env_guard_peek_dev(rcsh_sim* sim, const double* action_dev, int32_t* result_dev, double* t_contact_dev, uint8_t* blocked_dev);
/* The record of the most recent guarded step (RCSH_ERR_STATE: there was none): copied to the host, or as device pointers that stay
 * valid for the handle's life and are rewritten by every guarded step. */
int rcsh_env_guard_last(rcsh_sim* sim, int32_t* result, double* t_contact, uint8_t* blocked);
int rcsh_env_guard_last_dev(rcsh_sim* sim, const int32_t** result_dev, const double** t_contact_dev, const uint8_t** blocked_dev);


/* Depth images: the pixel path of SimCameraSet (reference src/sim/camera.cpp:86-140 render_single -> mjv_updateScene,
 * mjr_render, mjr_readPixels; python/rcs/camera/sim.py:45-115 for the row flip, the conversion to metres and the
 * uint16 millimetre image, the intrinsics and the extrinsics).  The reference rasterises MuJoCo's visual geoms with
 * OpenGL; this backend casts one ray per pixel against the shapes given here (floor plane, boxes, convex hulls of the
 * collision meshes), expressed in the frame of the link they ride on (-1: world, -2: the free box).  Colour: rcsh_sim_set_render_colours.
 * Frames are those of the last position stage, as mjData.geom_xpos / cam_xpos are. */
typedef struct rcsh_render_scene_desc {
  int32_t nshape, nplanes;
  const int32_t* shape;      /* [nshape] 0 plane (z = 0 of the shape frame, seen from +z), 1 box, 2 convex hull, 3 capsule (axis z) */
  const int32_t* link;       /* [nshape] */
  const double* pos;         /* [nshape][3] shape frame in the link frame */
  const double* rot;         /* [nshape][9] row-major */
  const double* size;        /* [nshape][3] box half extents; hulls: half extents of the bounding box centred at sphere[0..2]; capsules: (r, r, r + half length) */
  const int32_t* plane_adr;  /* [nshape] hulls: first row of `planes` */
  const int32_t* plane_num;  /* [nshape] */
  const double* sphere;      /* [nshape][4] bounding sphere, shape frame: centre, radius (< 0: unbounded) */
  const double* planes;      /* [nplanes][4] n . x <= d */
  double znear, zfar;        /* mjModel.vis.map.znear / zfar times mjModel.stat.extent */
} rcsh_render_scene_desc;
typedef struct rcsh_camera_desc {
  int32_t link, width, height;  /* mjModel.cam_bodyid folded to its link; resolution of SimCameraConfig */
  double pos[3], rot[9];        /* camera frame in the link frame (mjModel.cam_pos / cam_quat) */
  double fovy_deg;              /* mjModel.cam_fovy */
} rcsh_camera_desc;
int rcsh_sim_set_render_scene(rcsh_sim* sim, const rcsh_render_scene_desc* scene);
int rcsh_sim_add_camera(rcsh_sim* sim, const rcsh_camera_desc* cam, int32_t* cam_id);
/* Host only (no device needed): the edges of the convex polytope { x : n_i . x <= d_i } that `planes` ([nplanes][4]) describe --
 * what rcsh_sim_set_render_scene works out for every hull so that the ray caster can find the hull's outline as the camera
 * sees it (a ray hits the hull exactly when it passes inside the outline; its entry depth comes from the planes facing the
 * camera alone).  edge_planes: [capacity][2] the two planes meeting in the edge, edge_verts: [capacity][6] its end points (both may
 * be NULL to ask for the count), centre: [3] a point inside.  *nedges = 0: the planes bound no polytope the routine vouches
 * for (Euler's formula failed on what it found); such a hull is drawn by walking all its planes. */
int rcsh_hull_edges(const double* planes, int32_t nplanes, int32_t capacity, int32_t* edge_planes, double* edge_verts, int32_t* nedges, double* centre);
/* One image per environment.  depth_gl: [N][H][W] f32 in [0, 1], rows bottom-up, what mjr_readPixels returns;
 * depth_mm: [N][H][W] u16, rows top-down, millimetres: DataFrame.data of SimCameraSet(physical_units=True);
 * cam_pose: [N][12] mjData.cam_xmat (9) + cam_xpos (3).  Each may be NULL.  _dev: device pointers, enqueued on the
 * handle's stream. */
int rcsh_camera_render(rcsh_sim* sim, int32_t cam_id, float* depth_gl, uint16_t* depth_mm, double* cam_pose);
int rcsh_camera_render_dev(rcsh_sim* sim, int32_t cam_id, float* depth_gl_dev, uint16_t* depth_mm_dev, double* cam_pose_dev);
/* Colour frames (the ColorFrame of FrameSet, src/sim/camera.cpp:103-118: mjr_readPixels' rgb buffer).  The image is
 * ray-cast like the depth: the colour of the shape a ray enters first (mjModel.geom_rgba / mat_rgba; a material with the
 * builtin checker texture alternates its two colours in squares), flat-shaded on the entry face's normal by the headlight
 * (mjModel.vis.headlight ambient / diffuse) and one directional light of the scene; rays that leave the scene see the
 * skybox gradient.  No textures beyond the checker, no shadows, no specular term, no transparency: not OpenGL's pixels.
 * colour: [nshape][8] = rgb (3), second checker colour (3), edge of a checker square [m], checker flag (0 / 1). */
typedef struct rcsh_render_colours {
  const double* colour;
  double headlight_ambient[3], headlight_diffuse[3];
  double light_dir[3], light_diffuse[3]; /* directional light (world frame, pointing away from the light); diffuse 0: none */
  double sky_rgb1[3], sky_rgb2[3];       /* zenith / nadir colour of the background */
} rcsh_render_colours;
int rcsh_sim_set_render_colours(rcsh_sim* sim, const rcsh_render_colours* colours);
/* rgb: [N][H][W][3] u8, rows bottom-up (as mjr_readPixels returns them); the depth outputs as above; each may be NULL. */
int rcsh_camera_render_rgb(rcsh_sim* sim, int32_t cam_id, uint8_t* rgb, float* depth_gl, uint16_t* depth_mm, double* cam_pose);
/* The ray caster's arithmetic type.  Default (0): float32 -- the reference's depth image is a float32 OpenGL z-buffer read back
 * and quantised to uint16 millimetres (python/rcs/camera/sim.py:57-86), src/sim/camera.cpp:86-140 computes nothing in double.
 * 1: every ray in double -- the instantiation whose pixels equal the tests' numpy restatement bit for bit (about 1.4x the time).
 * (RCSH_RENDER_F64=1 in the environment selects it at rcsh_sim_create.) */
int rcsh_sim_set_render_f64(rcsh_sim* sim, int32_t on);
int rcsh_camera_render_rgb_dev(rcsh_sim* sim, int32_t cam_id, uint8_t* rgb_dev, float* depth_gl_dev, uint16_t* depth_mm_dev, double* cam_pose_dev);
/* Rendering callbacks: SimCameraSet(render_on_demand = false) (src/sim/camera.cpp:23-47,97-102; Sim::register_rendering_callback,
 * invoke_rendering_callbacks, reset_callbacks: src/sim/sim.cpp:63-81,108-115,131-137,160-173).  A camera with a frame rate is due
 * after a substep when more than seconds_between_calls (= 1 / frame_rate) of simulated time passed since its last frame; the
 * clocks start at -seconds_between_calls, and again after Sim::reset, so the first substep renders.  A kernel cannot call the
 * renderer: the substep loop RECORDS per environment what the renderer would have seen at that moment (the kinematic state
 * of the substep's position stage, the new time, which cameras are due), at most `capacity` records per environment and
 * launch, and the host renders them afterwards:
 *   launch (any stepping / env entry point) -> rcsh_render_pending(count[N]) -> for slot < max(count):
 *   rcsh_camera_render_snapshot(cam, slot, ..., timestamp[N], due[N]) for each scheduled camera.
 * Images of environments whose `due` is 0 for that slot and camera are meaningless.  ncam = 0 removes the schedule. */
int rcsh_sim_set_render_schedule(rcsh_sim* sim, const int32_t* cam_ids, const double* seconds_between_calls, int32_t ncam, int32_t capacity);
int rcsh_render_pending(rcsh_sim* sim, int32_t* count);
/* Calling rcsh_sim_set_render_schedule again with the SAME cameras and periods and a larger capacity grows the schedule in
 * place: clocks and pending records stay.  Records beyond the capacity are not written; rcsh_render_pending clamps its counts
 * to the capacity and adds what was lost to a counter that rcsh_render_dropped reads (reset with the schedule). */
int rcsh_render_dropped(rcsh_sim* sim, int64_t* dropped);
int rcsh_camera_render_snapshot(rcsh_sim* sim, int32_t cam_id, int32_t slot, uint8_t* rgb, float* depth_gl, uint16_t* depth_mm, double* cam_pose,
                                double* timestamp, uint8_t* due);

/* ---- multi-GPU: one process (one handle) per GPU, contiguous ranges of environments per rank, no data-path collective
 * except ONE exchange step: the all-gather of the observation tensor [n][obs_width] f64 of every rank into
 * [world * n][obs_width] on every GPU (the reference holds one model / data pair per Sim, src/sim/sim.h:75-77,
 * and has nothing to exchange).  RCCL (librccl.so, loaded on first use) over xGMI; no host framework involved:
 *   rank 0: rcsh_comm_get_unique_id -> ship the 128 bytes to the other ranks by any side channel -> every rank:
 *   rcsh_comm_init(sim, id, rank, world).
 * rcsh_env_allgather_obs_dev is ordered after the work already enqueued on the handle's stream (an event) but runs on
 * the communicator's OWN stream, so the next env-step overlaps it; the caller alternates two send / receive buffer pairs
 * (`slot` 0 / 1) and calls rcsh_comm_wait(slot) before it reads that slot's gathered tensor or overwrites its send buffer. */
#define RCSH_COMM_ID_BYTES 128
int rcsh_comm_get_unique_id(uint8_t id[RCSH_COMM_ID_BYTES]);
int rcsh_comm_init(rcsh_sim* sim, const uint8_t id[RCSH_COMM_ID_BYTES], int32_t rank, int32_t world);
int rcsh_comm_rank(const rcsh_sim* sim, int32_t* rank, int32_t* world);
int rcsh_env_allgather_obs_dev(rcsh_sim* sim, int32_t slot, const double* local_obs_dev, double* all_obs_dev);
int rcsh_comm_allgather_dev(rcsh_sim* sim, int32_t slot, const void* send_dev, void* recv_dev, size_t bytes_per_rank);
int rcsh_comm_wait(rcsh_sim* sim, int32_t slot, int32_t block_host); /* 0: the handle's stream waits for the slot's gather; 1: the host does */
int rcsh_comm_destroy(rcsh_sim* sim);
/* The same exchange over COPY ENGINES instead of RCCL's collective kernel (which needs 261-280 registers a lane and finds no SIMD free
 * beside a full batch's stepping wavefronts: its gather then starts when the env-step ends).  Every rank writes its block into the
 * receive buffer of every peer with asynchronous copies (SDMA over xGMI, one stream per peer), followed by an 8-byte sequence number
 * into a flag word of the peer; one 64-lane wavefront per gather waits for the flag words.  Set-up:
 *   every rank: rcsh_comm_copy_create(sim, rank, world, bytes_per_rank, blob)  -- allocates the two receive buffers and the flags,
 *   exports them; all-gather the blobs over any side channel; every rank: rcsh_comm_copy_connect(sim, blobs[world]).
 * Then rcsh_comm_allgather_dev / rcsh_env_allgather_obs_dev / rcsh_comm_wait / rcsh_comm_destroy as with RCCL, with ONE difference:
 * the receive buffer of a slot is the carrier's (rcsh_comm_copy_recv_buffer), since peers have to have it mapped.  World <= 16,
 * one rank per process. */
#define RCSH_COMM_COPY_BLOB_BYTES 256
int rcsh_comm_copy_create(rcsh_sim* sim, int32_t rank, int32_t world, size_t bytes_per_rank, uint8_t blob[RCSH_COMM_COPY_BLOB_BYTES]);
int rcsh_comm_copy_connect(rcsh_sim* sim, const uint8_t* blobs /* [world][RCSH_COMM_COPY_BLOB_BYTES], by rank */);
int rcsh_comm_copy_recv_buffer(rcsh_sim* sim, int32_t slot, void** recv_dev);

/* device allocation helpers so a host language without a HIP binding can keep rollouts resident */
int rcsh_dev_alloc(rcsh_sim* sim, size_t bytes, void** ptr);
int rcsh_dev_free(rcsh_sim* sim, void* ptr);
int rcsh_dev_upload(rcsh_sim* sim, void* dst_dev, const void* src_host, size_t bytes);
int rcsh_dev_download(rcsh_sim* sim, void* dst_host, const void* src_dev, size_t bytes);

/* development hook: copies the finalised device model tables (csrc/model.h DevModel) to `buf`; used by
 * tools/kbench to replay the exact FR3 tables in kernel micro-benchmarks */
int rcsh_debug_dump_model(rcsh_sim* sim, void* buf, size_t cap, size_t* size);

/* kernel timing hooks for bench.py: HIP events on the handle's stream around every `enable`-th fused env-step launch
 * (1: every launch; 0: off).  A pair of event records around EVERY launch costs ~8 us of dispatch gap per step.
 * enable < 0: REGION mode -- one event before the first stepping launch after this call, one when rcsh_prof_read is called;
 * read returns the stream time between them and the number of stepping launches it covers (the launches' durations plus the
 * dispatch gaps between them: an upper bound of the kernel's average duration, no event traffic inside the region). */
int rcsh_prof_enable(rcsh_sim* sim, int32_t enable);
int rcsh_prof_read(rcsh_sim* sim, double* total_ms, int64_t* launches);

/* ---- autoreset: finished episodes are reset on the device inside the fused env step (Gymnasium's VectorEnv autoreset, SAME_STEP
 * mode), so that a resident rollout never returns to the host because episodes end.  When enabled, rcsh_env_step_dev,
 * rcsh_env_step_task_dev and their host forms enqueue, behind the stepping launch (and behind a truncating guard's mark), one launch
 * that decides per environment (csrc/episode_team.h: k_episode_end)
 *   time_limit = max_episode_steps > 0 && elapsed >= max_episode_steps   (Gymnasium's TimeLimit; elapsed counts this step)
 *   terminated = the pick task is configured && the step's success        (task row, element 8)
 *   truncated  = info row byte 4 || time_limit,    done = terminated || truncated
 * writes time_limit into byte 4 of the caller's info row, adds the step's reward (task row, element 7; 0 without the pick task) to the
 * environment's running return in fp64, and for a done environment copies the step's observation, info row, gripper width and task
 * row into the record's final_*, writes the finished episode's return and length, zeroes both counters and counts the episode.  Then
 * the masked reset launch -- rcsh_env_reset_dev's, or with draw_box rcsh_env_reset_task_dev's with the poses drawn below -- runs with
 * `done` as its mask: it writes the new episode's first observation and gripper width into the rows of the done environments in the
 * CALLER's obs / gripper_width buffers, and its info rows into the record's reset_info.  The caller's info, substeps and task rows
 * are still the terminal step's after the call (a loop that reads info[:, 4] or task[:, 7:9] gets the terminal reward).  The reset
 * launch is enqueued whether or not anyone is done -- the host does not know --; a workgroup whose environments all sit out leaves
 * after its prologue.  A null obs / info / gripper_width (/ task, with the pick task) pointer of a _dev step stands for the library's
 * own staging slice.
 * Cube placement (draw_box) is counter-based -- an environment's draws depend neither on the batch size, nor on which other
 * environments finish, nor on how the batch is sharded --: Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter
 * (env_offset + e, k & 0xffffffff, k >> 32, j) with k the autoresets environment e has had before this one; j = 0 gives u0 (words
 * 0, 1) and u1 (words 2, 3), j = 1 gives u2 (words 0, 1); a uniform in [0, 1) from words (a, b) is ((a << 32 | b) >> 11) * 2^-53.
 * With p = box_pose (x y z qw qx qy qz): x = include_position ? (p[0] + u0 * 0.2) - 0.1 : p[0], y likewise from u1, z = p[2],
 * qw = include_rotation ? 2 * u2 - rotation_minus : p[3], qx qy qz = p[4..6], every operation rounded on its own.  RandomCubePos:
 * p = (iso_x, iso_y, 0.0144, 0, 0, 0, 1), rotation_minus = 1; RandomObjectPos: p = the initial pose, rotation_minus = its w.
 * With autoreset configured, rcsh_env_reset* (masked or not) also zeroes elapsed and running_return of the environments it resets
 * (episodes stays); rcsh_env_configure_autoreset zeroes every counter.  The counters are NOT part of rcsh_sim_get_state /
 * rcsh_sim_set_state: the blob's size and layout are what they were (as with the rate-driven cameras' clocks, a restored handle
 * keeps the counters it has).
 * RCSH_ERR_ARG: null description, negative max_episode_steps or env_offset, env_offset + N > 2^32, a non-finite pose (checked before
 * the handle is looked at); RCSH_ERR_STATE: before rcsh_env_configure, draw_box without rcsh_env_configure_pick_task, while a render
 * schedule is set (rate-driven cameras under autoreset are not built; rcsh_sim_set_render_schedule in turn refuses while autoreset
 * is enabled), and for the record before any step under autoreset.  A refused call changes nothing. */
typedef struct rcsh_autoreset_desc {
  int32_t enabled;            /* 0: steps run as before (the configuration and the counters are kept) */
  int32_t max_episode_steps;  /* 0: no time limit */
  int32_t draw_box;           /* 1: a done environment's free body is placed by the rule above (needs rcsh_env_configure_pick_task) */
  int32_t include_position, include_rotation;
  int64_t env_offset;         /* this handle's first environment in a sharded batch */
  uint64_t seed;
  double box_pose[7];
  double rotation_minus;
} rcsh_autoreset_desc;
int rcsh_env_configure_autoreset(rcsh_sim* sim, const rcsh_autoreset_desc* autoreset);
/* The record of the most recent step under autoreset: device pointers, valid for the handle's life, rewritten by every such step. */
typedef struct rcsh_autoreset_record {
  const uint8_t *done, *terminated, *truncated, *time_limit;          /* [N] */
  const double* final_obs; const uint8_t* final_info; const double *final_gripper_width, *final_task; /* rows of done environments (others: stale) */
  const double* episode_return; const int32_t* episode_length;        /* of the episode that just ended, where done */
  const int64_t* episodes; const int32_t* elapsed; const double* running_return;
  const uint8_t* reset_info; const double* reset_box_qpos;            /* [N][8], [N][7]: rows of done environments */
} rcsh_autoreset_record;
int rcsh_env_autoreset_record_dev(rcsh_sim* sim, rcsh_autoreset_record* out);
/* The same record copied to host arrays, any of which may be NULL (after rcsh_env_step / rcsh_env_step_task the verdict bytes, the
 * returns and the lengths come from the copy that step fetched with its own outputs: no further wait). */
int rcsh_env_autoreset_last(rcsh_sim* sim, uint8_t* done, uint8_t* terminated, uint8_t* truncated, uint8_t* time_limit, double* final_obs,
                            uint8_t* final_info, double* final_gripper_width, double* final_task, double* episode_return,
                            int32_t* episode_length, int64_t* episodes, int32_t* elapsed, double* running_return, uint8_t* reset_info,
                            double* reset_box_qpos);
/* Host only (no handle, no device): the pose the device draws for environment `env` of a handle with this description at its
 * autoreset number `episode`.  RCSH_ERR_ARG for a description rcsh_env_configure_autoreset would refuse on its own, a negative env or
 * episode, env_offset + env >= 2^32, a null output. */
int rcsh_autoreset_draw(const rcsh_autoreset_desc* autoreset, int64_t env, int64_t episode, double qpos7[7]);

#ifdef __cplusplus
}
#endif
#endif /* RCS_HIP_H */
