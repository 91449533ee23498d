// rcs_hip.hip -- C-ABI (include/rcs_hip.h) over the batched kernels.  gfx950 only.
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rcs_hip.h"
#include "model_host.h"
#include "owned.h"
#include "host_stage.h"
#include "sim_kernels.h"
#include "verify_team.h"
#include "render.h"
#include "query_team.h"
#include "clearance_team.h"
#include "swept_team.h"
#include "dynamics_team.h"
#include "dynamics_grad_team.h"
#include "opspace_team.h"
#include "torque_team.h"
#include "env_torque_team.h"
#include "guard_team.h"
#include "episode_team.h"

using namespace rcsh;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess)                                                                          \
      return fail(RCSH_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e));             \
  } while (0)

constexpr int kBlock = 64;     // accessor kernels
constexpr int kProfRing = 4096;

}  // namespace
int rcsh::episode_fail(int code, const char* msg) { return fail(code, msg); }  // (csrc/episode_host.cpp reports through rcsh_last_error)

struct CopyCarrier;
namespace {
void copy_carrier_free(CopyCarrier* c);
void rccl_comm_destroy(void* comm);
}  // namespace
// a buffer that grows on demand (grow_device / grow_pinned)
template <auto Release> struct Grown { Owned<void*, Release> p; size_t cap = 0; };
using GrownDev = Grown<hipFree>;
using GrownPin = Grown<hipHostFree>;
// Device staging of the host-pointer entry points: one allocation, cut by stage_layout -- and nowhere else -- into typed slices that
// do not overlap; each starts on a 256-byte boundary.  A slice with two names carries two contents that no single entry point uses together.
struct Staging {
  DevBuf<void> base;             // the slices below are views into it
  int action_w = 0, obs_w = 0, q0_w = 0;  // doubles per environment of `action`, `obs` and `q0`
  uint8_t* mask = nullptr;       // [n]: the caller's mask
  uint8_t* inv_mask = nullptr;   // [n]: its complement (observe_unmasked)
  uint8_t* info = nullptr;       // [n][kInfoBytes]: the env layer's info rows
  uint8_t* flag = nullptr;       // [n]: one flag bit as bytes (flag_host) | the IK's success (run_ik)
  int32_t* substeps = nullptr;   // [n]: the env-step's substeps | the IK's iterations (run_ik)
  float* grip_cmd = nullptr;     // [n]: the env-step's gripper command
  double* grip_width = nullptr;  // [n]: gripper widths out
  double* action = nullptr;      // [n][action_w]: the env-step's action
  double* box_task = nullptr;    // [n][kTaskWidth]: the box pose in (7 wide, rcsh_env_reset_task) | the task rows out (rcsh_env_step_task)
  double* obs = nullptr;         // [n][obs_w]: observations | the IK's output (nl or 7 wide, run_ik)
  double* wide = nullptr;        // [n][kStageWidth]: a field group on its way into or out of the state (scatter_host / gather_host)
  double* pose = nullptr;        // [n][7]: target poses (run_ik, rcsh_robot_set_cartesian_position)
  double* q0 = nullptr;          // [n][q0_w]: the IK's start configurations
  double* tcp = nullptr;         // [7]: the IK's tcp offset
};
// Page-locked staging of the env layer's host forms, between the caller's arrays and the device slices (offsets in bytes):
// [action | gripper | box pose | obs | info | gripper width | substeps | task]
struct PinLayout { size_t action, gripper, box, obs, info, gw, sub, task, total; };
constexpr size_t kEscRows = 4;  // rows of the escalation masks (RunOp::esc)
// Who owns what: every buffer, stream and event the handle creates lives in an owner (owned.h) below and goes when the handle is
// deleted -- members in reverse order, so own_stream, declared before every buffer, goes last.  An entry point that replaces or first
// creates a GROUP of resources builds it in local owners and moves it in after the last step that can fail: on failure the handle
// is what it was before the call.  Device-visible structs (Params, RunOp, RendCfg, RenderScene, ...) are filled from get().
struct rcsh_sim {
  int device = 0;
  int kernel = RCSH_KERNEL_AUTO;
  int n_simd = 1024;  // SIMDs of the device (4 per compute unit)
  hipStream_t stream = nullptr;  // view: own_stream, or the caller's (rcsh_sim_set_stream)
  Stream own_stream;
  int n = 0;
  HostModel hm;
  DevModel dm;
  DevBuf<DevModel> d_model;        // DevModel followed by LinkRec[kMaxLinks]
  std::vector<LinkRec> links;
  CollisionPoints cp;
  std::vector<uint8_t> cp_class;
  DevBuf<double> d_coll_xyzr;
  DevBuf<uint8_t> d_coll_cls;
  // contact phase (contact_team.h): the robot's collision geoms and their hull vertices
  std::vector<ContactGeom> cgeoms;
  std::string contact_overflow;  // why collision geoms were left out of `cgeoms` (capacity); empty: none were
  std::vector<int> cgeoms_dropped;  // mjModel ids of those geoms: invisible to geom-geom detection (the floor test by sample points still sees them)
  std::vector<double> cverts;
  DevBuf<ContactGeom> d_cgeoms;
  DevBuf<double> d_cverts;
  // what the collision tests may skip (model.cpp: build_collision_tables; rebuilt when the class bits change) and its device copies: the
  // self-collision pairs a collision callback reacts to; the once-per-launch check for contacts nobody resolves (check_team.h)
  CollisionTables tables;
  GrownDev d_pairs, d_chk_ent, d_chk_geoms;  // SelfPair[], CheckEntry[], CheckGeom[]
  DevBuf<float> d_lev;               // tables.link_lever
  DevBuf<float> d_slack;             // [n][kSlackStride]: the self-contact stage's remaining gaps per pair + the joints it saw last (CheckTable::slack)
  GrownDev d_query;                  // staging of every host-pointer query form (staged_call): point, motion, clearance, swept clearance, dynamics, and the peek's action
  // the environments' collision guard (guard_team.h; rcsh_env_configure_guard): its settings, and two records of [result | t_contact |
  // blocked | hold] -- the last guarded step's (rcsh_env_guard_last) and the scratch of rcsh_env_guard_peek.  d_guard and h_guard are
  // one group, present or absent together; so are d_episode and h_episode below.
  struct GuardCfg { bool configured = false, enabled = false, block_undecided = true, truncate = true; int kinds = 0; double resolution = 0; } guard;
  DevBuf<void> d_guard;
  bool guard_stepped = false;        // a guarded step has filled the first record
  PinBuf<char> h_guard;              // page-locked copy of that record: rcsh_env_step fetches it with its own outputs (one synchronisation)
  bool guard_host_valid = false;     // ... and it is the last guarded step's
  // autoreset (episode_team.h; rcsh_env_configure_autoreset): the description, the record every step under autoreset rewrites
  // (EpisodeLayout), and a page-locked copy of the record's front (verdict bytes, returns, lengths) that the host forms of env.step
  // fetch with their own outputs
  struct AutoresetCfg { bool configured = false, enabled = false; rcsh_autoreset_desc desc{}; } autoreset;
  DevBuf<void> d_episode;
  PinBuf<char> h_episode;
  bool episode_stepped = false;      // a step under autoreset has filled the record
  bool episode_host_valid = false;   // ... and h_episode is that step's
  // per-environment escalation (sim_kernels.h: RunOp::esc_role): a step is the lean launch over the environments not in contact plus
  // the contact-resolving launch over the others
  bool esc_mode = false;
  struct EscBufs {                 // one group, present or absent together (rcsh_sim_set_contact_options)
    DevBuf<uint64_t> mask;         // [kEscRows][(n + 63) / 64]: escalated, newly flagged, leaving, touching (RunOp::esc)
    DevBuf<uint32_t> ctr;          // [4] (sim_kernels.h: RunOp::esc_ctr)
    DevBuf<double> snap;           // [nfields][n]: what the lean launch of a step read (the step is redone from it on a hit)
    DevBuf<uint32_t> snap_flags;
    DevBuf<int32_t> snap_conv;
    DevBuf<double> trace;          // [kEscTraceCap][nl][n]: where the lean launch's substeps began (RunOp::trace)
  } esc;
  int conv_chunk = 48;              // step_until_convergence in pieces of this many substeps when contacts are resolved per environment (launch_run; RCSH_CONV_CHUNK)
  bool contact_check = true;  // RCSH_CONTACT_CHECK=0 switches the check off (measurements of its cost)
  int check_every = 1;        // the check ends every check_every-th stepping launch (rcsh_sim_set_contact_check); 0: never
  int64_t check_seq = 0;
  double plane_mu = 1.0;
  std::vector<int> act_slot;
  int narm = 0, nl = 0, nu = 0;
  bool grip = false;
  int nfields = 0;
  DevBuf<double> S;
  DevBuf<uint32_t> flags;
  DevBuf<int32_t> conv;
  SimCfg sim{0, 0, 30, 500};
  RobotCfg robot{};
  GripperCfg gripcfg{};
  EnvCfg env{};
  BoxCfg box{};
  TaskCfg task{};
  bool env_configured = false;
  // torque control (torque_team.h): whether every arm actuator is a plain torque source (settled by rcsh_sim_add_robot), the law as last
  // configured, and -- one group, allocated at the first use -- the law's targets and the environments' sticky `singular` bytes
  struct Torque {
    bool actuated = false;
    rcsh_torque_law law{};
    DevBuf<double> target;     // [kTorquePose + narm][n]
    DevBuf<uint8_t> singular;  // [n]
  } tq;
  DevBuf<BoxTaskCfg> d_boxtask;
  // depth renderer (render.h)
  RenderScene rscene{};              // its pointers are views into rbuf (rcsh_sim_set_render_scene, rcsh_sim_set_render_colours)
  struct RenderBufs {                // one group: a scene's buffers are replaced together
    DevBuf<RenderShape> shapes;
    DevBuf<double> planes;
    DevBuf<RenderColour> colours;
    DevBuf<int32_t> edge_planes;     // the outline method of the ray caster (render.h: k_hull_views)
    DevBuf<double> edge_verts, views;
    DevBuf<double> frames;           // present: a render scene is attached
    DevBuf<double> wframes;          // world frames of the shapes + camera per environment (k_shape_frames)
  } rbuf;
  RendCfg rend{};                    // rate-driven cameras (rcsh_sim_set_render_schedule); its pointers are views into the three owners
  DevBuf<double> rend_last, rend_snap;
  DevBuf<int32_t> rend_count;
  int rend_cam_id[kMaxRateCams] = {0, 0, 0, 0};
  int64_t rend_dropped = 0;          // records that did not fit the schedule's capacity (rcsh_render_pending counts them)
  const double* frames_src = nullptr; // view into rend_snap, set while a record of the render schedule is being rendered
  const double* frames_src_base(int slot) const { return rend.snap + (size_t)slot * (size_t)(nl + 9) * (size_t)n; }
  bool render_f64 = false;      // the ray caster's arithmetic type (rcsh_sim_set_render_f64; RCSH_RENDER_F64=1 at creation)
  std::vector<RenderCam> cams;
  GrownDev d_image;  // staging of the host-pointer render call (staged_call)
  double* pending_task = nullptr;  // view into the caller's memory or the staging: task output of the env-step being enqueued (rcsh_env_step_task*)
  // staging for the host-pointer entry points: the device side, fixed at creation (stage_create), and page-locked memory between it and
  // the caller's arrays for the env layer's host forms (PinLayout; a copy to or from pageable memory is staged by the runtime and waited
  // for, one array at a time: 0.19 of rcsh_env_step's 0.32 ms)
  Staging stage;
  PinLayout pin{};
  GrownPin h_pin;
  // multi-GPU exchange: built in a local by rcsh_comm_init / rcsh_comm_copy_create and attached whole; rcsh_comm_destroy is its one
  // teardown.  Destroyed in reverse: the carrier or the communicator, the events, the stream.
  struct Comm {
    Stream stream;
    Event ready, done[2];
    Owned<void*, rccl_comm_destroy> nccl;          // ncclComm_t (RCCL, loaded on first use)
    Owned<CopyCarrier*, copy_carrier_free> copy;   // the all-gather's second carrier: copy engines + flags in peer memory (rcsh_comm_copy_*)
    bool pending[2] = {false, false};
    int rank = 0, world = 1;
  } comm;
  // profiling
  Event order_ev;                      // rcsh_sim_wait_for: marks this handle's stream for another handle's stream to wait on
  bool prof = false;
  bool prof_region = false;            // one event pair around the whole timed region instead of sampled launches
  int64_t prof_region_launches = 0;
  std::vector<Event> ev_start, ev_stop;
  int prof_pending = 0;
  int prof_every = 1;       // HIP events around every prof_every-th stepping launch
  int64_t prof_seen = 0;
  double prof_ms = 0;
  int64_t prof_launches = 0;
};

namespace {

int grid_for(int n) { return (n + kBlock - 1) / kBlock; }

// The launch-invariant blocks come prebuilt (CollisionTables); a launch adds the pointers and what its configuration decides.
Params make_params(rcsh_sim* s) {
  const CollisionTables& t = s->tables;
  Params P;
  P.model = s->d_model.get();
  std::memcpy(&P.coll, &t.coll, sizeof(P.coll));
  P.coll.xyzr = s->d_coll_xyzr.get();
  P.coll.cls = s->d_coll_cls.get();
  P.S = s->S.get();
  P.flags = s->flags.get();
  P.conv_steps = s->conv.get();
  P.n = s->n;
  P.keep_qpre = bool(s->rbuf.frames);
  P.sim = s->sim;
  P.robot = s->robot;
  P.grip = s->gripcfg;
  P.env = s->env;
  P.boxtask = s->d_boxtask.get();
  P.rend = s->rend;
  std::memcpy(&P.ctab, &t.ctab, sizeof(P.ctab));
  P.ctab.geoms = s->d_cgeoms.get();
  P.ctab.verts = s->d_cverts.get();
  P.ctab.pairs = static_cast<const SelfPair*>(s->d_pairs.p.get());
  P.ctab.ngeom = s->box.resolve ? (int)s->cgeoms.size() : 0;
  P.ctab.plane_mu = s->plane_mu;
  std::memcpy(&P.chk, &t.chk, sizeof(P.chk));
  P.chk.ent = static_cast<const CheckEntry*>(s->d_chk_ent.p.get());
  P.chk.lev = s->d_lev.get();
  P.chk.geoms = static_cast<const CheckGeom*>(s->d_chk_geoms.p.get());
  P.chk.slack = s->d_slack.get();
  if (const char* dm = std::getenv("RCSH_CHECK_SKIP")) P.chk.pad = std::atoi(dm);  // development: bit 0 no narrow phase, 1 no boxes, 2 no spheres, 3 no
  // Gilbert fallback, 4 no slack record (timing experiments, check_team.h); bit 5 sends every coupled environment of a box-less scene to the
  // wide solve (contact_wide.h) whatever its contact count, not only those with more than kDenseCon contacts (contact_dense.h; the tests
  // of the wide solve's math on few contacts, tests/test_gpu_contact_wide.py); bit 6 takes the pairs-only shortcut out of the contact phase's
  // collision pass (contact_team.h: contact_collide; tests/test_gpu_quiet_escalated.py compares the two forms); bit 7 keeps every hull round of
  // that pass on teams of 16 lanes, where a lone pair takes the wavefront and two pairs half of it each (tests/test_gpu_wide_support.py
  // compares the two forms), bit 8 only the rounds of two pairs (a timing experiment).  Read on every launch.
  return P;
}

int upload_boxtask(rcsh_sim* s) {
  BoxTaskCfg bt{s->box, s->task};
  if (!s->d_boxtask) HIP_TRY(hipMalloc(s->d_boxtask.out(), sizeof(BoxTaskCfg)));
  HIP_TRY(hipMemcpyAsync(s->d_boxtask.get(), &bt, sizeof(bt), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return RCSH_OK;
}

int upload_model(rcsh_sim* s) {
  HIP_TRY(hipMemcpyAsync(s->d_model.get(), &s->dm, sizeof(DevModel), hipMemcpyHostToDevice, s->stream));
  // the team kernels' per-link records live right behind the DevModel
  s->links.resize(kMaxLinks);
  fill_link_records(s->dm, s->links.data());
  HIP_TRY(hipMemcpyAsync(reinterpret_cast<char*>(s->d_model.get()) + sizeof(DevModel), s->links.data(), sizeof(LinkRec) * kMaxLinks,
                         hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return RCSH_OK;
}

// class bits of the contact sample points: bit 0 arm collision geoms, bit 1 gripper collision geoms
int upload_coll_classes(rcsh_sim* s) {
  if (s->cp.geom.empty()) return RCSH_OK;
  HIP_TRY(hipMemcpyAsync(s->d_coll_cls.get(), s->cp_class.data(), s->cp_class.size(), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return RCSH_OK;
}

static_assert(kSelfStageVertsHost == kSelfStageVerts, "the pair filter's vertex cap is the self-contact stage's LDS room (contact_team.h)");

// one buffer, grown on demand: the stream may still be reading or writing the old one
template <class G, class Alloc>
int grow(rcsh_sim* s, G& g, size_t bytes, Alloc alloc) {
  if (bytes <= g.cap) return RCSH_OK;
  if (g.p) HIP_TRY(hipStreamSynchronize(s->stream));
  g.cap = 0;
  HIP_TRY(alloc(g.p.out(), bytes));
  g.cap = bytes;
  return RCSH_OK;
}
int grow_device(rcsh_sim* s, GrownDev& g, size_t bytes) { return grow(s, g, bytes, [](void** p, size_t b) { return hipMalloc(p, b); }); }
int grow_pinned(rcsh_sim* s, GrownPin& g, size_t bytes) { return grow(s, g, bytes, [](void** p, size_t b) { return hipHostMalloc(p, b, hipHostMallocDefault); }); }

// One host-pointer call over a grown device buffer, laid out by a StageLayout (host_stage.h): declare once, view after grow, one wait.
// Grows `g` to the layout's total, enqueues the uploads of the present inputs, runs `body` -- the launches --, enqueues the downloads
// of the outputs asked for and waits for the stream: the call's one wait.  Device views exist only as `dev(ticket)` of the function
// that `body` is handed, so none can be taken before the grow, which may free and reallocate.
template <class Body>
int staged_call(rcsh_sim* s, GrownDev& g, const StageLayout& L, Body body) {
  if (int rc = grow_device(s, g, L.total)) return rc;
  char* const base = static_cast<char*>(g.p.get());
  for (int i = 0; i < L.count; ++i)
    if (const auto& e = L.slice[i]; e.src) HIP_TRY(hipMemcpyAsync(base + e.at, e.src, e.bytes, hipMemcpyHostToDevice, s->stream));
  if (int rc = body([&](auto ticket) { return L.view(base, ticket); })) return rc;
  for (int i = 0; i < L.count; ++i)
    if (const auto& e = L.slice[i]; e.dst) HIP_TRY(hipMemcpyAsync(e.dst, e.from ? e.from : base + e.at, e.bytes, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return RCSH_OK;
}

// a host table's device copy; the buffer grows on demand (grow_device waits for the stream before it frees one a launch may still read)
int upload(rcsh_sim* s, GrownDev& g, const void* src, size_t bytes) {
  if (int rc = grow_device(s, g, bytes)) return rc;
  if (bytes) HIP_TRY(hipMemcpyAsync(g.p.get(), src, bytes, hipMemcpyHostToDevice, s->stream));
  return RCSH_OK;
}

int upload_contact_table(rcsh_sim* s) {
  CollisionTables& t = s->tables;
  build_collision_tables(s->hm, s->dm, s->cp, s->cgeoms, s->cverts, t);
  if (std::getenv("RCSH_DEBUG_NO_SELF_PAIRS")) { t.pairs.clear(); t.ctab.npair = 0; }  // development switch: what the pair tests cost
  if (s->cgeoms.empty()) return RCSH_OK;
  int rc = upload(s, s->d_pairs, t.pairs.data(), sizeof(SelfPair) * t.pairs.size());
  if (!rc) rc = upload(s, s->d_chk_ent, t.chk_ent.data(), sizeof(CheckEntry) * t.chk_ent.size());
  if (!rc) rc = upload(s, s->d_chk_geoms, t.chk_geoms.data(), sizeof(CheckGeom) * t.chk_geoms.size());
  if (rc) return rc;
  if (!s->d_lev) HIP_TRY(hipMalloc(s->d_lev.out(), sizeof(t.link_lever)));
  HIP_TRY(hipMemcpyAsync(s->d_lev.get(), t.link_lever, sizeof(t.link_lever), hipMemcpyHostToDevice, s->stream));
  if (!s->d_cgeoms) HIP_TRY(hipMalloc(s->d_cgeoms.out(), sizeof(ContactGeom) * s->cgeoms.size()));
  HIP_TRY(hipMemcpyAsync(s->d_cgeoms.get(), s->cgeoms.data(), sizeof(ContactGeom) * s->cgeoms.size(), hipMemcpyHostToDevice, s->stream));
  if (!s->d_cverts && !s->cverts.empty()) {
    HIP_TRY(hipMalloc(s->d_cverts.out(), sizeof(double) * s->cverts.size()));
    HIP_TRY(hipMemcpyAsync(s->d_cverts.get(), s->cverts.data(), sizeof(double) * s->cverts.size(), hipMemcpyHostToDevice, s->stream));
  }
  HIP_TRY(hipStreamSynchronize(s->stream));
  return RCSH_OK;
}

int prof_flush(rcsh_sim* s) {
  for (int i = 0; i < s->prof_pending; ++i) {
    float ms = 0;
    HIP_TRY(hipEventSynchronize(s->ev_stop[i].get()));
    HIP_TRY(hipEventElapsedTime(&ms, s->ev_start[i].get(), s->ev_stop[i].get()));
    s->prof_ms += ms;
  }
  s->prof_launches += s->prof_pending;
  s->prof_pending = 0;
  return RCSH_OK;
}

// Which compilation of the team kernel a launch without free box / contacts / detection takes.  Measured (profiles/r3_occ2):
// a second resident wavefront per SIMD is worth 1.4-1.6x once the batch brings more than one wavefront per SIMD -- for a build
// that fits 256 registers by itself (the 6-dof arms: 67.6 M env-steps/s at 8192 environments against 49.0 M at 4096) or spills
// a few values (SO101: 200 bytes of scratch, 1.21-1.31x); a build squeezed into 256 registers at the price of hundreds of
// scratch accesses per substep loses (FR3 + hand: 488 bytes, 0.70x; xArm7: 888 bytes, 0.9x).  Hence AUTO: the <= 256-register
// build when the batch has more wavefronts than the device has SIMDs AND that build's private segment is at most 256 bytes.
// RCSH_OCC2=0/1 in the environment overrides the rule (measurements).
template <class T, bool F>
bool occ2_build_pays() {
  static const bool pays = [] {
    hipFuncAttributes a{};
    if (hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_run_team_occ2<T, F, false, false, false>)) != hipSuccess) return false;
    return a.localSizeBytes <= 256;
  }();
  return pays;
}
template <class T, bool F>
bool use_occ2(const rcsh_sim* s) {
  if (s->kernel == RCSH_KERNEL_TEAM_OCC2) return true;
  if (s->kernel == RCSH_KERNEL_TEAM) return false;
  static const int forced = [] { const char* e = std::getenv("RCSH_OCC2"); return e ? std::atoi(e) : -1; }();
  if (forced >= 0) return forced != 0;
  return (s->n + 3) / 4 > s->n_simd && occ2_build_pays<T, F>();
}

int launch_run_once(rcsh_sim* s, const RunOp& op_in, bool timed);

// step_until_convergence with the robot's contacts resolved environment by environment runs in PIECES of conv_chunk substeps (RunOp::
// conv_chunk; RCSH_CONV_CHUNK, 0: one launch as before): a pair of launches per piece, each lean launch with its own copy of the state and
// its own certificate over the piece's travel alone.  Every piece is enqueued -- the host does not know who has converged --: a
// workgroup whose environments all have leaves after its prologue.
int launch_run(rcsh_sim* s, const RunOp& op_in, bool timed) {
  const int cap = s->sim.max_convergence_steps;
  const bool esc = s->esc_mode && s->box.resolve && !s->box.present && !op_in.observe_only;
  if (op_in.nsteps < 0 && !op_in.do_reset && esc && s->conv_chunk > 0 && cap > s->conv_chunk) {
    for (int done = 0; done < cap; done += s->conv_chunk) {
      RunOp op = op_in;
      op.conv_chunk = s->conv_chunk;
      if (done > 0) { op.conv_resume = 1; op.apply_action = 0; }
      if (int rc = launch_run_once(s, op, timed)) return rc;
    }
    return RCSH_OK;
  }
  return launch_run_once(s, op_in, timed);
}

int launch_run_once(rcsh_sim* s, const RunOp& op_in, bool timed) {
  Params P = make_params(s);
  RunOp op = op_in;
  // the end-of-launch check for contacts nobody resolves: stepping launches at the handle's cadence; a caller may ask for it itself
  if (!op.check && (op.nsteps != 0 || op.do_reset) && s->contact_check && s->check_every > 0) op.check = (s->check_seq++ % s->check_every) == 0;
  if (!s->contact_check) op.check = 0;
  hipError_t err = hipSuccess;
  if (timed && s->prof_region) {
    // region mode: one event before the first timed launch, one after the last (rcsh_prof_read): no event traffic in between
    if (s->prof_region_launches == 0) HIP_TRY(hipEventRecord(s->ev_start[0].get(), s->stream));
    s->prof_region_launches++;
  }
  const bool sample = timed && s->prof && !s->prof_region && (s->prof_seen++ % s->prof_every) == 0;
  if (sample) {
    if (s->prof_pending == kProfRing) {
      int rc = prof_flush(s);
      if (rc) return rc;
    }
    HIP_TRY(hipEventRecord(s->ev_start[s->prof_pending].get(), s->stream));
  }
  // k_run_team: 16 lanes per environment, 4 environments per wavefront.  4096 environments are 1024 wavefronts = one per
  // SIMD of the chip.  (A one-lane-per-environment kernel existed through round 1; it lost at every batch size and could
  // step neither dry friction nor free bodies, and was removed: csrc/dyn.h keeps its formulas for the host-side model
  // finalisation and the shared math.)
  // DET: launches that run the collision callbacks (step_until_convergence) of a model with collision geoms carry the
  // contact detection of the position stage; Sim::step(k) never looks at the flags (sim.cpp:108-115)
  const bool det = op.nsteps < 0 && (P.coll.has_plane || !s->tables.pairs.empty());
  // per-environment escalation: stepping launches of a box-less scene whose robot contacts are resolved environment by environment
  const bool esc = s->esc_mode && s->box.resolve && !s->box.present && (op.nsteps != 0 || op.do_reset) && !op.observe_only;
  if (esc) {
    op.esc = s->esc.mask.get(); op.esc_ctr = s->esc.ctr.get();
    op.snap = s->esc.snap.get(); op.snap_flags = s->esc.snap_flags.get(); op.snap_conv = s->esc.snap_conv.get();
  }
  bool launched = false;
  bool ok = dispatch_topology(s->narm, s->grip, [&](auto topo) {
    using T = decltype(topo);
    const dim3 grid(((s->n + 31) / 32) * 8), block(64);
    auto go = [&](auto fric, auto box, auto con) {
      constexpr bool F = decltype(fric)::value, B = decltype(box)::value, C = decltype(con)::value;
      if (det) hipLaunchKernelGGL((k_run_team<T, F, B, C, true>), grid, block, 0, s->stream, P, op);
      else if constexpr (!B && !C) {
        if (use_occ2<T, F>(s)) hipLaunchKernelGGL((k_run_team_occ2<T, F, false, false, false>), grid, block, 0, s->stream, P, op);
        else hipLaunchKernelGGL((k_run_team<T, F, false, false, false>), grid, block, 0, s->stream, P, op);
      } else hipLaunchKernelGGL((k_run_team<T, F, B, C, false>), grid, block, 0, s->stream, P, op);
      launched = true;
    };
    using Y = std::true_type;
    using N = std::false_type;
#ifdef RCSH_DEV_NO_CONTACT_KERNELS  // development builds: the lean instantiations alone
    if (s->dm.has_friction) go(Y{}, N{}, N{});
    else go(N{}, N{}, N{});
#else
    if (s->box.present && s->box.resolve) {
      // free box + contacts of the robot's geoms (FR3 + hand; xArm7 + gripper: friction rows in the coupled solve):
      // rcsh_sim_add_free_box checked the archetype
      if constexpr (T::NARM == 7 && T::GRIP) {
        if (s->dm.has_friction) go(Y{}, Y{}, Y{});
        else go(N{}, Y{}, Y{});
      }
    } else if (s->box.present) {
      // scenes with a free box that only touches the floor: FR3 + hand, and the 7-dof arm with dry joint friction
      if constexpr (T::NARM == 7 && T::GRIP) go(N{}, Y{}, N{});
      else if constexpr (T::NARM == 7) go(Y{}, Y{}, N{});
    } else if (s->box.resolve) {
      // no free body, contacts of the robot with the floor and with itself resolved (rcsh_sim_set_contact_options; FR3 + hand):
      // by the whole batch on the contact-resolving kernel, or environment by environment (RunOp::esc_role)
      if constexpr (T::NARM == 7 && T::GRIP) {
        if (esc) {
          // (the certifying check -- check_team.h -- is the default; RCSH_CHECK_CERTIFY=0: the check of the final position alone, round 5's)
          static const int certify = [] { const char* e = std::getenv("RCSH_CHECK_CERTIFY"); return e ? std::atoi(e) : 1; }();
          // Three launches, one behind the other: the lean launch over EVERY environment, which records where each
          // substep began; the verify launch, the collision passes of the substeps of whoever failed the certificate, side by side; the
          // contact-resolving launch over the environments one of those passes found touching, each redone from the copy.
          // RCSH_ESC_VERIFY=0 (read on every launch), launches longer than the trace and step_until_convergence's pieces take the two
          // launches of before: the lean launch over the environments not escalated, the contact-resolving launch over the others.
          const char* ev = std::getenv("RCSH_ESC_VERIFY");
          const int nsub = op.do_reset ? 1 : op.nsteps;
          const bool verify = !(ev && std::atoi(ev) == 0) && certify && !det && nsub > 0 && nsub <= kEscTraceCap;
          if (verify) { op.trace = s->esc.trace.get(); op.esc_part = 2; }
          op.esc_role = 1; op.check = certify ? 2 : 1;
          go(N{}, N{}, N{});
          if (verify) {
            const char* vm = std::getenv("RCSH_VERIFY_MAX");  // (read on every launch, like RCSH_ESC_VERIFY: the tests switch it)
            hipLaunchKernelGGL((k_verify_team<T>), dim3(kVerifyGrid), block, 0, s->stream, P, op, nsub, vm ? std::atoi(vm) : kVerifyMaxFlagged);
          }
          op.esc_role = 2; op.check = certify ? 2 : 0;
          go(N{}, N{}, Y{});
        } else {
          op.force_contact = (s->box.resolve & 2) ? 1 : 0;
          go(N{}, N{}, Y{});
        }
      }
    } else if (s->dm.has_friction)
      go(Y{}, N{}, N{});
    else
      go(N{}, N{}, N{});
#endif
    err = hipGetLastError();
  });
  if (!ok || !launched) return fail(RCSH_ERR_MODEL, "no kernel instantiated for this archetype");
  if (err != hipSuccess) return fail(RCSH_ERR_DEVICE, std::string("k_run launch: ") + hipGetErrorString(err));
  if (sample) {
    HIP_TRY(hipEventRecord(s->ev_stop[s->prof_pending].get(), s->stream));
    s->prof_pending++;
  }
  return RCSH_OK;
}

template <class F>
auto with_layout(rcsh_sim* s, F&& fn) {
  int out = -1;
  dispatch_topology(s->narm, s->grip, [&](auto topo) { out = fn(topo); });
  return out;
}

int field_of(rcsh_sim* s, const char* name) {
  return with_layout(s, [&](auto topo) {
    using L = Lay<decltype(topo)>;
    std::string f(name);
    if (f == "qpos") return (int)L::QPOS;
    if (f == "qvel") return (int)L::QVEL;
    if (f == "ctrl") return (int)L::CTRL;
    if (f == "time") return (int)L::TIME;
    if (f == "cb") return (int)L::CB;
    if (f == "prevq") return (int)L::PREVQ;
    if (f == "target") return (int)L::TARGET;
    if (f == "grip") return (int)L::GRIP;
    if (f == "site") return (int)L::SITE;
    if (f == "preva") return (int)L::PREVA;
    if (f == "origin") return (int)L::ORIGIN;
    if (f == "lasta") return (int)L::LASTA;
    if (f == "box") return (int)L::BOX;
    if (f == "qpre") return (int)L::QPRE;
    if (f == "xs") return (int)L::XS;
    if (f == "sep") return (int)L::SEP;
    return -1;
  });
}

// ---- staging of the host-pointer entry points
constexpr int kStageWidth = 48;  // doubles per environment of the widest field group (the free body's state)
constexpr int kInfoBytes = 8, kPoseWidth = 7, kTaskWidth = 9, kObsBase = 14;  // info row; pose; task row = box pose + reward + terminated; observation = kObsBase + narm
constexpr int kPairWidth = 2, kWitnessWidth = 6, kJacRows = 6, kCamPoseWidth = 12, kRgbWidth = 3;  // geom ids of a pair; two witness points; rows of the TCP Jacobian; camera xmat + xpos; bytes of a pixel
static_assert(kBoxState <= kStageWidth, "the free body's state passes through the staging buffer in one piece");
static_assert(kPoseWidth <= kTaskWidth, "the box pose comes in through the task rows' slice");
static_assert(kPoseWidth <= kObsBase, "a forward-kinematics pose goes out through the observations' slice");

int action_width(int mode, int narm) {
  if (mode == RCSH_MODE_JOINTS || mode == RCSH_MODE_TORQUE || mode == RCSH_MODE_JOINT_IMPEDANCE) return narm;
  return mode == RCSH_MODE_CARTESIAN_TRPY || mode == RCSH_MODE_CARTESIAN_IMPEDANCE_TRPY ? 6 : kPoseWidth;
}

int fits(int width, int slice_width, const char* what) {
  if (width < 0 || width > slice_width) return fail(RCSH_ERR_ARG, std::string(what) + ": wider than its staging slice");
  return RCSH_OK;
}

// The device staging's layout: every slice's place and width is decided here, from n and the model's widths.  Called twice: without
// a base for the size, then with the allocation.
size_t stage_layout(Staging& st, size_t n, uintptr_t base) {
  size_t o = 0;
  auto take = [&](auto*& p, size_t count) {
    p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(base + o);
    o += (count * sizeof(*p) + 255) & ~size_t(255);
  };
  take(st.mask, n); take(st.inv_mask, n); take(st.info, n * kInfoBytes); take(st.flag, n); take(st.substeps, n);
  take(st.grip_cmd, n); take(st.grip_width, n); take(st.action, n * st.action_w); take(st.box_task, n * kTaskWidth);
  take(st.obs, n * st.obs_w); take(st.wide, n * kStageWidth); take(st.pose, n * kPoseWidth); take(st.q0, n * st.q0_w);
  take(st.tcp, kPoseWidth);
  return o;
}
int stage_create(rcsh_sim* s) {
  Staging& st = s->stage;
  const size_t n = (size_t)s->n;
  for (int mode = RCSH_MODE_JOINTS; mode <= RCSH_MODE_CARTESIAN_TQUAT; ++mode) st.action_w = std::max(st.action_w, action_width(mode, s->narm));
  st.obs_w = kObsBase + s->narm;
  st.q0_w = s->narm;
  if (s->nl > st.obs_w) return fail(RCSH_ERR_MODEL, "the inverse kinematics' output (nq wide) does not fit the observations' staging slice");
  HIP_TRY(hipMalloc(st.base.out(), stage_layout(st, n, 0)));
  stage_layout(st, n, reinterpret_cast<uintptr_t>(st.base.get()));
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 63) & ~size_t(63); return at; };
  PinLayout& L = s->pin;
  L.action = take(sizeof(double) * n * st.action_w);
  L.gripper = take(sizeof(float) * n);
  L.box = take(sizeof(double) * n * kPoseWidth);
  L.obs = take(sizeof(double) * n * st.obs_w);
  L.info = take(n * kInfoBytes);
  L.gw = take(sizeof(double) * n);
  L.sub = take(sizeof(int32_t) * n);
  L.task = take(sizeof(double) * n * kTaskWidth);
  L.total = o;
  return RCSH_OK;
}

int upload_mask(rcsh_sim* s, const uint8_t* mask, const uint8_t** dev) {
  *dev = nullptr;
  if (!mask) return RCSH_OK;
  HIP_TRY(hipMemcpyAsync(s->stage.mask, mask, s->n, hipMemcpyHostToDevice, s->stream));
  *dev = s->stage.mask;
  return RCSH_OK;
}

// The state was written from outside the stepping launches (set_joints_hard, mjData.qpos = ..., a snapshot, another contact option) and
// the robot may have moved: the gaps the contact check and the contact phase remember for the old position are void; zero = "look at everything".
int void_remembered_gaps(rcsh_sim* s) {
  if (s->d_slack) HIP_TRY(hipMemsetAsync(s->d_slack.get(), 0, sizeof(float) * (size_t)kSlackStride * s->n, s->stream));
  return RCSH_OK;
}

// host [n][width] -> state fields
int scatter_host(rcsh_sim* s, int field0, int width, const double* src, const uint8_t* mask) {
  if (width > kStageWidth) return fail(RCSH_ERR_ARG, "scatter_host: field group wider than the staging buffer");
  const uint8_t* dm = nullptr;
  int rc = upload_mask(s, mask, &dm);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(s->stage.wide, src, sizeof(double) * s->n * width, hipMemcpyHostToDevice, s->stream));
  if ((rc = void_remembered_gaps(s))) return rc;
  hipLaunchKernelGGL(k_scatter, dim3(grid_for(s->n)), dim3(kBlock), 0, s->stream, s->S.get(), s->n, field0, width, s->stage.wide, dm);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s->stream));
  return RCSH_OK;
}

int gather_host(rcsh_sim* s, int field0, int width, double* dst) {
  if (width > kStageWidth) return fail(RCSH_ERR_ARG, "gather_host: field group wider than the staging buffer");
  hipLaunchKernelGGL(k_gather, dim3(grid_for(s->n)), dim3(kBlock), 0, s->stream, (const double*)s->S.get(), s->n, field0, width, s->stage.wide);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(dst, s->stage.wide, sizeof(double) * s->n * width, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return RCSH_OK;
}

int flag_host(rcsh_sim* s, uint32_t bit, uint8_t* dst) {
  if (!dst) return RCSH_OK;
  hipLaunchKernelGGL(k_flags_to_bytes, dim3(grid_for(s->n)), dim3(kBlock), 0, s->stream, (const uint32_t*)s->flags.get(), s->n, bit, s->stage.flag);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(dst, s->stage.flag, s->n, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return RCSH_OK;
}

// flags |= set, &= ~clear for masked environments: a small kernel on the handle's stream, so that it is ordered with
// everything the *_dev entry points enqueued there
int flags_update_host(rcsh_sim* s, uint32_t set, uint32_t clear, const uint8_t* mask) {
  const uint8_t* dm = nullptr;
  int rc = upload_mask(s, mask, &dm);
  if (rc) return rc;
  hipLaunchKernelGGL(k_flags_update, dim3(grid_for(s->n)), dim3(kBlock), 0, s->stream, s->flags.get(), s->n, set, clear, dm);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s->stream));
  return RCSH_OK;
}

// Host-buffer env.reset(mask): the reset launch writes observation / info / gripper width of the masked environments only,
// the rows of the others in the staging slices would be whatever an earlier call left there.  An observation-only
// pass (no stepping) over the complement fills them with the environments' current observation.
int observe_unmasked(rcsh_sim* s, const uint8_t* mask) {
  if (!mask) return RCSH_OK;
  std::vector<uint8_t> inv(s->n);
  bool any = false;
  for (int e = 0; e < s->n; ++e) { inv[e] = !mask[e]; any = any || inv[e]; }
  if (!any) return RCSH_OK;
  HIP_TRY(hipMemcpyAsync(s->stage.inv_mask, inv.data(), s->n, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));  // `inv` goes out of scope
  RunOp op{};
  op.nsteps = 0;
  op.write_obs = 1;
  op.observe_only = 1;  // the frames the reset launch just recorded for the masked environments stay pending (rend.count / last)
  op.mask = s->stage.inv_mask;
  op.obs = s->stage.obs; op.info = s->stage.info; op.gripper_width = s->stage.grip_width;
  return launch_run(s, op, false);
}

size_t align8(size_t x) { return (x + 7) & ~(size_t)7; }
// a record of the collision guard (rcsh_sim::d_guard holds two, h_guard the front of one): [t_contact | result | blocked | hold]
struct GuardLayout { size_t t_contact, result, blocked, hold, host_bytes, bytes; };  // host_bytes: up to the end of `blocked`, what a host copy takes
GuardLayout guard_layout(const rcsh_sim* s) {
  const size_t n = (size_t)s->n;
  GuardLayout G{};
  G.result = G.t_contact + align8(8 * n);
  G.blocked = G.result + align8(4 * n);
  G.hold = G.blocked + align8(n);
  G.host_bytes = G.blocked + n;
  G.bytes = G.hold + align8(n);
  return G;
}

// the autoreset's record (rcsh_sim::d_episode; offsets in bytes, every slice 8-byte aligned).  The front -- up to host_bytes -- is what
// a host form of env.step brings along: [episode_return | episode_length | done | terminated | truncated | time_limit]
struct EpisodeLayout {
  size_t episode_return, episode_length, done, terminated, truncated, time_limit, host_bytes;
  size_t final_obs, final_info, final_gw, final_task, episodes, elapsed, running_return, reset_info, reset_box_qpos, bytes;
};
EpisodeLayout episode_layout(const rcsh_sim* s) {
  const size_t n = (size_t)s->n;
  EpisodeLayout E{};
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += align8(bytes); return at; };
  E.episode_return = take(8 * n); E.episode_length = take(4 * n);
  E.done = take(n); E.terminated = take(n); E.truncated = take(n); E.time_limit = take(n);
  E.host_bytes = o;
  E.final_obs = take(8 * n * (size_t)(kObsBase + s->narm)); E.final_info = take(n * kInfoBytes); E.final_gw = take(8 * n);
  E.final_task = take(8 * n * kTaskWidth); E.episodes = take(8 * n); E.elapsed = take(4 * n); E.running_return = take(8 * n);
  E.reset_info = take(n * kInfoBytes); E.reset_box_qpos = take(8 * n * kPoseWidth);
  E.bytes = o;
  return E;
}

// the page-locked buffer (laid out by rcsh_sim::pin), allocated at its first use
int pin_ready(rcsh_sim* s, char*& h) {
  int rc = grow_pinned(s, s->h_pin, s->pin.total);
  h = static_cast<char*>(s->h_pin.p.get());
  return rc;
}
// host array -> page-locked memory -> device slice, enqueued (the entry point's closing wait covers it)
int pin_upload(rcsh_sim* s, void* dev, char* pinned, const void* src, size_t bytes) {
  std::memcpy(pinned, src, bytes);
  HIP_TRY(hipMemcpyAsync(dev, pinned, bytes, hipMemcpyHostToDevice, s->stream));
  return RCSH_OK;
}
// How the env layer's host forms end: the requested outputs go from their slices to page-locked memory -- with the last guarded step's
// record and the front of the autoreset's, if asked: rcsh_env_guard_last / rcsh_env_autoreset_last then need no wait of their own --,
// ONE wait, and out to the caller's arrays.
struct EnvOut { double* obs; uint8_t* info; double* gw; int32_t* substeps; double* task; };
int fetch_env_outputs(rcsh_sim* s, const EnvOut& out, bool guard_record_too, bool episode_record_too = false) {
  const PinLayout& L = s->pin;
  char* h = nullptr;
  int rc = pin_ready(s, h);
  if (rc) return rc;
  const Staging& st = s->stage;
  const size_t n = (size_t)s->n;
  const struct { void* dst; const void* src; size_t at, bytes; } pieces[] = {
      {out.obs, st.obs, L.obs, sizeof(double) * n * st.obs_w}, {out.info, st.info, L.info, n * kInfoBytes},
      {out.gw, st.grip_width, L.gw, sizeof(double) * n},       {out.substeps, st.substeps, L.sub, sizeof(int32_t) * n},
      {out.task, st.box_task, L.task, sizeof(double) * n * kTaskWidth}};
  for (const auto& p : pieces)
    if (p.dst) HIP_TRY(hipMemcpyAsync(h + p.at, p.src, p.bytes, hipMemcpyDeviceToHost, s->stream));
  if (guard_record_too) HIP_TRY(hipMemcpyAsync(s->h_guard.get(), s->d_guard.get(), guard_layout(s).host_bytes, hipMemcpyDeviceToHost, s->stream));
  if (episode_record_too) HIP_TRY(hipMemcpyAsync(s->h_episode.get(), s->d_episode.get(), episode_layout(s).host_bytes, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  for (const auto& p : pieces)
    if (p.dst) std::memcpy(p.dst, h + p.at, p.bytes);
  return RCSH_OK;
}

std::vector<double> tile(const double* row, int width, int n) {
  std::vector<double> v((size_t)n * width);
  for (int e = 0; e < n; ++e) std::memcpy(&v[(size_t)e * width], row, sizeof(double) * width);
  return v;
}

// The launch of a team kernel over m rows, four to a wavefront: launch(topo, grid, block) enqueues it for the archetype; `what` names
// it in the error text.
template <class F>
int team_launch(rcsh_sim* s, int32_t m, const char* what, F&& launch) {
  hipError_t err = hipSuccess;
  const bool ok = dispatch_topology(s->narm, s->grip, [&](auto topo) {
    launch(topo, dim3((m + 3) / 4), dim3(64));
    err = hipGetLastError();
  });
  if (!ok) return fail(RCSH_ERR_MODEL, "no kernel instantiated for this archetype");
  if (err != hipSuccess) return fail(RCSH_ERR_DEVICE, std::string(what) + " launch: " + hipGetErrorString(err));
  return RCSH_OK;
}
// the pair set of a query (model.cpp); the free body's geom is the scene's last, split off its articulated tables
QueryPairs query_pairs(rcsh_sim* s, int32_t kinds, bool with_ids = true) {
  return build_query_pairs(s->hm, s->cp, s->cgeoms, s->tables.chk_pairs, s->box.present ? s->hm.ngeom : -1, kinds, with_ids);
}

// every entry point works on the handle's own GPU, whatever device the calling thread had current
#define REQUIRE_SIM(s)                                        \
  if (!(s)) return fail(RCSH_ERR_ARG, "null sim handle"); \
  HIP_TRY(hipSetDevice((s)->device))
#define REQUIRE_ROBOT(s) \
  if (!(s)->robot.present) return fail(RCSH_ERR_STATE, "no robot attached: call rcsh_sim_add_robot first")
#define REQUIRE_GRIPPER(s) \
  if (!(s)->gripcfg.present) return fail(RCSH_ERR_STATE, "no gripper attached: call rcsh_sim_add_gripper first")

// ---- torque control (csrc/torque_team.h)
static_assert(RCSH_MAX_ARM == kMaxArm, "rcsh_torque_law's gain rows are the model's arm bound");
#define REQUIRE_TORQUE(s, what) \
  if (!(s)->tq.actuated) return fail(RCSH_ERR_ARG, std::string(what) + ": the robot is not torque-actuated (an arm actuator has a bias: a servo)")
// the targets and the singular bytes, zeroed, at their first use
int torque_buffers(rcsh_sim* s) {
  if (s->tq.target) return RCSH_OK;
  const size_t n = (size_t)s->n, w = (size_t)(kTorquePose + s->narm);
  DevBuf<double> tg;
  DevBuf<uint8_t> sg;
  HIP_TRY(hipMalloc(tg.out(), sizeof(double) * w * n));
  HIP_TRY(hipMalloc(sg.out(), n));
  HIP_TRY(hipMemsetAsync(tg.get(), 0, sizeof(double) * w * n, s->stream));
  HIP_TRY(hipMemsetAsync(sg.get(), 0, n, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  s->tq.target = std::move(tg);
  s->tq.singular = std::move(sg);
  return RCSH_OK;
}
// what the torque kernels are handed: the law with its TCP resolved into the site link's frame -- the pose rcsh_ik_forward reports is
// site * offset^-1 (quirk Q7), as the dynamics queries take it
TorqueArgs torque_args(rcsh_sim* s, const rcsh_torque_law& law, int32_t k) {
  TorqueArgs A{};
  A.model = s->d_model.get();
  A.S = s->S.get();
  A.n = s->n;
  A.k = k;
  A.keep_qpre = bool(s->rbuf.frames);
  A.enabled = law.enabled;
  A.target = s->tq.target.get();
  A.singular = s->tq.singular.get();
  TorqueLawDev& d = A.law;
  d.task_mask = law.task_mask;
  d.compensate_bias = law.compensate_bias;
  d.damping = law.damping;
  d.rel_pivot = RCSH_OPSPACE_REL_PIVOT;
  const double* o = law.tcp_offset7;
  const double nq = std::sqrt(o[3] * o[3] + o[4] * o[4] + o[5] * o[5] + o[6] * o[6]);
  double Roff[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, off[3] = {0, 0, 0};
  if (nq > 0.0) {
    const double qn[4] = {o[3] / nq, o[4] / nq, o[5] / nq, o[6] / nq};
    quat_to_mat(qn, Roff);
    for (int c = 0; c < 3; ++c) off[c] = -(Roff[c] * o[0] + Roff[3 + c] * o[1] + Roff[6 + c] * o[2]);
  }
  const double* sr = s->dm.site_rot;
  for (int r = 0; r < 3; ++r) {
    d.tcp_p[r] = s->dm.site_pos[r] + sr[3 * r] * off[0] + sr[3 * r + 1] * off[1] + sr[3 * r + 2] * off[2];
    for (int c = 0; c < 3; ++c) d.tcp_R[3 * r + c] = sr[3 * r] * Roff[3 * c] + sr[3 * r + 1] * Roff[3 * c + 1] + sr[3 * r + 2] * Roff[3 * c + 2];  // site_rot Roff^T
    d.base_p[r] = s->dm.base_pos[r];
  }
  const double bq[4] = {s->dm.base_quat[1], s->dm.base_quat[2], s->dm.base_quat[3], s->dm.base_quat[0]};
  quat_to_mat(bq, d.base_R);
  for (int r = 0; r < kTaskRows; ++r) { d.task_k[r] = law.task_k[r]; d.task_d[r] = law.task_d[r]; }
  for (int i = 0; i < kMaxArm; ++i) { d.joint_k[i] = law.joint_k[i]; d.joint_d[i] = law.joint_d[i]; }
  return A;
}
// why the fused launch does not serve this handle (empty: it does)
std::string torque_scope(const rcsh_sim* s) {
  if (!s->tq.actuated) return "the robot is not torque-actuated (an arm actuator has a bias: a servo)";
  if (s->box.present) return "the scene has a free body";
  if (s->box.resolve) return "robot contacts are resolved (rcsh_sim_set_contact_options)";
  if (s->rend.ncam > 0) return "rate-driven cameras are scheduled (rcsh_sim_set_render_schedule)";
  if (s->dm.site_link < 0) return "the attachment site is static";
  return "";
}
// q_des (device, [n][narm], null: keep) and / or pose7 (device, [n][7], null: keep) into the targets of the masked environments
int torque_target_dev(rcsh_sim* s, const double* pose7, const double* q_des, const uint8_t* mask_dev) {
  if (int rc = torque_buffers(s)) return rc;
  if (pose7) hipLaunchKernelGGL(k_scatter, dim3(grid_for(s->n)), dim3(kBlock), 0, s->stream, s->tq.target.get(), s->n, 0, kTorquePose, pose7, mask_dev);
  if (q_des) hipLaunchKernelGGL(k_scatter, dim3(grid_for(s->n)), dim3(kBlock), 0, s->stream, s->tq.target.get(), s->n, kTorquePose, s->narm, q_des, mask_dev);
  HIP_TRY(hipGetLastError());
  return RCSH_OK;
}
// A torque-actuated robot after set_joint_position / move_home / a reset to q (host, [n][narm]): zero torque, and the law's targets at
// that configuration and its TCP pose.  `clear`: the singular bytes of the masked environments too (the resets).
int torque_rest_at(rcsh_sim* s, const double* q, const uint8_t* mask, bool clear) {
  if (int rc = torque_buffers(s)) return rc;
  std::vector<double> z((size_t)s->n * s->narm, 0.0);
  int rc = scatter_host(s, field_of(s, "ctrl"), s->narm, z.data(), mask);
  if (rc) return rc;
  const uint8_t* dm = nullptr;
  if ((rc = upload_mask(s, mask, &dm))) return rc;
  HIP_TRY(hipMemcpyAsync(s->stage.wide, q, sizeof(double) * s->n * s->narm, hipMemcpyHostToDevice, s->stream));
  if ((rc = torque_target_dev(s, nullptr, s->stage.wide, dm))) return rc;
  TorqueArgs A = torque_args(s, s->tq.law, 0);
  rc = team_launch(s, s->n, "torque target pose", [&](auto topo, dim3 grid, dim3 block) {
    hipLaunchKernelGGL(k_torque_target_pose<decltype(topo)>, grid, block, 0, s->stream, A, dm);
  });
  if (rc) return rc;
  if (clear) {
    if (!mask) HIP_TRY(hipMemsetAsync(s->tq.singular.get(), 0, s->n, s->stream));
    else {
      std::vector<uint8_t> sg(s->n);
      HIP_TRY(hipMemcpyAsync(sg.data(), s->tq.singular.get(), s->n, hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipStreamSynchronize(s->stream));
      for (int e = 0; e < s->n; ++e) sg[e] = mask[e] ? 0 : sg[e];
      HIP_TRY(hipMemcpyAsync(s->tq.singular.get(), sg.data(), s->n, hipMemcpyHostToDevice, s->stream));
    }
  }
  HIP_TRY(hipStreamSynchronize(s->stream));
  return RCSH_OK;
}

}  // namespace

extern "C" {

const char* rcsh_last_error(void) { return g_err.c_str(); }
int rcsh_abi_version(void) { return RCSH_ABI_VERSION; }
int rcsh_device_count(void) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return 0;
  return c;
}

int rcsh_sim_create(const rcsh_model_desc* model, int32_t n_envs, int32_t device, rcsh_sim** out) {
  if (!model || !out || n_envs < 1) return fail(RCSH_ERR_ARG, "rcsh_sim_create: bad arguments");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
    return fail(RCSH_ERR_DEVICE, "no HIP device available: the batched backend has no CPU path");
  if (device < 0 || device >= count) return fail(RCSH_ERR_DEVICE, "device index out of range");
  struct Destroy { void operator()(rcsh_sim* s) const { rcsh_sim_destroy(s); } };
  std::unique_ptr<rcsh_sim, Destroy> owner(new rcsh_sim());  // (every return before the last destroys the half-built handle)
  rcsh_sim* s = owner.get();
  s->device = device;
  s->hm.copy_from(*model);
  std::string why = finalize_model(s->hm, s->dm, s->act_slot);
  if (!why.empty()) return fail(RCSH_ERR_MODEL, why);
  s->n = n_envs;
  s->narm = s->dm.narm; s->nl = s->dm.nl; s->grip = s->dm.has_gripper != 0;
  s->nu = s->narm + (s->grip ? 1 : 0);
  s->nfields = with_layout(s, [&](auto topo) { return (int)Lay<decltype(topo)>::COUNT; });
  HIP_TRY(hipSetDevice(device));
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) s->n_simd = 4 * cus;
  }
  HIP_TRY(hipStreamCreateWithFlags(s->own_stream.out(), hipStreamNonBlocking));
  s->stream = s->own_stream.get();
  const size_t n = (size_t)n_envs;
  HIP_TRY(hipMalloc(s->d_model.out(), sizeof(DevModel) + sizeof(LinkRec) * kMaxLinks));
  {
    std::string cwhy = build_collision_points(s->hm, s->cp);
    if (!cwhy.empty()) return fail(RCSH_ERR_MODEL, cwhy);
    s->cp_class.assign(s->cp.geom.size(), 0);
    cwhy = build_contact_table(s->hm, s->dm, s->cp.has_plane ? s->cp.plane_geom : -1, s->cgeoms, s->cverts, s->contact_overflow, &s->cgeoms_dropped);
    if (!cwhy.empty()) return fail(RCSH_ERR_MODEL, cwhy);
    if (s->cp.has_plane) s->plane_mu = s->hm.geom_friction[3 * (size_t)s->cp.plane_geom];
    if (!s->cp.geom.empty()) {
      HIP_TRY(hipMalloc(s->d_coll_xyzr.out(), sizeof(double) * s->cp.xyzr.size()));
      HIP_TRY(hipMalloc(s->d_coll_cls.out(), s->cp_class.size()));
      HIP_TRY(hipMemcpy(s->d_coll_xyzr.get(), s->cp.xyzr.data(), sizeof(double) * s->cp.xyzr.size(), hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(s->d_coll_cls.get(), s->cp_class.data(), s->cp_class.size(), hipMemcpyHostToDevice));
    }
  }
  HIP_TRY(hipMalloc(s->S.out(), sizeof(double) * n * s->nfields));
  HIP_TRY(hipMalloc(s->flags.out(), sizeof(uint32_t) * n));
  HIP_TRY(hipMalloc(s->conv.out(), sizeof(int32_t) * n));
  if (int rc = stage_create(s)) return rc;
  HIP_TRY(hipMemsetAsync(s->S.get(), 0, sizeof(double) * n * s->nfields, s->stream));
  HIP_TRY(hipMemsetAsync(s->conv.get(), 0, sizeof(int32_t) * n, s->stream));
  // Sim::converged starts true (reference src/sim/sim.h:70); SimRobotState.ik_success starts true
  {
    std::vector<uint32_t> f(n, kConverged | kIkSuccess);
    HIP_TRY(hipMemcpyAsync(s->flags.get(), f.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
  }
  // mjData starts at qpos0
  {
    std::vector<double> q0 = tile(s->dm.qpos0, s->nl, n_envs);
    int rc = scatter_host(s, field_of(s, "qpos"), s->nl, q0.data(), nullptr);
    if (!rc) rc = scatter_host(s, field_of(s, "qpre"), s->nl, q0.data(), nullptr);
    if (rc) return rc;
  }
  if (int rc = upload_model(s)) return rc;
  if (const char* cc = std::getenv("RCSH_CONTACT_CHECK")) s->contact_check = std::atoi(cc) != 0;
  if (const char* rf = std::getenv("RCSH_RENDER_F64")) s->render_f64 = std::atoi(rf) != 0;
  if (int rc = upload_contact_table(s)) return rc;  // (the contact check's pair tables exist before any robot is attached)
  *out = owner.release();
  return RCSH_OK;
}

// What has an order is written out; the rest is the handle's members, destroyed in reverse (own_stream last).
void rcsh_sim_destroy(rcsh_sim* s) {
  if (!s) return;
  hipSetDevice(s->device);
  if (s->stream) hipStreamSynchronize(s->stream);
  rcsh_comm_destroy(s);
  delete s;
}

int rcsh_sim_num_envs(const rcsh_sim* s) { return s ? s->n : 0; }
int rcsh_sim_nq(const rcsh_sim* s) { return s ? s->nl : 0; }
int rcsh_sim_nu(const rcsh_sim* s) { return s ? (int)s->act_slot.size() : 0; }
void* rcsh_sim_stream(rcsh_sim* s) { return s ? (void*)s->stream : nullptr; }

int rcsh_sim_set_stream(rcsh_sim* s, void* hip_stream) {
  REQUIRE_SIM(s);
  HIP_TRY(hipStreamSynchronize(s->stream));
  s->stream = hip_stream ? (hipStream_t)hip_stream : s->own_stream.get();
  return RCSH_OK;
}

int rcsh_sim_wait_for(rcsh_sim* s, rcsh_sim* producer) {
  REQUIRE_SIM(s);
  if (!producer) return fail(RCSH_ERR_ARG, "null producer handle");
  if (producer == s || producer->stream == s->stream) return RCSH_OK;  // same stream: already ordered
  HIP_TRY(hipSetDevice(producer->device));
  if (!producer->order_ev) HIP_TRY(hipEventCreateWithFlags(producer->order_ev.out(), hipEventDisableTiming));
  HIP_TRY(hipEventRecord(producer->order_ev.get(), producer->stream));
  HIP_TRY(hipStreamWaitEvent(s->stream, producer->order_ev.get(), 0));
  return RCSH_OK;
}

int rcsh_sim_set_kernel(rcsh_sim* s, int32_t variant) {
  REQUIRE_SIM(s);
  if (variant == RCSH_KERNEL_LANE) return fail(RCSH_ERR_ARG, "the one-lane-per-environment kernel was removed (ABI 2): every scene runs on the team kernel");
  if (variant != RCSH_KERNEL_AUTO && variant != RCSH_KERNEL_TEAM && variant != RCSH_KERNEL_TEAM_OCC2) return fail(RCSH_ERR_ARG, "unknown kernel variant");
  s->kernel = variant;
  return RCSH_OK;
}

int rcsh_sim_synchronize(rcsh_sim* s) {
  REQUIRE_SIM(s);
  HIP_TRY(hipStreamSynchronize(s->stream));
  return RCSH_OK;
}

int rcsh_sim_set_config(rcsh_sim* s, int32_t async_control, int32_t realtime, int32_t frequency, int32_t max_convergence_steps) {
  REQUIRE_SIM(s);
  if (frequency <= 0) return fail(RCSH_ERR_ARG, "SimConfig.frequency must be positive");
  s->sim = SimCfg{async_control, realtime, frequency, max_convergence_steps};
  return RCSH_OK;
}
int rcsh_sim_get_config(const rcsh_sim* s, int32_t* a, int32_t* r, int32_t* f, int32_t* m) {
  REQUIRE_SIM(s);
  if (a) *a = s->sim.async_control;
  if (r) *r = s->sim.realtime;
  if (f) *f = s->sim.frequency;
  if (m) *m = s->sim.max_convergence_steps;
  return RCSH_OK;
}

int rcsh_sim_step(rcsh_sim* s, int64_t k) {
  REQUIRE_SIM(s);
  if (k < 0) return fail(RCSH_ERR_ARG, "step count must be non-negative");
  RunOp op{};
  op.nsteps = (int32_t)k;
  int rc = launch_run(s, op, false);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  return RCSH_OK;
}

int rcsh_sim_step_until_convergence(rcsh_sim* s) {
  REQUIRE_SIM(s);
  if (s->tq.actuated) return fail(RCSH_ERR_ARG, "step_until_convergence: the robot is torque-actuated; the convergence predicates assume position servos");
  RunOp op{};
  op.nsteps = -1;
  int rc = launch_run(s, op, false);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  return RCSH_OK;
}

int rcsh_sim_is_converged(rcsh_sim* s, uint8_t* converged, int32_t* steps) {
  REQUIRE_SIM(s);
  int rc = flag_host(s, kConverged, converged);
  if (rc) return rc;
  if (steps) {
    HIP_TRY(hipMemcpyAsync(steps, s->conv.get(), sizeof(int32_t) * s->n, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
  }
  return RCSH_OK;
}

int rcsh_sim_reset(rcsh_sim* s, const uint8_t* mask) {
  REQUIRE_SIM(s);
  // mj_resetData: qpos := qpos0, qvel := 0, ctrl := 0, time := 0; reset_callbacks: timestamps := 0
  std::vector<double> z((size_t)s->n * 32, 0.0);
  static_assert(kBoxState - kBoxX <= 32, "the zero block covers the coupled solve's warm start");
  std::vector<double> q0 = tile(s->dm.qpos0, s->nl, s->n);
  int rc = scatter_host(s, field_of(s, "qpos"), s->nl, q0.data(), mask);
  if (!rc) rc = scatter_host(s, field_of(s, "qpre"), s->nl, q0.data(), mask);
  if (!rc) rc = scatter_host(s, field_of(s, "qvel"), s->nl, z.data(), mask);
  if (!rc) rc = scatter_host(s, field_of(s, "ctrl"), s->nu, z.data(), mask);
  if (!rc) rc = scatter_host(s, field_of(s, "time"), 1, z.data(), mask);
  if (!rc) rc = scatter_host(s, field_of(s, "cb"), 6, z.data(), mask);
  if (!rc) rc = scatter_host(s, field_of(s, "xs"), s->nl, z.data(), mask);  // (mj_resetData: qacc_warmstart := 0)
  if (!rc) rc = flags_update_host(s, 0, kContactOverflow | kContactUnresolved | kContactResolved | kEscQuiet, mask);
  if (!rc) rc = scatter_host(s, field_of(s, "sep"), kCheckSep, z.data(), mask);
  if (!rc && s->tq.actuated && s->robot.present) {
    // a torque-actuated robot: the law's targets go to the reset configuration and its pose, the singular bytes are cleared
    std::vector<double> qa((size_t)s->n * s->narm);
    for (int e = 0; e < s->n; ++e)
      for (int i = 0; i < s->narm; ++i) qa[(size_t)e * s->narm + i] = s->dm.qpos0[i];
    rc = torque_rest_at(s, qa.data(), mask, true);
  }
  if (!rc && s->esc.mask) {
    // per-environment escalation: a reset environment starts over on the lean kernel
    const size_t nw = ((size_t)s->n + 63) / 64;
    std::vector<uint64_t> w(kEscRows * nw, 0);
    if (mask) {
      HIP_TRY(hipMemcpyAsync(w.data(), s->esc.mask.get(), sizeof(uint64_t) * nw, hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipStreamSynchronize(s->stream));
      for (int e = 0; e < s->n; ++e)
        if (mask[e]) w[e >> 6] &= ~(1ull << (e & 63));
    }
    HIP_TRY(hipMemcpyAsync(s->esc.mask.get(), w.data(), sizeof(uint64_t) * kEscRows * nw, hipMemcpyHostToDevice, s->stream));
    uint32_t ctr[4] = {0, 0, 0, 0};  // (RunOp::esc_ctr: [1] has to say how many are escalated -- a role-2 launch trusts a zero)
    for (size_t i = 0; i < nw; ++i) ctr[1] += (uint32_t)__builtin_popcountll(w[i]);
    HIP_TRY(hipMemcpyAsync(s->esc.ctr.get(), ctr, sizeof(ctr), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
  }
  if (!rc && s->box.present) {
    std::vector<double> b0((size_t)s->n * kBoxState, 0.0);
    for (int e = 0; e < s->n; ++e)
      for (int k = 0; k < 7; ++k) b0[(size_t)e * kBoxState + k] = b0[(size_t)e * kBoxState + kBoxPre + k] = s->box.qpos0[k];
    rc = scatter_host(s, field_of(s, "box"), kBoxState, b0.data(), mask);
  } else if (!rc && s->box.resolve) {
    // contacts resolved without a free body: the phantom box's slot carries the coupled solve's warm start from launch to launch
    // (mjData.qacc_warmstart); mj_resetData zeroes it, so that a reset sim reproduces a fresh one bit for bit (advisor, round 3)
    rc = scatter_host(s, field_of(s, "box") + kBoxX, kBoxState - kBoxX, z.data(), mask);
  }
  if (!rc && s->rend.ncam > 0) {
    // reset_callbacks (sim.cpp:131-137): the cameras' clocks go back to -seconds_between_calls
    const size_t n = (size_t)s->n;
    std::vector<double> last(kMaxRateCams * n);
    HIP_TRY(hipMemcpyAsync(last.data(), s->rend.last, sizeof(double) * last.size(), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    for (int c = 0; c < s->rend.ncam; ++c)
      for (size_t e = 0; e < n; ++e)
        if (!mask || mask[e]) last[c * n + e] = -s->rend.period[c];
    HIP_TRY(hipMemcpyAsync(s->rend.last, last.data(), sizeof(double) * last.size(), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
  }
  return rc;
}

int rcsh_sim_add_robot(rcsh_sim* s, const rcsh_robot_desc* r) {
  REQUIRE_SIM(s);
  if (!r) return fail(RCSH_ERR_ARG, "null robot description");
  if (s->robot.present) return fail(RCSH_ERR_STATE, "a robot is already attached to this sim");
  if (r->dof != s->narm) return fail(RCSH_ERR_MODEL, "robot dof does not match the arm chain of the scene");
  for (int i = 0; i < r->dof; ++i) {
    if (r->joint_ids[i] != i) return fail(RCSH_ERR_MODEL, "robot joints must be the arm chain in order");
    const int u = r->actuator_ids[i];
    if (u < 0 || u >= (int)s->act_slot.size() || s->act_slot[u] != i)
      return fail(RCSH_ERR_MODEL, "robot actuators must drive the arm joints one to one");
  }
  std::string why = attach_robot_frames(s->hm, s->dm, r->attachment_site, r->base_body);
  if (!why.empty()) return fail(RCSH_ERR_MODEL, why);
  int rc = upload_model(s);
  if (rc) return rc;
  s->robot.present = 1;
  s->robot.conv_registered = r->register_convergence_callback;
  s->robot.tolerance = r->joint_rotational_tolerance;
  s->robot.period = r->seconds_between_callbacks;
  std::memcpy(s->robot.tcp, r->tcp_offset, sizeof(s->robot.tcp));
  for (int i = 0; i < r->dof; ++i) s->robot.q_home[i] = r->q_home[i];
  for (int c = 0; c < r->n_collision_geoms; ++c) {
    const int g = r->collision_geom_ids[c];
    if (g < 0 || g >= s->hm.ngeom) return fail(RCSH_ERR_NAME, "arm collision geom id out of range");
    // a collision callback must not be registered on a geom the geom-geom detection cannot see (advisor, round 3): its contacts
    // with other geoms would silently never raise the flag
    for (int d : s->cgeoms_dropped)
      if (d == g) return fail(RCSH_ERR_MODEL, "arm collision geom " + std::to_string(g) + " is not in the contact table (" + s->contact_overflow + "): its geom-geom collisions would go undetected");
    for (size_t k = 0; k < s->cp.geom.size(); ++k)
      if (s->cp.geom[k] == g) s->cp_class[k] |= 1u;
    for (auto& cg : s->cgeoms)
      if (cg.geom_id == g) cg.cls |= 1;
  }
  rc = upload_coll_classes(s);
  if (!rc) rc = upload_contact_table(s);
  if (rc) return rc;
  // torque-actuated: every arm actuator a plain torque source (biastype none, zero biasprm); a mixed arm is not
  s->tq.actuated = true;
  for (int i = 0; i < s->narm; ++i)
    s->tq.actuated = s->tq.actuated && s->dm.arm_has_act[i] && !s->dm.arm_biasaffine[i] && s->dm.arm_bias[i][0] == 0.0 &&
                     s->dm.arm_bias[i][1] == 0.0 && s->dm.arm_bias[i][2] == 0.0;
  return rcsh_robot_reset(s, nullptr);  // SimRobot ctor ends with m_reset()
}

namespace {
// set_joints_hard; `reset`: on a torque-actuated robot the singular bytes of the masked environments are cleared too
int joints_hard(rcsh_sim* s, const double* q, const uint8_t* mask, bool reset) {
  int rc = scatter_host(s, field_of(s, "qpos"), s->narm, q, mask);
  if (!rc && s->tq.actuated) return torque_rest_at(s, q, mask, reset);  // (ctrl is a torque: zero, and the law's targets at q)
  if (!rc) rc = scatter_host(s, field_of(s, "ctrl"), s->narm, q, mask);
  return rc;
}
}  // namespace

int rcsh_robot_set_joints_hard(rcsh_sim* s, const double* q, const uint8_t* mask) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  return joints_hard(s, q, mask, false);
}

int rcsh_robot_reset(rcsh_sim* s, const uint8_t* mask) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  std::vector<double> q = tile(s->robot.q_home, s->narm, s->n);
  return joints_hard(s, q.data(), mask, true);
}

int rcsh_robot_set_joint_position(rcsh_sim* s, const double* q, const uint8_t* mask) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  // target := q, previous := current q, ctrl := q, is_moving := true, is_arrived := false
  std::vector<double> cur((size_t)s->n * s->narm);
  int rc = gather_host(s, field_of(s, "qpos"), s->narm, cur.data());
  if (!rc) rc = scatter_host(s, field_of(s, "target"), s->narm, q, mask);
  if (!rc) rc = scatter_host(s, field_of(s, "prevq"), s->narm, cur.data(), mask);
  if (!rc) rc = s->tq.actuated ? torque_rest_at(s, q, mask, false) : scatter_host(s, field_of(s, "ctrl"), s->narm, q, mask);
  if (!rc) rc = flags_update_host(s, kIsMoving, kIsArrived, mask);
  return rc;
}

int rcsh_robot_move_home(rcsh_sim* s, const uint8_t* mask) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  std::vector<double> q = tile(s->robot.q_home, s->narm, s->n);
  return rcsh_robot_set_joint_position(s, q.data(), mask);
}

int rcsh_robot_get_joint_position(rcsh_sim* s, double* q) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  return gather_host(s, field_of(s, "qpos"), s->narm, q);
}

int rcsh_robot_get_cartesian_position(rcsh_sim* s, double* pose) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  RunOp op{};
  op.nsteps = 0;
  op.write_obs = 1;
  op.observe_only = 1;
  op.obs = s->stage.obs;
  int rc = launch_run(s, op, false);
  if (rc) return rc;
  char* h = nullptr;
  if ((rc = pin_ready(s, h))) return rc;
  h += s->pin.obs;
  const size_t ow = (size_t)s->stage.obs_w;
  HIP_TRY(hipMemcpyAsync(h, s->stage.obs, sizeof(double) * s->n * ow, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  for (int e = 0; e < s->n; ++e) std::memcpy(pose + kPoseWidth * e, h + sizeof(double) * e * ow, kPoseWidth * sizeof(double));  // (an observation begins with the pose)
  return RCSH_OK;
}

int rcsh_robot_get_base_pose(rcsh_sim* s, double* pose) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  for (int e = 0; e < s->n; ++e) {
    double* p = pose + 7 * e;
    p[0] = s->dm.base_pos[0]; p[1] = s->dm.base_pos[1]; p[2] = s->dm.base_pos[2];
    p[3] = s->dm.base_quat[1]; p[4] = s->dm.base_quat[2]; p[5] = s->dm.base_quat[3]; p[6] = s->dm.base_quat[0];
  }
  return RCSH_OK;
}

namespace {
int launch_cartesian(rcsh_sim* s, const CartOp& op) {
  Params P = make_params(s);
  hipError_t err = hipSuccess;
  bool ok = dispatch_topology(s->narm, s->grip, [&](auto topo) {
    using T = decltype(topo);
    hipLaunchKernelGGL(k_cartesian_team<T>, dim3(((s->n + 31) / 32) * 8), dim3(64), 0, s->stream, P, op);
    err = hipGetLastError();
  });
  if (!ok) return fail(RCSH_ERR_MODEL, "no kernel instantiated for this archetype");
  if (err != hipSuccess) return fail(RCSH_ERR_DEVICE, std::string("k_cartesian launch: ") + hipGetErrorString(err));
  return RCSH_OK;
}
}  // namespace

int rcsh_robot_set_cartesian_position(rcsh_sim* s, const double* pose, const uint8_t* mask) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  if (!pose) return fail(RCSH_ERR_ARG, "null pose");
  if (s->tq.actuated) return fail(RCSH_ERR_ARG, "set_cartesian_position: the robot is torque-actuated; the CLIK commands position servos");
  const uint8_t* dm = nullptr;
  int rc = upload_mask(s, mask, &dm);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(s->stage.pose, pose, sizeof(double) * s->n * kPoseWidth, hipMemcpyHostToDevice, s->stream));
  CartOp op{};
  op.env_layer = 0;
  op.mask = dm;
  op.action = s->stage.pose;
  rc = launch_cartesian(s, op);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  return RCSH_OK;
}

namespace {
int run_ik(rcsh_sim* s, const double* pose, const double* q0, const double* tcp7, double* out, int out_width, uint8_t* success,
           int32_t* iterations, int forward) {
  const size_t n = s->n;
  const Staging& st = s->stage;
  int rc = fits(s->narm, st.q0_w, "the IK's start configuration");
  if (!rc) rc = fits(out_width, st.obs_w, "the IK's output");
  if (rc) return rc;
  double *d_pose = st.pose, *d_q0 = st.q0, *d_tcp = st.tcp, *d_out = st.obs;
  if (pose) HIP_TRY(hipMemcpyAsync(d_pose, pose, sizeof(double) * n * kPoseWidth, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(d_q0, q0, sizeof(double) * n * s->narm, hipMemcpyHostToDevice, s->stream));
  if (tcp7) HIP_TRY(hipMemcpyAsync(d_tcp, tcp7, sizeof(double) * kPoseWidth, hipMemcpyHostToDevice, s->stream));
  Params P = make_params(s);
  hipError_t err = hipSuccess;
  dispatch_topology(s->narm, s->grip, [&](auto topo) {
    using T = decltype(topo);
    if (forward)
      hipLaunchKernelGGL(k_ik<T>, dim3((s->n + 63) / 64), dim3(64), 0, s->stream, P, (const double*)d_pose, (const double*)d_q0,
                         tcp7 ? (const double*)d_tcp : (const double*)nullptr, d_out, st.flag, st.substeps, forward);
    else
      hipLaunchKernelGGL(k_ik_team<T>, dim3((s->n + 3) / 4), dim3(64), 0, s->stream, P, (const double*)d_pose, (const double*)d_q0,
                         tcp7 ? (const double*)d_tcp : (const double*)nullptr, d_out, st.flag, st.substeps);
    err = hipGetLastError();
  });
  if (err != hipSuccess) return fail(RCSH_ERR_DEVICE, std::string("k_ik launch: ") + hipGetErrorString(err));
  HIP_TRY(hipMemcpyAsync(out, d_out, sizeof(double) * n * out_width, hipMemcpyDeviceToHost, s->stream));
  if (success) HIP_TRY(hipMemcpyAsync(success, st.flag, n, hipMemcpyDeviceToHost, s->stream));
  if (iterations) HIP_TRY(hipMemcpyAsync(iterations, st.substeps, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return RCSH_OK;
}
}  // namespace

int rcsh_ik_inverse(rcsh_sim* s, const double* pose, const double* q0, const double* tcp7, double* q, uint8_t* success,
                    int32_t* iterations) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  if (!pose || !q0 || !q) return fail(RCSH_ERR_ARG, "null argument");
  return run_ik(s, pose, q0, tcp7, q, s->nl, success, iterations, 0);
}
int rcsh_ik_forward(rcsh_sim* s, const double* q0, const double* tcp7, double* pose) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  if (!q0 || !pose) return fail(RCSH_ERR_ARG, "null argument");
  return run_ik(s, nullptr, q0, tcp7, pose, kPoseWidth, nullptr, nullptr, 1);
}

// ---- collision queries on caller-supplied configurations (csrc/query_team.h)
namespace {
int query_check(rcsh_sim* s, int32_t m, int32_t kinds, const double* free_qpos) {
  if (m < 0) return fail(RCSH_ERR_ARG, "negative query count");
  if (kinds & ~kQueryKinds) return fail(RCSH_ERR_ARG, "unknown bit in the kinds mask (bit 0 floor, 1 self, 2 free body)");
  if (free_qpos && !s->box.present) return fail(RCSH_ERR_ARG, "free_qpos given in a scene without a free body");
  if (!s->cgeoms_dropped.empty()) return fail(RCSH_ERR_MODEL, "collision geoms beyond the contact table's capacity: the answer could not be exact");
  if (s->tables.chk_unchecked > 0) return fail(RCSH_ERR_MODEL, "admitted geom pairs beyond the check's table: the answer could not be exact");
  for (int g = 0; g < s->hm.ngeom; ++g) {
    // (the contact table holds capsules, boxes and convex meshes; a colliding geom of another type would be left out silently)
    const int ty = s->hm.geom_type[g];
    if (ty != 0 && ty != 3 && ty != 6 && ty != 7 && (s->hm.geom_contype[g] || s->hm.geom_conaffinity[g]))
      return fail(RCSH_ERR_MODEL, "the scene has a colliding geom of a type the collision queries do not test (mjtGeom " + std::to_string(ty) + ")");
  }
  return RCSH_OK;
}
int query_finite(const double* a, size_t n, const char* what) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(a[i])) return fail(RCSH_ERR_ARG, std::string("non-finite entry in ") + what);
  return RCSH_OK;
}
QueryArgs query_args(rcsh_sim* s, int32_t m, int32_t kinds, const QueryPairs& pairs) {
  const Params P = make_params(s);
  QueryArgs A{};
  A.links = reinterpret_cast<const LinkRec*>(reinterpret_cast<const char*>(s->d_model.get()) + sizeof(DevModel));
  A.ck = P.chk;
  A.ck.slack = nullptr;
  A.ck.pad = 0;
  A.geoms = s->d_cgeoms.get();
  A.verts = s->d_cverts.get();
  for (int k = 0; k < 3; ++k) A.plane_n[k] = s->cp.plane_n[k];
  A.plane_d = s->cp.plane_d;
  A.plane_geom = s->cp.has_plane ? s->cp.plane_geom : -1;
  A.box_geom = s->box.present ? s->hm.ngeom : -1;
  A.floor_bits = pairs.floor_bits;
  A.box_bits = pairs.box_bits;
  for (int k = 0; k < 3; ++k) A.box_size[k] = s->box.size[k];
  for (int L = 0; L < 12; ++L) {
    // (model.cpp build_self_levers: a slide's lever holds over qpos0 -+ its stroke)
    const bool slide = L < s->nl && s->dm.jtype[L] == kSlide;
    const double stroke = slide ? std::max(std::fabs(s->dm.range[L][0] - s->dm.qpos0[L]), std::fabs(s->dm.range[L][1] - s->dm.qpos0[L])) : HUGE_VAL;
    A.slide_lo[L] = slide ? s->dm.qpos0[L] - stroke : -HUGE_VAL;
    A.slide_hi[L] = slide ? s->dm.qpos0[L] + stroke : HUGE_VAL;
  }
  A.m = m;
  A.kinds = kinds;
  return A;
}
int query_launch(rcsh_sim* s, const QueryArgs& A, bool motion) {
  return team_launch(s, A.m, "collision query", [&](auto topo, dim3 grid, dim3 block) {
    using T = decltype(topo);
    if (motion) hipLaunchKernelGGL(k_motion_query<T>, grid, block, 0, s->stream, A);
    else hipLaunchKernelGGL(k_collision_query<T>, grid, block, 0, s->stream, A);
  });
}
// device pointers in: the answer for a robot without collision geometry is written without a kernel
int point_query_dev(rcsh_sim* s, const double* q, const double* free_qpos, int32_t m, int32_t kinds, uint8_t* hit, uint8_t* kinds_hit,
                    int32_t* pair) {
  if (s->cgeoms.empty()) {
    HIP_TRY(hipMemsetAsync(hit, 0, m, s->stream));
    if (kinds_hit) HIP_TRY(hipMemsetAsync(kinds_hit, 0, m, s->stream));
    if (pair) HIP_TRY(hipMemsetAsync(pair, 0xff, sizeof(int32_t) * 2 * (size_t)m, s->stream));
    return RCSH_OK;
  }
  QueryArgs A = query_args(s, m, kinds, query_pairs(s, kinds, false));
  A.q0 = q; A.free_qpos = free_qpos; A.hit = hit; A.kinds_hit = kinds_hit; A.pair = pair;
  return query_launch(s, A, false);
}
__global__ void k_query_fill(int32_t* result, double* t_contact, int m) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) { result[i] = 0; t_contact[i] = -1.0; }
}
int motion_query_dev(rcsh_sim* s, const double* q_from, const double* q_to, const double* free_qpos, int32_t m, int32_t kinds, double resolution,
                     int32_t* result, double* t_contact) {
  if (s->cgeoms.empty()) {
    hipLaunchKernelGGL(k_query_fill, dim3((m + 63) / 64), dim3(64), 0, s->stream, result, t_contact, m);
    HIP_TRY(hipGetLastError());
    return RCSH_OK;
  }
  QueryArgs A = query_args(s, m, kinds, query_pairs(s, kinds, false));
  A.q0 = q_from; A.q1 = q_to; A.free_qpos = free_qpos; A.resolution = resolution; A.result = result; A.t_contact = t_contact;
  return query_launch(s, A, true);
}
int motion_check(rcsh_sim* s, int32_t m, int32_t kinds, const double* free_qpos, double resolution) {
  if (int rc = query_check(s, m, kinds, free_qpos)) return rc;
  if (!(resolution > 0.0) || !std::isfinite(resolution)) return fail(RCSH_ERR_ARG, "resolution must be positive and finite");
  return RCSH_OK;
}
}  // namespace

int rcsh_collision_query(rcsh_sim* s, const double* q, const double* free_qpos, int32_t m, int32_t kinds, uint8_t* hit, uint8_t* kinds_hit,
                         int32_t* pair) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  int rc = query_check(s, m, kinds, free_qpos);
  if (rc) return rc;
  if (m == 0) return RCSH_OK;
  if (!q || !hit) return fail(RCSH_ERR_ARG, "null argument");
  const size_t nl = (size_t)s->nl, n = (size_t)m;
  if ((rc = query_finite(q, n * nl, "q"))) return rc;
  if (free_qpos && (rc = query_finite(free_qpos, n * kPoseWidth, "free_qpos"))) return rc;
  StageLayout L;
  const auto dq = L.in(q, n * nl), df = L.in(free_qpos, n * kPoseWidth);
  // (the kernel is handed all three outputs whatever the caller asked for, as in the clearance form)
  const auto dh = L.out_always(hit, n), dk = L.out_always(kinds_hit, n);
  const auto dp = L.out_always(pair, n * kPairWidth);
  return staged_call(s, s->d_query, L, [&](auto dev) { return point_query_dev(s, dev(dq), dev(df), m, kinds, dev(dh), dev(dk), dev(dp)); });
}
int rcsh_collision_query_dev(rcsh_sim* s, const double* q_dev, const double* free_qpos_dev, int32_t m, int32_t kinds, uint8_t* hit_dev,
                             uint8_t* kinds_hit_dev, int32_t* pair_dev) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  int rc = query_check(s, m, kinds, free_qpos_dev);
  if (rc) return rc;
  if (m == 0) return RCSH_OK;
  if (!q_dev || !hit_dev) return fail(RCSH_ERR_ARG, "null argument");
  return point_query_dev(s, q_dev, free_qpos_dev, m, kinds, hit_dev, kinds_hit_dev, pair_dev);
}
int rcsh_motion_query(rcsh_sim* s, const double* q_from, const double* q_to, const double* free_qpos, int32_t m, int32_t kinds, double resolution,
                      int32_t* result, double* t_contact) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  int rc = motion_check(s, m, kinds, free_qpos, resolution);
  if (rc) return rc;
  if (m == 0) return RCSH_OK;
  if (!q_from || !q_to || !result || !t_contact) return fail(RCSH_ERR_ARG, "null argument");
  const size_t nl = (size_t)s->nl, n = (size_t)m;
  if ((rc = query_finite(q_from, n * nl, "q_from")) || (rc = query_finite(q_to, n * nl, "q_to"))) return rc;
  if (free_qpos && (rc = query_finite(free_qpos, n * kPoseWidth, "free_qpos"))) return rc;
  StageLayout L;
  const auto da = L.in(q_from, n * nl), db = L.in(q_to, n * nl), df = L.in(free_qpos, n * kPoseWidth);
  const auto dr = L.out(result, n);
  const auto dt = L.out(t_contact, n);
  return staged_call(s, s->d_query, L, [&](auto dev) { return motion_query_dev(s, dev(da), dev(db), dev(df), m, kinds, resolution, dev(dr), dev(dt)); });
}
int rcsh_motion_query_dev(rcsh_sim* s, const double* q_from_dev, const double* q_to_dev, const double* free_qpos_dev, int32_t m, int32_t kinds,
                          double resolution, int32_t* result_dev, double* t_contact_dev) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  int rc = motion_check(s, m, kinds, free_qpos_dev, resolution);
  if (rc) return rc;
  if (m == 0) return RCSH_OK;
  if (!q_from_dev || !q_to_dev || !result_dev || !t_contact_dev) return fail(RCSH_ERR_ARG, "null argument");
  return motion_query_dev(s, q_from_dev, q_to_dev, free_qpos_dev, m, kinds, resolution, result_dev, t_contact_dev);
}

// ---- clearance queries (csrc/clearance_team.h)
namespace {
int clearance_check(rcsh_sim* s, int32_t m, int32_t kinds, const double* free_qpos, double d_max) {
  int rc = query_check(s, m, kinds, free_qpos);
  if (rc) return rc;
  if (!(d_max > 0.0)) return fail(RCSH_ERR_ARG, "d_max must be greater than 0 (+inf is allowed)");
  return RCSH_OK;
}
struct ClearOut { double* distance; uint8_t* status; int32_t* pair; double* witness; double* grad; };
// device pointers in; S non-null: the environments' own rows (m = n_envs; box_field as GuardArgs::box_field)
int clearance_dev(rcsh_sim* s, const QueryPairs& pairs, const double* q, const double* free_qpos, int32_t m, int32_t kinds, const uint8_t* pair_mask,
                  double d_max, const ClearOut& o, const double* S, int box_field) {
  if (s->cgeoms.empty()) {
    hipLaunchKernelGGL(k_clearance_fill, dim3((m + 63) / 64), dim3(64), 0, s->stream, o.distance, o.status, o.pair, o.witness, o.grad, d_max, m, s->nl);
    HIP_TRY(hipGetLastError());
    return RCSH_OK;
  }
  ClearArgs A{};
  A.Q = query_args(s, m, kinds, pairs);
  A.Q.q0 = q; A.Q.free_qpos = free_qpos;
  A.pair_mask = pair_mask; A.d_max = d_max;
  A.distance = o.distance; A.status = o.status; A.pair = o.pair; A.witness = o.witness; A.grad = o.grad;
  A.S = S; A.qpos_field = field_of(s, "qpos"); A.box_field = box_field;
  return team_launch(s, m, "clearance query", [&](auto topo, dim3 grid, dim3 block) {
    hipLaunchKernelGGL(k_clearance_query<decltype(topo)>, grid, block, 0, s->stream, A);
  });
}
// the host form of both queries: q null: the environments' own rows
int clearance_host(rcsh_sim* s, const double* q, const double* free_qpos, int32_t m, int32_t kinds, const uint8_t* pair_mask, double d_max,
                   double* distance, uint8_t* status, int32_t* pair, double* witness, double* grad, const double* S, int box_field) {
  const size_t nl = (size_t)s->nl, n = (size_t)m;
  const QueryPairs pairs = query_pairs(s, kinds, pair_mask != nullptr);
  StageLayout L;
  const auto dq = L.in(q, n * nl), df = L.in(free_qpos, n * kPoseWidth);
  const auto dm = L.in(pair_mask, (size_t)pairs.count());
  // Unlike the swept and the dynamics form, this one stages all five outputs and hands the kernel all five whatever the caller
  // asked for; only the ones asked for come back.  Handing it fewer would change the kernel's work.
  const auto dd = L.out_always(distance, n), dw = L.out_always(witness, n * kWitnessWidth), dg = L.out_always(grad, n * nl);
  const auto dp = L.out_always(pair, n * kPairWidth);
  const auto ds = L.out_always(status, n);
  return staged_call(s, s->d_query, L, [&](auto dev) {
    return clearance_dev(s, pairs, dev(dq), dev(df), m, kinds, dev(dm), d_max, ClearOut{dev(dd), dev(ds), dev(dp), dev(dw), dev(dg)}, S, box_field);
  });
}
// the free body of the environments' own rows: tested when the scene has one and `kinds` asks for it
int env_clearance_box_field(rcsh_sim* s, int32_t kinds) { return (kinds & kQueryBox) && s->box.present ? field_of(s, "box") + kBoxQ : -1; }
}  // namespace

int rcsh_clearance_pairs(rcsh_sim* s, int32_t kinds, int32_t* geom_ids, int32_t capacity, int32_t* count) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  if (!count || capacity < 0 || (capacity > 0 && !geom_ids)) return fail(RCSH_ERR_ARG, "null argument");
  int rc = query_check(s, 0, kinds, nullptr);
  if (rc) return rc;
  const QueryPairs L = query_pairs(s, kinds);
  *count = L.count();
  for (int i = 0; i < L.count() && i < capacity; ++i) { geom_ids[2 * i] = L.ids[2 * i]; geom_ids[2 * i + 1] = L.ids[2 * i + 1]; }
  return RCSH_OK;
}
int rcsh_clearance_query(rcsh_sim* s, const double* q, const double* free_qpos, int32_t m, int32_t kinds, const uint8_t* pair_mask, double d_max,
                         double* distance, uint8_t* status, int32_t* pair, double* witness, double* grad) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  int rc = clearance_check(s, m, kinds, free_qpos, d_max);
  if (rc) return rc;
  if (m == 0) return RCSH_OK;
  if (!q || !distance) return fail(RCSH_ERR_ARG, "null argument");
  if ((rc = query_finite(q, (size_t)m * s->nl, "q"))) return rc;
  if (free_qpos && (rc = query_finite(free_qpos, (size_t)m * kPoseWidth, "free_qpos"))) return rc;
  return clearance_host(s, q, free_qpos, m, kinds, pair_mask, d_max, distance, status, pair, witness, grad, nullptr, -1);
}
int rcsh_clearance_query_dev(rcsh_sim* s, const double* q_dev, const double* free_qpos_dev, int32_t m, int32_t kinds, const uint8_t* pair_mask_dev,
                             double d_max, double* distance_dev, uint8_t* status_dev, int32_t* pair_dev, double* witness_dev, double* grad_dev) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  int rc = clearance_check(s, m, kinds, free_qpos_dev, d_max);
  if (rc) return rc;
  if (m == 0) return RCSH_OK;
  if (!q_dev || !distance_dev) return fail(RCSH_ERR_ARG, "null argument");
  return clearance_dev(s, query_pairs(s, kinds, false), q_dev, free_qpos_dev, m, kinds, pair_mask_dev, d_max, ClearOut{distance_dev, status_dev, pair_dev, witness_dev, grad_dev},
                       nullptr, -1);
}
int rcsh_env_clearance(rcsh_sim* s, int32_t kinds, const uint8_t* pair_mask, double d_max, double* distance, uint8_t* status, int32_t* pair,
                       double* witness, double* grad) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  int rc = clearance_check(s, s->n, kinds, nullptr, d_max);
  if (rc) return rc;
  if (!distance) return fail(RCSH_ERR_ARG, "null argument");
  return clearance_host(s, nullptr, nullptr, s->n, kinds, pair_mask, d_max, distance, status, pair, witness, grad, s->S.get(),
                        env_clearance_box_field(s, kinds));
}
int rcsh_env_clearance_dev(rcsh_sim* s, int32_t kinds, const uint8_t* pair_mask_dev, double d_max, double* distance_dev, uint8_t* status_dev,
                           int32_t* pair_dev, double* witness_dev, double* grad_dev) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  int rc = clearance_check(s, s->n, kinds, nullptr, d_max);
  if (rc) return rc;
  if (!distance_dev) return fail(RCSH_ERR_ARG, "null argument");
  return clearance_dev(s, query_pairs(s, kinds, false), nullptr, nullptr, s->n, kinds, pair_mask_dev, d_max, ClearOut{distance_dev, status_dev, pair_dev, witness_dev, grad_dev},
                       s->S.get(), env_clearance_box_field(s, kinds));
}

// ---- swept clearance (csrc/swept_team.h)
namespace {
int swept_check(rcsh_sim* s, int32_t m, int32_t kinds, const double* free_qpos, double d_max, double tolerance, double resolution) {
  int rc = clearance_check(s, m, kinds, free_qpos, d_max);
  if (rc) return rc;
  if (!(tolerance > 0.0) || !std::isfinite(tolerance)) return fail(RCSH_ERR_ARG, "tolerance must be positive and finite");
  if (!(resolution > 0.0) || !std::isfinite(resolution)) return fail(RCSH_ERR_ARG, "resolution must be positive and finite");
  return RCSH_OK;
}
// device pointers in; S non-null: the environments' own rows are the segments' starts (m = n_envs)
int swept_dev(rcsh_sim* s, const QueryPairs& pairs, const double* q_from, const double* q_to, const double* free_qpos, int32_t m, int32_t kinds,
              const uint8_t* pair_mask, double d_max, double tolerance, double resolution, const rcsh_swept_out& o, const double* S, int box_field) {
  if (s->cgeoms.empty()) {
    hipLaunchKernelGGL(k_clearance_fill, dim3((m + 63) / 64), dim3(64), 0, s->stream, o.distance, o.status, o.pair, o.witness, o.grad, d_max, m, s->nl);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_swept_fill, dim3((m + 63) / 64), dim3(64), 0, s->stream, o.lower, o.s, o.evals, d_max, m);
    HIP_TRY(hipGetLastError());
    return RCSH_OK;
  }
  SweptArgs A{};
  A.C.Q = query_args(s, m, kinds, pairs);
  A.C.Q.q0 = q_from; A.C.Q.q1 = q_to; A.C.Q.free_qpos = free_qpos; A.C.Q.resolution = resolution;
  A.C.pair_mask = pair_mask; A.C.d_max = d_max;
  A.C.distance = o.distance; A.C.status = o.status; A.C.pair = o.pair; A.C.witness = o.witness; A.C.grad = o.grad;
  A.C.S = S; A.C.qpos_field = field_of(s, "qpos"); A.C.box_field = box_field;
  A.tolerance = tolerance; A.lower = o.lower; A.s = o.s; A.evals = o.evals;
  return team_launch(s, m, "swept clearance", [&](auto topo, dim3 grid, dim3 block) {
    hipLaunchKernelGGL(k_swept_clearance<decltype(topo)>, grid, block, 0, s->stream, A);
  });
}
// the host form of both queries: q_from null: the environments' own rows
int swept_host(rcsh_sim* s, const double* q_from, const double* q_to, const double* free_qpos, int32_t m, int32_t kinds, const uint8_t* pair_mask,
               double d_max, double tolerance, double resolution, const rcsh_swept_out& o, const double* S, int box_field) {
  const size_t nl = (size_t)s->nl, n = (size_t)m;
  const QueryPairs pairs = query_pairs(s, kinds, pair_mask != nullptr);
  StageLayout L;
  const auto da = L.in(q_from, n * nl), db = L.in(q_to, n * nl), df = L.in(free_qpos, n * kPoseWidth);
  const auto dm = L.in(pair_mask, (size_t)pairs.count());
  const auto dd = L.out(o.distance, n), dl = L.out(o.lower, n), dx = L.out(o.s, n);
  const auto dp = L.out(o.pair, n * kPairWidth);
  const auto dw = L.out(o.witness, n * kWitnessWidth), dg = L.out(o.grad, n * nl);
  const auto de = L.out(o.evals, n);
  const auto du = L.out(o.status, n);
  return staged_call(s, s->d_query, L, [&](auto dev) {
    rcsh_swept_out od{};
    od.distance = dev(dd); od.lower = dev(dl); od.s = dev(dx); od.pair = dev(dp);
    od.witness = dev(dw); od.grad = dev(dg); od.evals = dev(de); od.status = dev(du);
    return swept_dev(s, pairs, dev(da), dev(db), dev(df), m, kinds, dev(dm), d_max, tolerance, resolution, od, S, box_field);
  });
}
}  // namespace

int rcsh_swept_clearance(rcsh_sim* s, const double* q_from, const double* q_to, const double* free_qpos, int32_t m, int32_t kinds,
                         const uint8_t* pair_mask, double d_max, double tolerance, double resolution, const rcsh_swept_out* out) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  int rc = swept_check(s, m, kinds, free_qpos, d_max, tolerance, resolution);
  if (rc) return rc;
  if (m == 0) return RCSH_OK;
  if (!q_from || !q_to || !out || !out->distance) return fail(RCSH_ERR_ARG, "null argument");
  if ((rc = query_finite(q_from, (size_t)m * s->nl, "q_from")) || (rc = query_finite(q_to, (size_t)m * s->nl, "q_to"))) return rc;
  if (free_qpos && (rc = query_finite(free_qpos, (size_t)m * kPoseWidth, "free_qpos"))) return rc;
  return swept_host(s, q_from, q_to, free_qpos, m, kinds, pair_mask, d_max, tolerance, resolution, *out, nullptr, -1);
}
int rcsh_swept_clearance_dev(rcsh_sim* s, const double* q_from_dev, const double* q_to_dev, const double* free_qpos_dev, int32_t m, int32_t kinds,
                             const uint8_t* pair_mask_dev, double d_max, double tolerance, double resolution, const rcsh_swept_out* out_dev) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  int rc = swept_check(s, m, kinds, free_qpos_dev, d_max, tolerance, resolution);
  if (rc) return rc;
  if (m == 0) return RCSH_OK;
  if (!q_from_dev || !q_to_dev || !out_dev || !out_dev->distance) return fail(RCSH_ERR_ARG, "null argument");
  return swept_dev(s, query_pairs(s, kinds, false), q_from_dev, q_to_dev, free_qpos_dev, m, kinds, pair_mask_dev, d_max, tolerance, resolution, *out_dev,
                   nullptr, -1);
}
int rcsh_env_swept_clearance(rcsh_sim* s, const double* q_to, int32_t kinds, const uint8_t* pair_mask, double d_max, double tolerance,
                             double resolution, const rcsh_swept_out* out) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  int rc = swept_check(s, s->n, kinds, nullptr, d_max, tolerance, resolution);
  if (rc) return rc;
  if (!q_to || !out || !out->distance) return fail(RCSH_ERR_ARG, "null argument");
  if ((rc = query_finite(q_to, (size_t)s->n * s->nl, "q_to"))) return rc;
  return swept_host(s, nullptr, q_to, nullptr, s->n, kinds, pair_mask, d_max, tolerance, resolution, *out, s->S.get(), env_clearance_box_field(s, kinds));
}
int rcsh_env_swept_clearance_dev(rcsh_sim* s, const double* q_to_dev, int32_t kinds, const uint8_t* pair_mask_dev, double d_max, double tolerance,
                                 double resolution, const rcsh_swept_out* out_dev) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  int rc = swept_check(s, s->n, kinds, nullptr, d_max, tolerance, resolution);
  if (rc) return rc;
  if (!q_to_dev || !out_dev || !out_dev->distance) return fail(RCSH_ERR_ARG, "null argument");
  return swept_dev(s, query_pairs(s, kinds, false), nullptr, q_to_dev, nullptr, s->n, kinds, pair_mask_dev, d_max, tolerance, resolution, *out_dev,
                   s->S.get(), env_clearance_box_field(s, kinds));
}

// ---- dynamics queries (csrc/dynamics_team.h)
namespace {
// what both forms check before anything is read; fills the TCP point in the site link's frame
int dynamics_check(rcsh_sim* s, int32_t m, const double* qacc_in, const double* qfrc_in, const double* tcp7, const rcsh_dynamics_out* out,
                   double* tcp_p) {
  if (m < 0) return fail(RCSH_ERR_ARG, "negative query count");
  if (m > 0 && !out) return fail(RCSH_ERR_ARG, "null argument");
  if (out && out->qfrc_inverse && !qacc_in) return fail(RCSH_ERR_ARG, "qfrc_inverse asked for without qacc_in");
  if (out && out->qacc && !qfrc_in) return fail(RCSH_ERR_ARG, "qacc asked for without qfrc_in");
  // the pose rcsh_ik_forward reports is site * offset^-1 (quirk Q7): its origin in the site's frame is -R_offset^T t_offset
  double off[3] = {0.0, 0.0, 0.0};
  if (tcp7) {
    if (int rc = query_finite(tcp7, 7, "tcp_offset7")) return rc;
    const double n = std::sqrt(tcp7[3] * tcp7[3] + tcp7[4] * tcp7[4] + tcp7[5] * tcp7[5] + tcp7[6] * tcp7[6]);
    if (!(n > 0.0)) return fail(RCSH_ERR_ARG, "tcp_offset7 quaternion of zero norm");
    const double qn[4] = {tcp7[3] / n, tcp7[4] / n, tcp7[5] / n, tcp7[6] / n};
    double Rt[9];
    quat_to_mat(qn, Rt);
    for (int k = 0; k < 3; ++k) off[k] = -(Rt[k] * tcp7[0] + Rt[3 + k] * tcp7[1] + Rt[6 + k] * tcp7[2]);
  }
  for (int r = 0; r < 3; ++r)
    tcp_p[r] = s->dm.site_pos[r] + s->dm.site_rot[3 * r] * off[0] + s->dm.site_rot[3 * r + 1] * off[1] + s->dm.site_rot[3 * r + 2] * off[2];
  return RCSH_OK;
}
// device pointers in; S non-null: the environments' own rows (m = n_envs)
int dynamics_dev(rcsh_sim* s, const double* q, const double* qvel, const double* qacc_in, const double* qfrc_in, int32_t m, const double* tcp_p,
                 const rcsh_dynamics_out& o, const double* S) {
  DynArgs A{};
  A.links = reinterpret_cast<const LinkRec*>(reinterpret_cast<const char*>(s->d_model.get()) + sizeof(DevModel));
  A.m = m;
  A.site_link = s->dm.site_link;
  for (int k = 0; k < 3; ++k) { A.gravity[k] = s->dm.gravity[k]; A.tcp_p[k] = tcp_p[k]; }
  const double bq[4] = {s->dm.base_quat[1], s->dm.base_quat[2], s->dm.base_quat[3], s->dm.base_quat[0]};
  quat_to_mat(bq, A.base_R);
  A.q = q; A.qvel = qvel; A.qacc_in = qacc_in; A.qfrc_in = qfrc_in;
  A.o = DynOut{o.qM, o.qfrc_bias, o.gravity, o.qfrc_gravcomp, o.jac, o.qfrc_inverse, o.qacc};
  A.S = S; A.qpos_field = field_of(s, "qpos"); A.qvel_field = field_of(s, "qvel");
  return team_launch(s, m, "dynamics query", [&](auto topo, dim3 grid, dim3 block) {
    hipLaunchKernelGGL(k_dynamics_query<decltype(topo)>, grid, block, 0, s->stream, A);
  });
}
// the host form of both queries: q null: the environments' own rows
int dynamics_host(rcsh_sim* s, const double* q, const double* qvel, const double* qacc_in, const double* qfrc_in, int32_t m, const double* tcp_p,
                  const rcsh_dynamics_out& o, const double* S) {
  const size_t nl = (size_t)s->nl, n = (size_t)m, row = n * nl;
  const double* in[4] = {q, qvel, o.qfrc_inverse ? qacc_in : nullptr, o.qacc ? qfrc_in : nullptr};
  const char* names[4] = {"q", "qvel", "qacc_in", "qfrc_in"};
  for (int k = 0; k < 4; ++k)
    if (in[k])
      if (int rc = query_finite(in[k], n * nl, names[k])) return rc;
  StageLayout L;
  const auto dq = L.in(in[0], row), dv = L.in(in[1], row), da = L.in(in[2], row), df = L.in(in[3], row);
  const auto dM = L.out(o.qM, row * nl), db = L.out(o.qfrc_bias, row), dg = L.out(o.gravity, row), dc = L.out(o.qfrc_gravcomp, row);
  const auto dj = L.out(o.jac, row * kJacRows), di = L.out(o.qfrc_inverse, row), dx = L.out(o.qacc, row);
  return staged_call(s, s->d_query, L, [&](auto dev) {
    rcsh_dynamics_out od{};
    od.qM = dev(dM); od.qfrc_bias = dev(db); od.gravity = dev(dg); od.qfrc_gravcomp = dev(dc);
    od.jac = dev(dj); od.qfrc_inverse = dev(di); od.qacc = dev(dx);
    return dynamics_dev(s, dev(dq), dev(dv), dev(da), dev(df), m, tcp_p, od, S);
  });
}
}  // namespace

int rcsh_dynamics_query(rcsh_sim* s, const double* q, const double* qvel, const double* qacc_in, const double* qfrc_in, int32_t m,
                        const double* tcp_offset7, const rcsh_dynamics_out* out) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  double tcp_p[3];
  int rc = dynamics_check(s, m, qacc_in, qfrc_in, tcp_offset7, out, tcp_p);
  if (rc) return rc;
  if (m == 0) return RCSH_OK;
  if (!q) return fail(RCSH_ERR_ARG, "null argument");
  return dynamics_host(s, q, qvel, qacc_in, qfrc_in, m, tcp_p, *out, nullptr);
}
int rcsh_dynamics_query_dev(rcsh_sim* s, const double* q_dev, const double* qvel_dev, const double* qacc_in_dev, const double* qfrc_in_dev,
                            int32_t m, const double* tcp_offset7, const rcsh_dynamics_out* out_dev) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  double tcp_p[3];
  int rc = dynamics_check(s, m, qacc_in_dev, qfrc_in_dev, tcp_offset7, out_dev, tcp_p);
  if (rc) return rc;
  if (m == 0) return RCSH_OK;
  if (!q_dev) return fail(RCSH_ERR_ARG, "null argument");
  return dynamics_dev(s, q_dev, qvel_dev, qacc_in_dev, qfrc_in_dev, m, tcp_p, *out_dev, nullptr);
}
int rcsh_env_dynamics(rcsh_sim* s, const double* qacc_in, const double* qfrc_in, const double* tcp_offset7, const rcsh_dynamics_out* out) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  double tcp_p[3];
  int rc = dynamics_check(s, s->n, qacc_in, qfrc_in, tcp_offset7, out, tcp_p);
  if (rc) return rc;
  return dynamics_host(s, nullptr, nullptr, qacc_in, qfrc_in, s->n, tcp_p, *out, s->S.get());
}
int rcsh_env_dynamics_dev(rcsh_sim* s, const double* qacc_in_dev, const double* qfrc_in_dev, const double* tcp_offset7,
                          const rcsh_dynamics_out* out_dev) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  double tcp_p[3];
  int rc = dynamics_check(s, s->n, qacc_in_dev, qfrc_in_dev, tcp_offset7, out_dev, tcp_p);
  if (rc) return rc;
  return dynamics_dev(s, nullptr, nullptr, qacc_in_dev, qfrc_in_dev, s->n, tcp_p, *out_dev, s->S.get());
}

// ---- dynamics derivatives (csrc/dynamics_grad_team.h)
namespace {
// what every form checks before anything is read
int dynamics_grad_check(int32_t m, const double* qacc_in, const double* qfrc_in, const rcsh_dynamics_grad_out* out) {
  if (m < 0) return fail(RCSH_ERR_ARG, "negative query count");
  if (m > 0 && !out) return fail(RCSH_ERR_ARG, "null argument");
  if (out && out->dqfrc_inverse_dq && !qacc_in) return fail(RCSH_ERR_ARG, "dqfrc_inverse_dq asked for without qacc_in");
  if (out && (out->dqacc_dq || out->dqacc_dqvel) && !qfrc_in) return fail(RCSH_ERR_ARG, "dqacc_dq / dqacc_dqvel asked for without qfrc_in");
  return RCSH_OK;
}
// device pointers in; S non-null: the environments' own rows (m = n_envs)
int dynamics_grad_dev(rcsh_sim* s, const double* q, const double* qvel, const double* qacc_in, const double* qfrc_in, int32_t m,
                      const rcsh_dynamics_grad_out& o, const double* S) {
  DynGradArgs A{};
  A.links = reinterpret_cast<const LinkRec*>(reinterpret_cast<const char*>(s->d_model.get()) + sizeof(DevModel));
  A.m = m;
  for (int k = 0; k < 3; ++k) A.gravity[k] = s->dm.gravity[k];
  A.q = q; A.qvel = qvel; A.qacc_in = qacc_in; A.qfrc_in = qfrc_in;
  A.o = DynGradOut{o.dqfrc_inverse_dq, o.dqfrc_inverse_dqvel, o.dqacc_dq, o.dqacc_dqvel, o.qM_inv};
  A.S = S; A.qpos_field = field_of(s, "qpos"); A.qvel_field = field_of(s, "qvel");
  return team_launch(s, m, "dynamics derivatives", [&](auto topo, dim3 grid, dim3 block) {
    hipLaunchKernelGGL(k_dynamics_derivatives<decltype(topo)>, grid, block, 0, s->stream, A);
  });
}
// the host form of both: q null: the environments' own rows
int dynamics_grad_host(rcsh_sim* s, const double* q, const double* qvel, const double* qacc_in, const double* qfrc_in, int32_t m,
                       const rcsh_dynamics_grad_out& o, const double* S) {
  const size_t nl = (size_t)s->nl, n = (size_t)m, row = n * nl, mat = row * nl;
  const double* in[4] = {q, qvel, o.dqfrc_inverse_dq ? qacc_in : nullptr, o.dqacc_dq ? qfrc_in : nullptr};
  const char* names[4] = {"q", "qvel", "qacc_in", "qfrc_in"};
  for (int k = 0; k < 4; ++k)
    if (in[k])
      if (int rc = query_finite(in[k], row, names[k])) return rc;
  StageLayout L;
  const auto dq = L.in(in[0], row), dv = L.in(in[1], row), da = L.in(in[2], row), df = L.in(in[3], row);
  const auto d0 = L.out(o.dqfrc_inverse_dq, mat), d1 = L.out(o.dqfrc_inverse_dqvel, mat), d2 = L.out(o.dqacc_dq, mat);
  const auto d3 = L.out(o.dqacc_dqvel, mat), d4 = L.out(o.qM_inv, mat);
  return staged_call(s, s->d_query, L, [&](auto dev) {
    rcsh_dynamics_grad_out od{};
    od.dqfrc_inverse_dq = dev(d0); od.dqfrc_inverse_dqvel = dev(d1); od.dqacc_dq = dev(d2); od.dqacc_dqvel = dev(d3); od.qM_inv = dev(d4);
    return dynamics_grad_dev(s, dev(dq), dev(dv), dev(da), dev(df), m, od, S);
  });
}
}  // namespace

int rcsh_dynamics_derivatives(rcsh_sim* s, const double* q, const double* qvel, const double* qacc_in, const double* qfrc_in, int32_t m,
                              const rcsh_dynamics_grad_out* out) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  if (int rc = dynamics_grad_check(m, qacc_in, qfrc_in, out)) return rc;
  if (m == 0) return RCSH_OK;
  if (!q) return fail(RCSH_ERR_ARG, "null argument");
  return dynamics_grad_host(s, q, qvel, qacc_in, qfrc_in, m, *out, nullptr);
}
int rcsh_dynamics_derivatives_dev(rcsh_sim* s, const double* q_dev, const double* qvel_dev, const double* qacc_in_dev,
                                  const double* qfrc_in_dev, int32_t m, const rcsh_dynamics_grad_out* out_dev) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  if (int rc = dynamics_grad_check(m, qacc_in_dev, qfrc_in_dev, out_dev)) return rc;
  if (m == 0) return RCSH_OK;
  if (!q_dev) return fail(RCSH_ERR_ARG, "null argument");
  return dynamics_grad_dev(s, q_dev, qvel_dev, qacc_in_dev, qfrc_in_dev, m, *out_dev, nullptr);
}
int rcsh_env_dynamics_derivatives(rcsh_sim* s, const double* qacc_in, const double* qfrc_in, const rcsh_dynamics_grad_out* out) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  if (int rc = dynamics_grad_check(s->n, qacc_in, qfrc_in, out)) return rc;
  return dynamics_grad_host(s, nullptr, nullptr, qacc_in, qfrc_in, s->n, *out, s->S.get());
}
int rcsh_env_dynamics_derivatives_dev(rcsh_sim* s, const double* qacc_in_dev, const double* qfrc_in_dev,
                                      const rcsh_dynamics_grad_out* out_dev) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  if (int rc = dynamics_grad_check(s->n, qacc_in_dev, qfrc_in_dev, out_dev)) return rc;
  return dynamics_grad_dev(s, nullptr, nullptr, qacc_in_dev, qfrc_in_dev, s->n, *out_dev, s->S.get());
}

// ---- operational-space dynamics (csrc/opspace_team.h)
namespace {
struct OpsCall {
  double tcp_p[3];
  uint32_t task_mask = 0x3F;
  double damping = 0.0;
};
// what every form checks before anything is read; fills the TCP point, the mask and the damping
int opspace_check(rcsh_sim* s, int32_t m, const double* xacc_des, const rcsh_opspace_opts* opts, const rcsh_opspace_out* out, OpsCall& c) {
  if (m < 0) return fail(RCSH_ERR_ARG, "negative query count");
  if (m > 0 && !out) return fail(RCSH_ERR_ARG, "null argument");
  if (out && out->qfrc && !xacc_des) return fail(RCSH_ERR_ARG, "qfrc asked for without xacc_des");
  if (opts) {
    if (opts->task_mask == 0 || opts->task_mask > 0x3Fu) return fail(RCSH_ERR_ARG, "task_mask outside 0x01 .. 0x3F");
    if (!(opts->damping >= 0.0) || !std::isfinite(opts->damping)) return fail(RCSH_ERR_ARG, "damping negative or non-finite");
    c.task_mask = opts->task_mask;
    c.damping = opts->damping;
  }
  // the TCP of the dynamics queries for the same offset (and their errors for a bad one)
  return dynamics_check(s, 0, nullptr, nullptr, opts ? opts->tcp_offset7 : nullptr, nullptr, c.tcp_p);
}
// device pointers in; S non-null: the environments' own rows (m = n_envs)
int opspace_dev(rcsh_sim* s, const double* q, const double* qvel, const double* xacc_des, const double* qfrc_null, int32_t m, const OpsCall& c,
                const rcsh_opspace_out& o, const double* S) {
  OpsArgs A{};
  A.links = reinterpret_cast<const LinkRec*>(reinterpret_cast<const char*>(s->d_model.get()) + sizeof(DevModel));
  A.m = m;
  A.site_link = s->dm.site_link;
  A.task_mask = c.task_mask;
  A.damping = c.damping;
  A.rel_pivot = RCSH_OPSPACE_REL_PIVOT;
  for (int k = 0; k < 3; ++k) { A.gravity[k] = s->dm.gravity[k]; A.tcp_p[k] = c.tcp_p[k]; }
  const double bq[4] = {s->dm.base_quat[1], s->dm.base_quat[2], s->dm.base_quat[3], s->dm.base_quat[0]};
  quat_to_mat(bq, A.base_R);
  A.q = q; A.qvel = qvel; A.xacc_des = xacc_des; A.qfrc_null = qfrc_null;
  A.o = OpsOut{o.twist, o.jdot_qvel, o.lambda_inv, o.lambda, o.jbar, o.op_bias, o.null_proj, o.qfrc, o.status};
  A.S = S; A.qpos_field = field_of(s, "qpos"); A.qvel_field = field_of(s, "qvel");
  return team_launch(s, m, "operational-space query", [&](auto topo, dim3 grid, dim3 block) {
    hipLaunchKernelGGL(k_opspace_query<decltype(topo)>, grid, block, 0, s->stream, A);
  });
}
// the host form of both: q null: the environments' own rows
int opspace_host(rcsh_sim* s, const double* q, const double* qvel, const double* xacc_des, const double* qfrc_null, int32_t m, const OpsCall& c,
                 const rcsh_opspace_out& o, const double* S) {
  const size_t nl = (size_t)s->nl, n = (size_t)m, row = n * nl, six = n * kTaskRows;
  const double* in[4] = {q, qvel, o.qfrc ? xacc_des : nullptr, o.qfrc ? qfrc_null : nullptr};
  const size_t count[4] = {row, row, six, row};
  const char* names[4] = {"q", "qvel", "xacc_des", "qfrc_null"};
  for (int k = 0; k < 4; ++k)
    if (in[k])
      if (int rc = query_finite(in[k], count[k], names[k])) return rc;
  StageLayout L;
  const auto dq = L.in(in[0], row), dv = L.in(in[1], row), dx = L.in(in[2], six), dn = L.in(in[3], row);
  const auto d0 = L.out(o.twist, six), d1 = L.out(o.jdot_qvel, six), d2 = L.out(o.lambda_inv, six * kTaskRows), d3 = L.out(o.lambda, six * kTaskRows);
  const auto d4 = L.out(o.jbar, row * kTaskRows), d5 = L.out(o.op_bias, six), d6 = L.out(o.null_proj, row * nl), d7 = L.out(o.qfrc, row);
  const auto d8 = L.out(o.status, n);
  return staged_call(s, s->d_query, L, [&](auto dev) {
    rcsh_opspace_out od{};
    od.twist = dev(d0); od.jdot_qvel = dev(d1); od.lambda_inv = dev(d2); od.lambda = dev(d3); od.jbar = dev(d4); od.op_bias = dev(d5);
    od.null_proj = dev(d6); od.qfrc = dev(d7); od.status = dev(d8);
    return opspace_dev(s, dev(dq), dev(dv), dev(dx), dev(dn), m, c, od, S);
  });
}
}  // namespace

int rcsh_opspace_query(rcsh_sim* s, const double* q, const double* qvel, const double* xacc_des, const double* qfrc_null, int32_t m,
                       const rcsh_opspace_opts* opts, const rcsh_opspace_out* out) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  OpsCall c;
  if (int rc = opspace_check(s, m, xacc_des, opts, out, c)) return rc;
  if (m == 0) return RCSH_OK;
  if (!q) return fail(RCSH_ERR_ARG, "null argument");
  return opspace_host(s, q, qvel, xacc_des, qfrc_null, m, c, *out, nullptr);
}
int rcsh_opspace_query_dev(rcsh_sim* s, const double* q_dev, const double* qvel_dev, const double* xacc_des_dev, const double* qfrc_null_dev,
                           int32_t m, const rcsh_opspace_opts* opts, const rcsh_opspace_out* out_dev) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  OpsCall c;
  if (int rc = opspace_check(s, m, xacc_des_dev, opts, out_dev, c)) return rc;
  if (m == 0) return RCSH_OK;
  if (!q_dev) return fail(RCSH_ERR_ARG, "null argument");
  return opspace_dev(s, q_dev, qvel_dev, xacc_des_dev, qfrc_null_dev, m, c, *out_dev, nullptr);
}
int rcsh_env_opspace(rcsh_sim* s, const double* xacc_des, const double* qfrc_null, const rcsh_opspace_opts* opts, const rcsh_opspace_out* out) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  OpsCall c;
  if (int rc = opspace_check(s, s->n, xacc_des, opts, out, c)) return rc;
  return opspace_host(s, nullptr, nullptr, xacc_des, qfrc_null, s->n, c, *out, s->S.get());
}
int rcsh_env_opspace_dev(rcsh_sim* s, const double* xacc_des_dev, const double* qfrc_null_dev, const rcsh_opspace_opts* opts,
                         const rcsh_opspace_out* out_dev) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  OpsCall c;
  if (int rc = opspace_check(s, s->n, xacc_des_dev, opts, out_dev, c)) return rc;
  return opspace_dev(s, nullptr, nullptr, xacc_des_dev, qfrc_null_dev, s->n, c, *out_dev, s->S.get());
}

// ---- torque control (csrc/torque_team.h)
int rcsh_robot_is_torque_actuated(rcsh_sim* s, int32_t* yes) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  if (!yes) return fail(RCSH_ERR_ARG, "null argument");
  *yes = s->tq.actuated ? 1 : 0;
  return RCSH_OK;
}
int rcsh_robot_set_joint_torque_dev(rcsh_sim* s, const double* tau_dev, const uint8_t* mask_dev) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s); REQUIRE_TORQUE(s, "set_joint_torque");
  if (!tau_dev) return fail(RCSH_ERR_ARG, "null argument");
  hipLaunchKernelGGL(k_scatter, dim3(grid_for(s->n)), dim3(kBlock), 0, s->stream, s->S.get(), s->n, field_of(s, "ctrl"), s->narm, tau_dev, mask_dev);
  HIP_TRY(hipGetLastError());
  return RCSH_OK;
}
int rcsh_robot_set_joint_torque(rcsh_sim* s, const double* tau, const uint8_t* mask) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s); REQUIRE_TORQUE(s, "set_joint_torque");
  if (!tau) return fail(RCSH_ERR_ARG, "null argument");
  const size_t row = (size_t)s->n * s->narm;
  if (int rc = query_finite(tau, row, "tau")) return rc;
  StageLayout L;
  const auto dt = L.in(tau, row);
  const auto dk = L.in(mask, (size_t)s->n);
  return staged_call(s, s->d_query, L, [&](auto dev) { return rcsh_robot_set_joint_torque_dev(s, dev(dt), dev(dk)); });
}
int rcsh_torque_configure(rcsh_sim* s, const rcsh_torque_law* law) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  if (!law) return fail(RCSH_ERR_ARG, "null argument");
  if (const std::string why = torque_scope(s); !why.empty()) return fail(RCSH_ERR_ARG, "torque law: " + why);
  if (law->task_mask > 0x3Fu) return fail(RCSH_ERR_ARG, "task_mask above 0x3F");
  if (!(law->damping >= 0.0) || !std::isfinite(law->damping)) return fail(RCSH_ERR_ARG, "damping negative or non-finite");
  if (int rc = query_finite(law->tcp_offset7, 7, "tcp_offset7")) return rc;
  const double* o = law->tcp_offset7;
  const bool none = o[0] == 0 && o[1] == 0 && o[2] == 0 && o[3] == 0 && o[4] == 0 && o[5] == 0 && o[6] == 0;
  if (!none && !(o[3] * o[3] + o[4] * o[4] + o[5] * o[5] + o[6] * o[6] > 0.0)) return fail(RCSH_ERR_ARG, "tcp_offset7 quaternion of zero norm");
  for (int r = 0; r < kTaskRows; ++r)
    if (!(law->task_k[r] >= 0.0) || !(law->task_d[r] >= 0.0) || !std::isfinite(law->task_k[r]) || !std::isfinite(law->task_d[r]))
      return fail(RCSH_ERR_ARG, "task gain negative or non-finite");
  for (int i = 0; i < s->narm; ++i)
    if (!(law->joint_k[i] >= 0.0) || !(law->joint_d[i] >= 0.0) || !std::isfinite(law->joint_k[i]) || !std::isfinite(law->joint_d[i]))
      return fail(RCSH_ERR_ARG, "joint gain negative or non-finite");
  if (int rc = torque_buffers(s)) return rc;
  s->tq.law = *law;
  return RCSH_OK;
}
int rcsh_torque_set_target_dev(rcsh_sim* s, const double* pose7_dev, const double* q_des_dev, const uint8_t* mask_dev) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s); REQUIRE_TORQUE(s, "torque target");
  return torque_target_dev(s, pose7_dev, q_des_dev, mask_dev);
}
int rcsh_torque_set_target(rcsh_sim* s, const double* pose7, const double* q_des, const uint8_t* mask) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s); REQUIRE_TORQUE(s, "torque target");
  const size_t n = (size_t)s->n;
  if (pose7) {
    if (int rc = query_finite(pose7, n * kTorquePose, "pose7")) return rc;
    for (size_t e = 0; e < n; ++e) {
      const double* q = pose7 + e * kTorquePose + 3;
      if ((!mask || mask[e]) && !(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] > 0.0)) return fail(RCSH_ERR_ARG, "pose7 quaternion of zero norm");
    }
  }
  if (q_des)
    if (int rc = query_finite(q_des, n * s->narm, "q_des")) return rc;
  StageLayout L;
  const auto dp = L.in(pose7, n * kTorquePose), dq = L.in(q_des, n * (size_t)s->narm);
  const auto dk = L.in(mask, n);
  return staged_call(s, s->d_query, L, [&](auto dev) { return torque_target_dev(s, dev(dp), dev(dq), dev(dk)); });
}
int rcsh_torque_get_target(rcsh_sim* s, double* pose7, double* q_des) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s); REQUIRE_TORQUE(s, "torque target");
  if (int rc = torque_buffers(s)) return rc;
  const size_t n = (size_t)s->n, w = (size_t)(kTorquePose + s->narm);
  std::vector<double> t(w * n);
  HIP_TRY(hipMemcpyAsync(t.data(), s->tq.target.get(), sizeof(double) * w * n, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  for (size_t e = 0; e < n; ++e) {
    if (pose7) for (int k = 0; k < kTorquePose; ++k) pose7[e * kTorquePose + k] = t[(size_t)k * n + e];
    if (q_des) for (int i = 0; i < s->narm; ++i) q_des[e * s->narm + i] = t[(size_t)(kTorquePose + i) * n + e];
  }
  return RCSH_OK;
}
int rcsh_torque_status(rcsh_sim* s, uint8_t* singular) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s); REQUIRE_TORQUE(s, "torque status");
  if (!singular) return fail(RCSH_ERR_ARG, "null argument");
  if (int rc = torque_buffers(s)) return rc;
  HIP_TRY(hipMemcpyAsync(singular, s->tq.singular.get(), s->n, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return RCSH_OK;
}
int rcsh_sim_step_torque(rcsh_sim* s, int64_t k) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  if (const std::string why = torque_scope(s); !why.empty()) return fail(RCSH_ERR_ARG, "step_torque: " + why);
  if (k < 0 || k > 0x7fffffff) return fail(RCSH_ERR_ARG, "step count must be non-negative");
  if (int rc = torque_buffers(s)) return rc;
  if (k > 0) {
    const TorqueArgs A = torque_args(s, s->tq.law, (int32_t)k);
    bool launched = false;
    int rc = team_launch(s, s->n, "step_torque", [&](auto topo, dim3 grid, dim3 block) {
      using T = decltype(topo);
      if (!s->dm.has_friction) {
        hipLaunchKernelGGL((k_run_torque<T, false>), grid, block, 0, s->stream, A);
        launched = true;
      } else if constexpr (T::NARM == 7 && !T::GRIP) {
        hipLaunchKernelGGL((k_run_torque<T, true>), grid, block, 0, s->stream, A);
        launched = true;
      }
    });
    if (rc) return rc;
    if (!launched) return fail(RCSH_ERR_MODEL, "step_torque: no kernel instantiated for this archetype with dry joint friction");
    // the end-of-launch check for contacts nobody resolves, at the handle's cadence: the zero-substep launch that asks for it alone
    if (s->contact_check && s->check_every > 0 && (s->check_seq++ % s->check_every) == 0) {
      RunOp op{};
      op.nsteps = 0;
      op.observe_only = 1;
      op.check = 1;
      if ((rc = launch_run(s, op, false))) return rc;
    }
  }
  HIP_TRY(hipStreamSynchronize(s->stream));
  return RCSH_OK;
}

int rcsh_robot_get_state(rcsh_sim* s, uint8_t* ik_success, uint8_t* collision, uint8_t* is_moving, uint8_t* is_arrived,
                         double* previous_angles, double* target_angles) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  int rc = flag_host(s, kIkSuccess, ik_success);
  if (!rc) rc = flag_host(s, kRobotCollision, collision);
  if (!rc) rc = flag_host(s, kIsMoving, is_moving);
  if (!rc) rc = flag_host(s, kIsArrived, is_arrived);
  if (!rc && previous_angles) rc = gather_host(s, field_of(s, "prevq"), s->narm, previous_angles);
  if (!rc && target_angles) rc = gather_host(s, field_of(s, "target"), s->narm, target_angles);
  return rc;
}

int rcsh_sim_add_gripper(rcsh_sim* s, const rcsh_gripper_desc* g) {
  REQUIRE_SIM(s);
  if (!g) return fail(RCSH_ERR_ARG, "null gripper description");
  if (!s->grip) return fail(RCSH_ERR_MODEL, "scene has no two-finger gripper");
  if (s->gripcfg.present) return fail(RCSH_ERR_STATE, "a gripper is already attached to this sim");
  if (g->joint_id != s->narm && g->joint_id != s->narm + 1) return fail(RCSH_ERR_MODEL, "gripper joint must be a finger joint");
  if (g->actuator_id < 0 || g->actuator_id >= (int)s->act_slot.size() || s->act_slot[g->actuator_id] != s->narm)
    return fail(RCSH_ERR_MODEL, "gripper actuator must be the finger tendon actuator");
  s->gripcfg.present = 1;
  s->gripcfg.finger = g->joint_id - s->narm;
  s->gripcfg.eps_inner = g->epsilon_inner; s->gripcfg.eps_outer = g->epsilon_outer;
  s->gripcfg.period = g->seconds_between_callbacks;
  s->gripcfg.max_act = g->max_actuator_width; s->gripcfg.min_act = g->min_actuator_width;
  s->gripcfg.max_joint = g->max_joint_width; s->gripcfg.min_joint = g->min_joint_width;
  // SimGripper::collision_callback (SimGripper.cpp:108-130) on plane contacts {geom[0] = plane, geom[1] = robot geom}:
  // counted when geom[1] is a gripper collision geom and not in the ignore list (the finger-finger skip cannot
  // apply: the plane is no finger geom; the ignore test reads geom[1] twice, reference quirk Q6 -- same set here)
  for (int c = 0; c < g->n_collision_geoms; ++c) {
    const int gid = g->collision_geom_ids[c];
    if (gid < 0 || gid >= s->hm.ngeom) return fail(RCSH_ERR_NAME, "gripper collision geom id out of range");
    for (int d : s->cgeoms_dropped)
      if (d == gid) return fail(RCSH_ERR_MODEL, "gripper collision geom " + std::to_string(gid) + " is not in the contact table (" + s->contact_overflow + "): its geom-geom collisions would go undetected");
    for (auto& cg : s->cgeoms)
      if (cg.geom_id == gid) cg.cls |= 16;
    bool ignored = false;
    for (int q = 0; q < g->n_ignored_geoms; ++q) ignored = ignored || g->ignored_geom_ids[q] == gid;
    if (ignored) continue;
    for (size_t k = 0; k < s->cp.geom.size(); ++k)
      if (s->cp.geom[k] == gid) s->cp_class[k] |= 2u;
    for (auto& cg : s->cgeoms)
      if (cg.geom_id == gid) cg.cls |= 2;
  }
  for (int c = 0; c < g->n_finger_geoms; ++c)
    for (auto& cg : s->cgeoms)
      if (cg.geom_id == g->finger_geom_ids[c]) cg.cls |= 4;
  for (int q = 0; q < g->n_ignored_geoms; ++q)
    for (auto& cg : s->cgeoms)
      if (cg.geom_id == g->ignored_geom_ids[q]) cg.cls |= 8;
  {
    int rc = upload_coll_classes(s);
    if (!rc) rc = upload_contact_table(s);
    if (rc) return rc;
  }
  return rcsh_gripper_reset(s, nullptr);  // SimGripper ctor ends with m_reset()
}

int rcsh_gripper_reset(rcsh_sim* s, const uint8_t* mask) {
  REQUIRE_SIM(s); REQUIRE_GRIPPER(s);
  std::vector<double> z((size_t)s->n * 2, 0.0);
  std::vector<double> qj((size_t)s->n, s->gripcfg.max_joint), ca((size_t)s->n, s->gripcfg.max_act);
  int rc = scatter_host(s, field_of(s, "grip"), 2, z.data(), mask);
  if (!rc) rc = scatter_host(s, field_of(s, "qpos") + s->narm + s->gripcfg.finger, 1, qj.data(), mask);
  if (!rc) rc = scatter_host(s, field_of(s, "ctrl") + s->narm, 1, ca.data(), mask);
  if (!rc) rc = flags_update_host(s, 0, kGripMoving | kGripCollision, mask);
  return rc;
}

int rcsh_gripper_set_normalized_width(rcsh_sim* s, const double* width, double force, const uint8_t* mask) {
  REQUIRE_SIM(s); REQUIRE_GRIPPER(s);
  if (force < 0) return fail(RCSH_ERR_ARG, "width must be between 0 and 1, force must be positive");
  std::vector<double> c((size_t)s->n);
  for (int e = 0; e < s->n; ++e) {
    if (mask && !mask[e]) continue;
    if (width[e] < 0 || width[e] > 1) return fail(RCSH_ERR_ARG, "width must be between 0 and 1, force must be positive");
    c[e] = width[e] * (s->gripcfg.max_act - s->gripcfg.min_act) + s->gripcfg.min_act;
  }
  int rc = scatter_host(s, field_of(s, "grip"), 1, width, mask);
  if (!rc) rc = scatter_host(s, field_of(s, "ctrl") + s->narm, 1, c.data(), mask);
  return rc;
}

int rcsh_gripper_get_normalized_width(rcsh_sim* s, double* width) {
  REQUIRE_SIM(s); REQUIRE_GRIPPER(s);
  int rc = gather_host(s, field_of(s, "qpos") + s->narm + s->gripcfg.finger, 1, width);
  if (rc) return rc;
  for (int e = 0; e < s->n; ++e) {
    double w = (width[e] - s->gripcfg.min_joint) / (s->gripcfg.max_joint - s->gripcfg.min_joint);
    width[e] = w < 0 ? 0 : (w > 1 ? 1 : w);
  }
  return RCSH_OK;
}

int rcsh_gripper_is_grasped(rcsh_sim* s, uint8_t* grasped) {
  REQUIRE_SIM(s); REQUIRE_GRIPPER(s);
  std::vector<double> w(s->n), st((size_t)s->n * 2);
  int rc = rcsh_gripper_get_normalized_width(s, w.data());
  if (!rc) rc = gather_host(s, field_of(s, "grip"), 2, st.data());
  if (rc) return rc;
  for (int e = 0; e < s->n; ++e) {
    const double lc = st[2 * e];
    grasped[e] = (lc - s->gripcfg.eps_inner < w[e]) && (w[e] < lc + s->gripcfg.eps_outer);
  }
  return RCSH_OK;
}

int rcsh_gripper_get_state(rcsh_sim* s, double* last_commanded_width, uint8_t* is_moving, double* last_width, uint8_t* collision) {
  REQUIRE_SIM(s); REQUIRE_GRIPPER(s);
  std::vector<double> st((size_t)s->n * 2);
  int rc = gather_host(s, field_of(s, "grip"), 2, st.data());
  if (rc) return rc;
  for (int e = 0; e < s->n; ++e) {
    if (last_commanded_width) last_commanded_width[e] = st[2 * e];
    if (last_width) last_width[e] = st[2 * e + 1];
  }
  rc = flag_host(s, kGripMoving, is_moving);
  if (!rc) rc = flag_host(s, kGripCollision, collision);
  return rc;
}

int rcsh_sim_get_qpos(rcsh_sim* s, double* q) { REQUIRE_SIM(s); return gather_host(s, field_of(s, "qpos"), s->nl, q); }
int rcsh_sim_get_qvel(rcsh_sim* s, double* q) { REQUIRE_SIM(s); return gather_host(s, field_of(s, "qvel"), s->nl, q); }
int rcsh_sim_get_time(rcsh_sim* s, double* t) { REQUIRE_SIM(s); return gather_host(s, field_of(s, "time"), 1, t); }
int rcsh_sim_get_ctrl(rcsh_sim* s, double* c) {
  REQUIRE_SIM(s);
  std::vector<double> slots((size_t)s->n * s->nu);
  int rc = gather_host(s, field_of(s, "ctrl"), s->nu, slots.data());
  if (rc) return rc;
  const int nu = (int)s->act_slot.size();
  for (int e = 0; e < s->n; ++e)
    for (int u = 0; u < nu; ++u) c[(size_t)e * nu + u] = slots[(size_t)e * s->nu + s->act_slot[u]];
  return RCSH_OK;
}
int rcsh_sim_set_qpos(rcsh_sim* s, const double* q, const uint8_t* mask) { REQUIRE_SIM(s); return scatter_host(s, field_of(s, "qpos"), s->nl, q, mask); }
int rcsh_sim_set_qvel(rcsh_sim* s, const double* q, const uint8_t* mask) { REQUIRE_SIM(s); return scatter_host(s, field_of(s, "qvel"), s->nl, q, mask); }

// ---- free box of the scene (reference: mjData.joint("box_joint").qpos, python/rcs/envs/sim.py:379-383,399,412)
int rcsh_sim_add_free_box(rcsh_sim* s, const rcsh_free_box_desc* d) {
  REQUIRE_SIM(s);
  if (!d) return fail(RCSH_ERR_ARG, "null free-box description");
  if (s->box.present) return fail(RCSH_ERR_STATE, "a free box is already attached to this sim");
  if (!(s->narm == 7 && (s->grip || s->dm.has_friction != 0)))
    return fail(RCSH_ERR_MODEL, "free bodies are compiled for three archetypes: 7-dof arm + two-finger gripper without dry joint friction (FR3) "
                                "and with it (xArm7 + gripper), 7-dof arm without gripper with it (xArm7)");
  if (s->grip && s->dm.has_friction && !d->resolve_robot_contacts)
    return fail(RCSH_ERR_MODEL, "7-dof arm + gripper with dry joint friction next to a free body: compiled with robot contacts resolved only");
  if (s->dm.has_friction && d->noslip_iterations > 0)
    return fail(RCSH_ERR_MODEL, "the noslip pass over dry joint friction rows is not built: scenes with frictionloss need noslip_iterations = 0");
  if (!d->cone_elliptic) return fail(RCSH_ERR_MODEL, "contacts use elliptic friction cones (option cone=\"elliptic\")");
  if (!(d->mass > 0) || !(d->inertia[0] > 0) || !(d->inertia[1] > 0) || !(d->inertia[2] > 0) || !(d->impratio > 0))
    return fail(RCSH_ERR_ARG, "free box: mass, inertia and impratio must be positive");
  BoxCfg b{};
  b.present = 1;
  b.noslip_iterations = d->noslip_iterations;
  for (int k = 0; k < 7; ++k) b.qpos0[k] = d->qpos0[k];
  b.mass = d->mass; b.inv_mass = 1.0 / d->mass;
  for (int k = 0; k < 3; ++k) { b.inertia[k] = d->inertia[k]; b.inv_inertia[k] = 1.0 / d->inertia[k]; b.size[k] = d->size[k]; }
  b.fr = d->friction[0];
  b.geom_mu = d->geom_friction[0] > 0 ? d->geom_friction[0] : d->friction[0];
  // contacts of the robot's geoms with the floor and the box enter one constraint problem with the robot's own rows
  // (limit / equality rows; dry-friction rows in the xArm7 + gripper archetype)
  b.resolve = (d->resolve_robot_contacts && s->grip && !s->cgeoms.empty()) ? (1 | (d->resolve_robot_contacts & 2)) : 0;  // (bit 1: self contact too)
  if (b.resolve && !s->contact_overflow.empty()) return fail(RCSH_ERR_MODEL, "robot contacts cannot be resolved in this scene: " + s->contact_overflow);
  make_kb(d->solref, d->solimp, s->dm.timestep, b.K, b.B);
  b.imp = make_imp(d->solimp);
  b.inv_impratio = 1.0 / d->impratio;
  b.plane_z = d->plane_z;
  // mjModel.stat.meaninertia: mean diagonal of M(qpos0) over all dofs of the scene
  const int nv = s->nl + 6;
  const double meaninertia = (s->dm.inertia_diag_sum + 3 * d->mass + d->inertia[0] + d->inertia[1] + d->inertia[2]) / nv;
  b.scale = 1.0 / (meaninertia * nv);
  b.noslip_tolerance = d->noslip_tolerance;
  s->box = b;
  if (int rc = upload_boxtask(s)) return rc;
  if (int rc = upload_contact_table(s)) return rc;
  return rcsh_sim_reset_free_box(s);
}
int rcsh_sim_set_contact_options(rcsh_sim* s, const rcsh_contact_options* o) {
  REQUIRE_SIM(s);
  if (!o) return fail(RCSH_ERR_ARG, "null contact options");
  if (s->box.present) return fail(RCSH_ERR_STATE, "this scene has a free box: its description (rcsh_sim_add_free_box) carries the contact options");
  // (whenever the option is switched -- off, on, or between its forms -- the escalation masks, their counters and the phantom box's warm
  // start begin empty: stale bits of a rollout under another option would send environments to a launch that no longer knows them;
  // advisor, round 5)
  if (s->esc.mask) {
    const size_t nw = ((size_t)s->n + 63) / 64;
    HIP_TRY(hipMemsetAsync(s->esc.mask.get(), 0, sizeof(uint64_t) * kEscRows * nw, s->stream));
    HIP_TRY(hipMemsetAsync(s->esc.ctr.get(), 0, sizeof(uint32_t) * 4, s->stream));
    int f_box = -1;
    dispatch_topology(s->narm, s->grip, [&](auto topo) { f_box = (int)Lay<decltype(topo)>::BOX; });
    if (f_box >= 0) HIP_TRY(hipMemsetAsync(s->S.get() + (size_t)(f_box + kBoxX) * s->n, 0, sizeof(double) * (size_t)(kBoxState - kBoxX) * s->n, s->stream));
    if (int rc = void_remembered_gaps(s)) return rc;
  }
  if (!o->resolve_robot_contacts) { s->box = BoxCfg{}; s->esc_mode = false; return RCSH_OK; }
  if (!(s->narm == 7 && s->grip && !s->dm.has_friction)) return fail(RCSH_ERR_MODEL, "contacts of the robot's geoms are resolved for the FR3 + hand archetype (no dry joint friction)");
  if (!o->cone_elliptic) return fail(RCSH_ERR_MODEL, "contacts use elliptic friction cones (option cone=\"elliptic\")");
  if (!(o->impratio > 0)) return fail(RCSH_ERR_ARG, "impratio must be positive");
  if (!s->contact_overflow.empty()) return fail(RCSH_ERR_MODEL, "robot contacts cannot be resolved in this scene: " + s->contact_overflow);
  if (s->cgeoms.empty() || !s->cp.has_plane) return RCSH_OK;  // nothing the robot could touch
  // the phantom box of the contact phase: unit inertia, zero size, parked 1 km above the scene
  BoxCfg b{};
  b.present = 0;
  b.resolve = 1 | (o->resolve_robot_contacts & 2);  // (bit 1: contacts between two geoms of the robot too)
  const bool esc_mode = (o->resolve_robot_contacts & 4) != 0;  // (bit 2: environment by environment instead of the whole batch)
  // what the option needs and the handle does not have yet is built here and attached below, with the option itself: the six
  // escalation buffers as one group, the slack record as another
  rcsh_sim::EscBufs esc;
  DevBuf<float> slack;
  if (esc_mode && !s->esc.mask) {
    const size_t nw = ((size_t)s->n + 63) / 64;
    HIP_TRY(hipMalloc(esc.mask.out(), sizeof(uint64_t) * kEscRows * nw));
    HIP_TRY(hipMalloc(esc.ctr.out(), sizeof(uint32_t) * 4));
    HIP_TRY(hipMalloc(esc.snap.out(), sizeof(double) * (size_t)(s->nfields + kMaxRateCams) * s->n));  // (+ the rate-driven cameras' clocks)
    HIP_TRY(hipMalloc(esc.snap_flags.out(), sizeof(uint32_t) * s->n));
    HIP_TRY(hipMalloc(esc.snap_conv.out(), sizeof(int32_t) * s->n));
    HIP_TRY(hipMalloc(esc.trace.out(), sizeof(double) * (size_t)kEscTraceCap * s->nl * s->n));
    HIP_TRY(hipMemsetAsync(esc.mask.get(), 0, sizeof(uint64_t) * kEscRows * nw, s->stream));
    HIP_TRY(hipMemsetAsync(esc.ctr.get(), 0, sizeof(uint32_t) * 4, s->stream));
    HIP_TRY(hipMemsetAsync(esc.snap.get(), 0, sizeof(double) * (size_t)(s->nfields + kMaxRateCams) * s->n, s->stream));
  }
  if ((b.resolve & 2) && !s->d_slack) {
    HIP_TRY(hipMalloc(slack.out(), sizeof(float) * (size_t)kSlackStride * s->n));
    HIP_TRY(hipMemsetAsync(slack.get(), 0, sizeof(float) * (size_t)kSlackStride * s->n, s->stream));  // (no gap known: every pair is looked at)
  }
  b.noslip_iterations = o->noslip_iterations;
  b.qpos0[2] = 1000.0; b.qpos0[3] = 1.0;
  b.mass = b.inv_mass = 1.0;
  for (int k = 0; k < 3; ++k) { b.inertia[k] = b.inv_inertia[k] = 1.0; b.size[k] = 0.0; }
  b.fr = b.geom_mu = 1.0;
  make_kb(o->solref, o->solimp, s->dm.timestep, b.K, b.B);
  b.imp = make_imp(o->solimp);
  b.inv_impratio = 1.0 / o->impratio;
  b.plane_z = s->cp.plane_d;
  b.scale = 1.0 / (s->dm.inertia_diag_sum / s->nl * s->nl);  // 1 / (meaninertia * nv)
  b.noslip_tolerance = o->noslip_tolerance;
  // the last allocation is behind: the option and its buffers are attached together (the two uploads below read them from the handle)
  if (esc.mask) {
    s->esc = std::move(esc);
    if (const char* e = std::getenv("RCSH_CONV_CHUNK")) s->conv_chunk = std::atoi(e);
  }
  if (slack) s->d_slack = std::move(slack);
  s->esc_mode = esc_mode;
  s->box = b;
  if (int rc = upload_boxtask(s)) return rc;
  return upload_contact_table(s);
}
int rcsh_sim_contact_unresolved(rcsh_sim* s, uint8_t* unresolved) {
  REQUIRE_SIM(s);
  if (s->contact_check && s->check_every != 1) {
    // the handle checks less often than every launch: check the present state now, so that the answer is up to date
    RunOp op{};
    op.nsteps = 0;
    op.observe_only = 1;
    op.check = 1;
    if (int rc = launch_run(s, op, false)) return rc;
  }
  return flag_host(s, kContactUnresolved, unresolved);
}
int rcsh_sim_contact_overflow(rcsh_sim* s, uint8_t* overflow) {
  REQUIRE_SIM(s);
  return flag_host(s, kContactOverflow, overflow);
}
int rcsh_sim_contact_escalated(rcsh_sim* s, uint8_t* now, uint8_t* ever) {
  REQUIRE_SIM(s);
  if (now) {
    std::memset(now, 0, s->n);
    if (s->esc_mode && s->esc.mask) {
      const size_t nw = ((size_t)s->n + 63) / 64;
      std::vector<uint64_t> w(nw);
      HIP_TRY(hipMemcpyAsync(w.data(), s->esc.mask.get(), sizeof(uint64_t) * nw, hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipStreamSynchronize(s->stream));
      for (int e = 0; e < s->n; ++e) now[e] = (uint8_t)((w[e >> 6] >> (e & 63)) & 1u);
    }
  }
  return flag_host(s, kContactResolved, ever);
}
int rcsh_sim_set_contact_check(rcsh_sim* s, int32_t every) {
  REQUIRE_SIM(s);
  if (every < 0) return fail(RCSH_ERR_ARG, "contact check cadence must be >= 0 (0: off, 1: every stepping launch)");
  s->check_every = every;
  s->check_seq = 0;
  return RCSH_OK;
}
int rcsh_sim_contact_check_unchecked_pairs(rcsh_sim* s, int32_t* count) {
  REQUIRE_SIM(s);
  if (!count) return fail(RCSH_ERR_ARG, "count is null");
  *count = s->tables.chk_unchecked;
  return RCSH_OK;
}
int rcsh_sim_contact_table_dropped(rcsh_sim* s, int32_t* geom_ids, int32_t capacity, int32_t* count, char* reason, size_t reason_capacity) {
  REQUIRE_SIM(s);
  if (count) *count = (int32_t)s->cgeoms_dropped.size();
  for (int i = 0; geom_ids && i < capacity && i < (int)s->cgeoms_dropped.size(); ++i) geom_ids[i] = s->cgeoms_dropped[i];
  if (reason && reason_capacity > 0) {
    std::strncpy(reason, s->contact_overflow.c_str(), reason_capacity - 1);
    reason[reason_capacity - 1] = 0;
  }
  return RCSH_OK;
}

int rcsh_sim_reset_free_box(rcsh_sim* s) {
  REQUIRE_SIM(s);
  if (!s->box.present) return fail(RCSH_ERR_STATE, "no free box attached: call rcsh_sim_add_free_box first");
  std::vector<double> b0((size_t)s->n * kBoxState, 0.0);
  for (int e = 0; e < s->n; ++e)
    for (int k = 0; k < 7; ++k) b0[(size_t)e * kBoxState + k] = b0[(size_t)e * kBoxState + kBoxPre + k] = s->box.qpos0[k];
  return scatter_host(s, field_of(s, "box"), kBoxState, b0.data(), nullptr);
}
#define REQUIRE_BOX(s) \
  if (!(s)->box.present) return fail(RCSH_ERR_STATE, "no free box attached: call rcsh_sim_add_free_box first")
int rcsh_sim_get_free_qpos(rcsh_sim* s, double* q) { REQUIRE_SIM(s); REQUIRE_BOX(s); return gather_host(s, field_of(s, "box") + kBoxQ, 7, q); }
int rcsh_sim_get_free_qvel(rcsh_sim* s, double* v) { REQUIRE_SIM(s); REQUIRE_BOX(s); return gather_host(s, field_of(s, "box") + kBoxV, 6, v); }
int rcsh_sim_set_free_qpos(rcsh_sim* s, const double* q, const uint8_t* mask) { REQUIRE_SIM(s); REQUIRE_BOX(s); return scatter_host(s, field_of(s, "box") + kBoxQ, 7, q, mask); }
int rcsh_sim_set_free_qvel(rcsh_sim* s, const double* v, const uint8_t* mask) { REQUIRE_SIM(s); REQUIRE_BOX(s); return scatter_host(s, field_of(s, "box") + kBoxV, 6, v, mask); }

// (the blob begins with a header -- a magic word with the layout's version, n_envs, the number of state fields: a blob of another
// build or handle is refused by what it says, not only when its size happens to differ; advisor, round 5)
constexpr size_t kStateHeader = 16;
constexpr char kStateMagic[8] = {'R', 'C', 'S', 'H', 'S', 'T', '0', '2'};
size_t rcsh_sim_state_bytes(const rcsh_sim* s) {
  if (!s) return 0;
  // (the tail: which environments are on the contact-resolving kernel -- per-environment escalation; a replay from a snapshot takes
  // the same kernels environment by environment as the rollout it was taken from)
  return kStateHeader + (size_t)s->n * (sizeof(double) * s->nfields + sizeof(uint32_t) + sizeof(int32_t)) + sizeof(uint64_t) * (((size_t)s->n + 63) / 64);
}
int rcsh_sim_get_state(rcsh_sim* s, void* blob) {
  REQUIRE_SIM(s);
  if (!blob) return fail(RCSH_ERR_ARG, "null state blob");
  char* b = static_cast<char*>(blob);
  {
    const uint32_t hn = (uint32_t)s->n, hf = (uint32_t)s->nfields;
    std::memcpy(b, kStateMagic, 8); std::memcpy(b + 8, &hn, 4); std::memcpy(b + 12, &hf, 4);
    b += kStateHeader;
  }
  const size_t ns = sizeof(double) * (size_t)s->n * s->nfields, nf = sizeof(uint32_t) * (size_t)s->n, nc = sizeof(int32_t) * (size_t)s->n;
  HIP_TRY(hipMemcpyAsync(b, s->S.get(), ns, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(b + ns, s->flags.get(), nf, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipMemcpyAsync(b + ns + nf, s->conv.get(), nc, hipMemcpyDeviceToHost, s->stream));
  const size_t ne = sizeof(uint64_t) * (((size_t)s->n + 63) / 64);
  if (s->esc.mask) HIP_TRY(hipMemcpyAsync(b + ns + nf + nc, s->esc.mask.get(), ne, hipMemcpyDeviceToHost, s->stream));
  else std::memset(b + ns + nf + nc, 0, ne);
  HIP_TRY(hipStreamSynchronize(s->stream));
  return RCSH_OK;
}
int rcsh_sim_set_state(rcsh_sim* s, const void* blob) {
  REQUIRE_SIM(s);
  if (!blob) return fail(RCSH_ERR_ARG, "null state blob");
  const char* b = static_cast<const char*>(blob);
  {
    uint32_t hn = 0, hf = 0;
    std::memcpy(&hn, b + 8, 4); std::memcpy(&hf, b + 12, 4);
    if (std::memcmp(b, kStateMagic, 8) != 0 || hn != (uint32_t)s->n || hf != (uint32_t)s->nfields)
      return fail(RCSH_ERR_ARG, "state blob of another layout (taken by another build, or from a handle with another scene / n_envs)");
    b += kStateHeader;
  }
  const size_t ns = sizeof(double) * (size_t)s->n * s->nfields, nf = sizeof(uint32_t) * (size_t)s->n, nc = sizeof(int32_t) * (size_t)s->n;
  if (int rc = void_remembered_gaps(s)) return rc;
  HIP_TRY(hipMemcpyAsync(s->S.get(), b, ns, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(s->flags.get(), b + ns, nf, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(s->conv.get(), b + ns + nf, nc, hipMemcpyHostToDevice, s->stream));
  if (s->esc.mask) {
    const size_t ne = sizeof(uint64_t) * (((size_t)s->n + 63) / 64);
    HIP_TRY(hipMemcpyAsync(s->esc.mask.get(), b + ns + nf + nc, ne, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemsetAsync(s->esc.mask.get() + ne / sizeof(uint64_t), 0, (kEscRows - 1) * ne, s->stream));
    uint32_t ctr[4] = {0, 0, 0, 0};  // (RunOp::esc_ctr[1]: how many are escalated)
    const uint64_t* w = reinterpret_cast<const uint64_t*>(b + ns + nf + nc);
    for (size_t i = 0; i < ne / sizeof(uint64_t); ++i) { uint64_t v; std::memcpy(&v, w + i, sizeof(v)); ctr[1] += (uint32_t)__builtin_popcountll(v); }
    HIP_TRY(hipMemcpyAsync(s->esc.ctr.get(), ctr, sizeof(ctr), hipMemcpyHostToDevice, s->stream));
  }
  HIP_TRY(hipStreamSynchronize(s->stream));
  return RCSH_OK;
}

// ---- fused Gymnasium loop

namespace {
static_assert(RCSH_MODE_TORQUE == kEnvModeTorque && RCSH_MODE_JOINT_IMPEDANCE == kEnvModeJointImpedance &&
              RCSH_MODE_CARTESIAN_IMPEDANCE_TRPY == kEnvModeCartImpedanceTrpy && RCSH_MODE_CARTESIAN_IMPEDANCE_TQUAT == kEnvModeCartImpedanceTquat,
              "csrc/env_torque_team.h restates the control modes it serves");
bool env_torque_mode(int mode) { return mode >= RCSH_MODE_TORQUE && mode <= RCSH_MODE_CARTESIAN_IMPEDANCE_TQUAT; }
}  // namespace

int rcsh_env_configure(rcsh_sim* s, const rcsh_env_desc* env) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  if (!env) return fail(RCSH_ERR_ARG, "null env description");
  if (env->control_mode < RCSH_MODE_JOINTS || env->control_mode > RCSH_MODE_CARTESIAN_IMPEDANCE_TQUAT)
    return fail(RCSH_ERR_ARG, "bad control_mode");
  if (env->relative_to < 0 || env->relative_to > 2) return fail(RCSH_ERR_ARG, "bad relative_to");
  if (env_torque_mode(env->control_mode)) {
    // the torque and impedance modes (csrc/env_torque_team.h): every refusal before anything is written
    if (s->guard.enabled) return fail(RCSH_ERR_STATE, "the collision guard is enabled and guards position commands only: disable it (rcsh_env_configure_guard) before configuring a torque / impedance control mode");
    if (s->task.pick_cube) return fail(RCSH_ERR_STATE, "the pick task is configured: it is not built for the torque / impedance control modes");
    if (const std::string why = torque_scope(s); !why.empty()) return fail(RCSH_ERR_ARG, "torque / impedance control mode: " + why);
    if (!s->sim.async_control) return fail(RCSH_ERR_ARG, "torque / impedance control mode: async_control = 0 steps until convergence, and the convergence predicates assume position servos");
    if (env->control_mode == RCSH_MODE_TORQUE && env->relative_to != RCSH_REL_NONE)
      return fail(RCSH_ERR_ARG, "RCSH_MODE_TORQUE has no relative action space: relative_to must be RCSH_REL_NONE");
    if (int rc = torque_buffers(s)) return rc;
  }
  if (s->guard.enabled && env->control_mode != RCSH_MODE_JOINTS)
    return fail(RCSH_ERR_STATE, "the collision guard is enabled and guards joint-space actions only: disable it (rcsh_env_configure_guard) before configuring a Cartesian control mode");
  s->env.mode = env->control_mode;
  s->env.relative_to = env->relative_to;
  s->env.binary_gripper = env->binary_gripper;
  s->env.max_mov[0] = env->max_mov[0]; s->env.max_mov[1] = env->max_mov[1];
  for (int i = 0; i < s->narm; ++i) {
    s->env.low[i] = env->joint_low ? env->joint_low[i] : -INFINITY;
    s->env.high[i] = env->joint_high ? env->joint_high[i] : INFINITY;
  }
  s->env_configured = true;
  return RCSH_OK;
}

int rcsh_env_obs_width(const rcsh_sim* s) { return s ? kObsBase + s->narm : 0; }
int rcsh_env_action_width(const rcsh_sim* s) {
  if (!s) return 0;
  return action_width(s->env.mode, s->narm);
}

// ---- autoreset (csrc/episode_team.h)
namespace {
struct EpisodeRecord {
  uint8_t *done, *terminated, *truncated, *time_limit;
  double* final_obs; uint8_t* final_info; double *final_gw, *final_task;
  double* episode_return; int32_t* episode_length;
  int64_t* episodes; int32_t* elapsed; double* running_return;
  uint8_t* reset_info; double* reset_box_qpos;
};
EpisodeRecord episode_record(const rcsh_sim* s) {
  const EpisodeLayout E = episode_layout(s);
  char* d = static_cast<char*>(s->d_episode.get());
  auto at = [&](size_t o, auto* type) { return reinterpret_cast<decltype(type)>(d + o); };
  EpisodeRecord r{};
  r.done = at(E.done, r.done); r.terminated = at(E.terminated, r.terminated); r.truncated = at(E.truncated, r.truncated);
  r.time_limit = at(E.time_limit, r.time_limit);
  r.final_obs = at(E.final_obs, r.final_obs); r.final_info = at(E.final_info, r.final_info); r.final_gw = at(E.final_gw, r.final_gw);
  r.final_task = at(E.final_task, r.final_task);
  r.episode_return = at(E.episode_return, r.episode_return); r.episode_length = at(E.episode_length, r.episode_length);
  r.episodes = at(E.episodes, r.episodes); r.elapsed = at(E.elapsed, r.elapsed); r.running_return = at(E.running_return, r.running_return);
  r.reset_info = at(E.reset_info, r.reset_info); r.reset_box_qpos = at(E.reset_box_qpos, r.reset_box_qpos);
  return r;
}
// an explicit env reset begins the episodes of the environments it resets again
int episode_clear(rcsh_sim* s, const uint8_t* mask_dev) {
  if (!s->autoreset.configured) return RCSH_OK;
  const EpisodeRecord r = episode_record(s);
  hipLaunchKernelGGL(k_episode_clear, dim3(grid_for(s->n)), dim3(kBlock), 0, s->stream, mask_dev, r.elapsed, r.running_return, s->n);
  HIP_TRY(hipGetLastError());
  return RCSH_OK;
}
// ---- the torque and impedance control modes (csrc/env_torque_team.h)
// The law's TCP is the site composed with the INVERSE of its tcp_offset7 (quirk Q7), the env layer's the site composed with the robot's
// tcp_offset: the same TCP when offset7 * tcp is the identity (all-zero offset7: the identity; the quaternion up to sign).
bool env_torque_same_tcp(const rcsh_sim* s) {
  const double* o = s->tq.law.tcp_offset7;
  Pose a, b, c;
  const double nq = std::sqrt(o[3] * o[3] + o[4] * o[4] + o[5] * o[5] + o[6] * o[6]);
  const double ident[4] = {0, 0, 0, 1}, zero[3] = {0, 0, 0};
  if (nq > 0.0) {
    const double qn[4] = {o[3] / nq, o[4] / nq, o[5] / nq, o[6] / nq};
    pose_from_quat(qn, o, a);
  } else {
    pose_from_quat(ident, zero, a);
  }
  const double* r = s->robot.tcp;
  const double nr = std::sqrt(r[3] * r[3] + r[4] * r[4] + r[5] * r[5] + r[6] * r[6]);
  if (nr > 0.0) {
    const double qn[4] = {r[3] / nr, r[4] / nr, r[5] / nr, r[6] / nr};
    pose_from_quat(qn, r, b);
  } else {
    pose_from_quat(ident, r, b);
  }
  pose_mul(a, b, c);
  constexpr double kTol = 1e-12;  // (round-off of one pose product; a metre-sized offset differs by far more)
  const double sg = c.q[3] < 0.0 ? -1.0 : 1.0;
  return std::fabs(c.t[0]) <= kTol && std::fabs(c.t[1]) <= kTol && std::fabs(c.t[2]) <= kTol && std::fabs(c.q[0]) <= kTol &&
         std::fabs(c.q[1]) <= kTol && std::fabs(c.q[2]) <= kTol && std::fabs(sg * c.q[3] - 1.0) <= kTol;
}
// why a step or reset in a torque / impedance mode is refused now (RCSH_OK: it is not); nothing has been written when it is
int env_torque_ready(rcsh_sim* s, const char* what) {
  const int mode = s->env.mode;
  if (const std::string why = torque_scope(s); !why.empty()) return fail(RCSH_ERR_ARG, std::string(what) + ": " + why);
  if (!s->sim.async_control) return fail(RCSH_ERR_ARG, std::string(what) + ": async_control = 0 in a torque / impedance control mode");
  if (s->guard.enabled) return fail(RCSH_ERR_STATE, std::string(what) + ": the collision guard is enabled in a torque / impedance control mode");
  if (s->task.pick_cube) return fail(RCSH_ERR_STATE, std::string(what) + ": the pick task is configured in a torque / impedance control mode");
  // (k_env_torque parks the site frame in its substeps: a step of none would leave the observing pass and the next origin a zero frame)
  if (std::nearbyint(1.0 / s->sim.frequency / s->dm.timestep) < 1.0)
    return fail(RCSH_ERR_ARG, std::string(what) + ": round(1 / frequency / timestep) is zero substeps an env step in a torque / impedance control mode");
  if (mode != RCSH_MODE_TORQUE && !s->tq.law.enabled)
    return fail(RCSH_ERR_STATE, std::string(what) + ": the impedance control modes need an enabled torque law (rcsh_torque_configure)");
  if ((mode == RCSH_MODE_CARTESIAN_IMPEDANCE_TRPY || mode == RCSH_MODE_CARTESIAN_IMPEDANCE_TQUAT) && !env_torque_same_tcp(s))
    return fail(RCSH_ERR_ARG, std::string(what) + ": the law's tcp_offset7 and the robot's tcp_offset do not describe the same TCP (the law's TCP is the "
                              "site composed with the INVERSE of tcp_offset7: configure the inverse of the robot's tcp_offset)");
  if (s->dm.has_friction && !(s->narm == 7 && !s->grip))
    return fail(RCSH_ERR_MODEL, std::string(what) + ": no kernel instantiated for this archetype with dry joint friction");
  return torque_buffers(s);
}
// the ONE stepping launch of a step (action_dev) or a reset (do_reset, mask_dev) in a torque / impedance mode
int env_torque_launch(rcsh_sim* s, bool do_reset, const uint8_t* mask_dev, const double* action_dev, const float* gripper_dev, int32_t* substeps_dev) {
  Params P = make_params(s);
  const int mode = s->env.mode;
  // (cart_prepare reads the position mode of the same action row)
  P.env.mode = mode == RCSH_MODE_CARTESIAN_IMPEDANCE_TRPY ? RCSH_MODE_CARTESIAN_TRPY
               : mode == RCSH_MODE_CARTESIAN_IMPEDANCE_TQUAT ? RCSH_MODE_CARTESIAN_TQUAT : RCSH_MODE_JOINTS;
  // RobotSimWrapper.step (reference python/rcs/envs/sim.py:49-59); Python's round(): half to even
  const int32_t k = (int32_t)std::nearbyint(1.0 / s->sim.frequency / s->dm.timestep);
  const TorqueArgs A = torque_args(s, s->tq.law, k);
  EnvTorqueOp op{};
  op.mode = mode;
  op.do_reset = do_reset ? 1 : 0;
  op.mask = mask_dev;
  op.action = action_dev;
  op.gripper = gripper_dev;
  op.substeps = substeps_dev;
  bool launched = false;
  int rc = team_launch(s, s->n, "env step (torque / impedance)", [&](auto topo, dim3 grid, dim3 block) {
    using T = decltype(topo);
    if (!s->dm.has_friction) {
      hipLaunchKernelGGL((k_env_torque<T, false>), grid, block, 0, s->stream, P, op, A);
      launched = true;
    } else if constexpr (T::NARM == 7 && !T::GRIP) {
      hipLaunchKernelGGL((k_env_torque<T, true>), grid, block, 0, s->stream, P, op, A);
      launched = true;
    }
  });
  if (rc) return rc;
  if (!launched) return fail(RCSH_ERR_MODEL, "env step (torque / impedance): no kernel instantiated for this archetype with dry joint friction");
  return RCSH_OK;
}
// the handle's observing pass behind that launch: observation, info and gripper width of the masked environments, and the check for
// contacts nobody resolves at the handle's cadence -- so contact_unresolved belongs to the step that reports it
int env_torque_observe(rcsh_sim* s, const uint8_t* mask_dev, double* obs_dev, uint8_t* info_dev, double* gw_dev) {
  RunOp op{};
  op.nsteps = 0;
  op.observe_only = 1;
  op.write_obs = obs_dev != nullptr;
  op.check = s->contact_check && s->check_every > 0 && (s->check_seq++ % s->check_every) == 0;
  op.mask = mask_dev;
  op.obs = obs_dev; op.info = info_dev; op.gripper_width = gw_dev;
  if (!op.write_obs && !op.check) return RCSH_OK;
  return launch_run(s, op, false);
}

// What follows the stepping launch of a step under autoreset: k_episode_end over the step's outputs, then the masked reset launch
// (rcsh_env_reset_dev's, or rcsh_env_reset_task_dev's with the poses just drawn) with `done` as its mask -- always enqueued, the host
// does not know who is done --, writing the new episodes' first observation into the step's own obs / gripper_width rows.
int episode_end(rcsh_sim* s, double* obs, uint8_t* info, double* gw, const double* task) {
  const EpisodeRecord r = episode_record(s);
  const rcsh_autoreset_desc& a = s->autoreset.desc;
  EpisodeArgs A{};
  A.n = s->n; A.obs_w = kObsBase + s->narm; A.max_steps = a.max_episode_steps; A.draw_box = a.draw_box != 0;
  A.envs_per_block = kEpisodeBlock / episode_row_items(A.obs_w);
  if (A.envs_per_block < 1) return fail(RCSH_ERR_MODEL, "an environment's rows do not fit one workgroup of k_episode_end");
  A.obs = obs; A.info = info; A.gw = gw; A.task = s->task.pick_cube ? task : nullptr;
  A.done = r.done; A.terminated = r.terminated; A.truncated = r.truncated; A.time_limit = r.time_limit;
  A.final_obs = r.final_obs; A.final_info = r.final_info; A.final_gw = r.final_gw; A.final_task = r.final_task;
  A.episode_return = r.episode_return; A.episode_length = r.episode_length;
  A.episodes = r.episodes; A.elapsed = r.elapsed; A.running_return = r.running_return;
  A.reset_box_qpos = r.reset_box_qpos;
  A.draw = episode_draw_of(a);
  hipLaunchKernelGGL(k_episode_end, dim3((s->n + A.envs_per_block - 1) / A.envs_per_block), dim3(kEpisodeBlock), 0, s->stream, A);
  HIP_TRY(hipGetLastError());
  int rc = RCSH_OK;
  if (env_torque_mode(s->env.mode)) {  // (the reset form of k_env_torque, then the observing pass, both under `done`)
    rc = env_torque_launch(s, true, r.done, nullptr, nullptr, nullptr);
    if (!rc) rc = env_torque_observe(s, r.done, obs, r.reset_info, gw);
  } else {
    RunOp op{};
    op.do_reset = 1;
    op.nsteps = 1;
    op.write_obs = 1;
    op.mask = r.done;
    op.box_qpos = A.draw_box ? r.reset_box_qpos : nullptr;
    op.obs = obs; op.info = r.reset_info; op.gripper_width = gw;
    rc = launch_run(s, op, false);
  }
  if (rc) return rc;
  s->episode_stepped = true;
  s->episode_host_valid = false;
  return RCSH_OK;
}
}  // namespace

int rcsh_env_configure_autoreset(rcsh_sim* s, const rcsh_autoreset_desc* a) {
  if (const char* why = autoreset_desc_error(a, 0)) return fail(RCSH_ERR_ARG, why);  // (what needs no handle comes first)
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  if (const char* why = autoreset_desc_error(a, s->n)) return fail(RCSH_ERR_ARG, why);
  if (!s->env_configured) return fail(RCSH_ERR_STATE, "call rcsh_env_configure first");
  if (a->draw_box && !s->task.pick_cube) return fail(RCSH_ERR_STATE, "draw_box places the pick task's cube: call rcsh_env_configure_pick_task first");
  if (s->rend.ncam > 0)
    return fail(RCSH_ERR_STATE, "a render schedule is set: rate-driven cameras under autoreset are not built (remove it with rcsh_sim_set_render_schedule(ncam = 0) first)");
  const EpisodeLayout E = episode_layout(s);
  if (!s->d_episode) {  // the record and its page-locked copy: both or neither
    DevBuf<void> d;
    PinBuf<char> h;
    HIP_TRY(hipMalloc(d.out(), E.bytes));
    HIP_TRY(hipHostMalloc(h.out(), E.host_bytes, hipHostMallocDefault));
    s->d_episode = std::move(d);
    s->h_episode = std::move(h);
  }
  HIP_TRY(hipMemsetAsync(s->d_episode.get(), 0, E.bytes, s->stream));  // every counter begins again
  s->autoreset.configured = true;
  s->autoreset.enabled = a->enabled != 0;
  s->autoreset.desc = *a;
  s->episode_stepped = false;
  s->episode_host_valid = false;
  return RCSH_OK;
}

int rcsh_env_autoreset_record_dev(rcsh_sim* s, rcsh_autoreset_record* out) {
  REQUIRE_SIM(s);
  if (!s->autoreset.configured || !s->episode_stepped) return fail(RCSH_ERR_STATE, "no step under autoreset has run");
  if (!out) return fail(RCSH_ERR_ARG, "null record");
  const EpisodeRecord r = episode_record(s);
  out->done = r.done; out->terminated = r.terminated; out->truncated = r.truncated; out->time_limit = r.time_limit;
  out->final_obs = r.final_obs; out->final_info = r.final_info; out->final_gripper_width = r.final_gw; out->final_task = r.final_task;
  out->episode_return = r.episode_return; out->episode_length = r.episode_length;
  out->episodes = r.episodes; out->elapsed = r.elapsed; out->running_return = r.running_return;
  out->reset_info = r.reset_info; out->reset_box_qpos = r.reset_box_qpos;
  return RCSH_OK;
}

int rcsh_env_autoreset_last(rcsh_sim* s, uint8_t* done, uint8_t* terminated, uint8_t* truncated, uint8_t* time_limit, double* final_obs,
                            uint8_t* final_info, double* final_gripper_width, double* final_task, double* episode_return,
                            int32_t* episode_length, int64_t* episodes, int32_t* elapsed, double* running_return, uint8_t* reset_info,
                            double* reset_box_qpos) {
  REQUIRE_SIM(s);
  if (!s->autoreset.configured || !s->episode_stepped) return fail(RCSH_ERR_STATE, "no step under autoreset has run");
  const size_t n = (size_t)s->n;
  const EpisodeLayout E = episode_layout(s);
  const char* d = static_cast<const char*>(s->d_episode.get());
  const struct { void* dst; size_t at, bytes; bool front; } pieces[] = {
      {episode_return, E.episode_return, 8 * n, true}, {episode_length, E.episode_length, 4 * n, true},
      {done, E.done, n, true}, {terminated, E.terminated, n, true}, {truncated, E.truncated, n, true}, {time_limit, E.time_limit, n, true},
      {final_obs, E.final_obs, 8 * n * (size_t)(kObsBase + s->narm), false}, {final_info, E.final_info, n * kInfoBytes, false},
      {final_gripper_width, E.final_gw, 8 * n, false}, {final_task, E.final_task, 8 * n * kTaskWidth, false},
      {episodes, E.episodes, 8 * n, false}, {elapsed, E.elapsed, 4 * n, false}, {running_return, E.running_return, 8 * n, false},
      {reset_info, E.reset_info, n * kInfoBytes, false}, {reset_box_qpos, E.reset_box_qpos, 8 * n * kPoseWidth, false}};
  bool wait = false;
  for (const auto& p : pieces) {
    if (!p.dst) continue;
    if (p.front && s->episode_host_valid) { std::memcpy(p.dst, s->h_episode.get() + p.at, p.bytes); continue; }  // (rcsh_env_step brought it along)
    HIP_TRY(hipMemcpyAsync(p.dst, d + p.at, p.bytes, hipMemcpyDeviceToHost, s->stream));
    wait = true;
  }
  if (wait) HIP_TRY(hipStreamSynchronize(s->stream));
  return RCSH_OK;
}

namespace {
// env.reset's launch: with the box pose of the pick-up task's reset, or without
int env_reset_launch(rcsh_sim* s, const uint8_t* mask_dev, const double* box_qpos_dev, double* obs_dev, uint8_t* info_dev, double* gw_dev) {
  RunOp op{};
  op.do_reset = 1;
  op.nsteps = 1;
  op.write_obs = obs_dev != nullptr;
  op.mask = mask_dev;
  op.box_qpos = box_qpos_dev;
  op.obs = obs_dev; op.info = info_dev; op.gripper_width = gw_dev;
  int rc = launch_run(s, op, false);
  return rc ? rc : episode_clear(s, mask_dev);
}
}  // namespace

int rcsh_env_reset_dev(rcsh_sim* s, const uint8_t* mask_dev, double* obs_dev, uint8_t* info_dev, double* gw_dev) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  if (!s->env_configured) return fail(RCSH_ERR_STATE, "call rcsh_env_configure first");
  if (env_torque_mode(s->env.mode)) {
    int rc = env_torque_ready(s, "env reset");
    if (!rc) rc = env_torque_launch(s, true, mask_dev, nullptr, nullptr, nullptr);
    if (!rc) rc = env_torque_observe(s, mask_dev, obs_dev, info_dev, gw_dev);
    return rc ? rc : episode_clear(s, mask_dev);
  }
  return env_reset_launch(s, mask_dev, nullptr, obs_dev, info_dev, gw_dev);
}

// ---- the collision guard (csrc/guard_team.h)
namespace {
struct GuardRecord { int32_t* result; double* t_contact; uint8_t* blocked; uint8_t* hold; };
GuardRecord guard_record(const rcsh_sim* s, int which) {  // 0: the last guarded step, 1: the peek's scratch
  const GuardLayout G = guard_layout(s);
  char* d = static_cast<char*>(s->d_guard.get()) + (size_t)which * G.bytes;
  GuardRecord r{};
  r.t_contact = reinterpret_cast<double*>(d + G.t_contact);
  r.result = reinterpret_cast<int32_t*>(d + G.result);
  r.blocked = reinterpret_cast<uint8_t*>(d + G.blocked);
  r.hold = reinterpret_cast<uint8_t*>(d + G.hold);
  return r;
}
// a host form's downloads of a record's arrays, read where they lie (null: not asked for)
void guard_outputs(StageLayout& L, const GuardRecord& r, size_t n, int32_t* result, double* t_contact, uint8_t* blocked) {
  L.out_from(result, r.result, n);
  L.out_from(t_contact, r.t_contact, n);
  L.out_from(blocked, r.blocked, n);
}
__global__ void k_guard_fill(int32_t* result, double* t_contact, uint8_t* blocked, uint8_t* hold, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { result[i] = 0; t_contact[i] = -1.0; blocked[i] = 0; if (hold) hold[i] = kGuardLive; }
}
// RobotSimWrapper.step's `truncated` of a blocked environment (info row, byte 4), after the stepping launch
__global__ void k_guard_truncate(uint8_t* info, const uint8_t* blocked, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && blocked[i]) info[(size_t)i * 8 + 4] = 1;
}
// the guard kernel over every environment for the actions at action_dev, into device buffers
int guard_launch(rcsh_sim* s, const double* action_dev, int32_t* result, double* t_contact, uint8_t* blocked, uint8_t* hold) {
  if (s->cgeoms.empty()) {  // (a robot without collision geometry: nothing can be in contact, as the queries answer)
    hipLaunchKernelGGL(k_guard_fill, dim3((s->n + 63) / 64), dim3(64), 0, s->stream, result, t_contact, blocked, hold, s->n);
    HIP_TRY(hipGetLastError());
    return RCSH_OK;
  }
  GuardArgs G{};
  const bool box = (s->guard.kinds & kQueryBox) && s->box.present;
  const int32_t kinds = s->guard.kinds & (box ? kQueryKinds : (kQueryFloor | kQuerySelf));
  G.Q = query_args(s, s->n, kinds, query_pairs(s, kinds, false));
  G.Q.resolution = s->guard.resolution;
  // A finger of the open hand rests ON its joint limit, and the soft limit lets it through by some 10 um (measured: up to 44 um in a
  // rollout): for the motion query such a row has left the stroke the levers were built for and is never certified -- the guard
  // would block a quarter of a batch for it.  The levers hold further than the query admits: model.cpp build_self_levers charges a hinge
  // 1.01 (d + stroke) + kLeverSlack for a geom whose distance bound is d + stroke, and a chain holds one slide, so a slide up to
  // kLeverSlack past its stroke is covered by that additive term alone.  The guard admits half of it.
  constexpr double kGuardSlideTol = 5e-4;
  static_assert(kGuardSlideTol <= 0.5 * kLeverSlack, "the guard's slide tolerance lives inside the levers' additive slack");
  for (int L = 0; L < 12; ++L) { G.Q.slide_lo[L] -= kGuardSlideTol; G.Q.slide_hi[L] += kGuardSlideTol; }
  G.S = s->S.get();
  G.flags = s->flags.get();
  G.action = action_dev;
  G.env = s->env;
  G.box_field = box ? field_of(s, "box") + kBoxQ : -1;
  G.block_undecided = s->guard.block_undecided ? 1 : 0;
  G.result = result; G.t_contact = t_contact; G.blocked = blocked; G.hold = hold;
  return team_launch(s, s->n, "collision guard", [&](auto topo, dim3 grid, dim3 block) {
    hipLaunchKernelGGL(k_env_guard<decltype(topo)>, grid, block, 0, s->stream, G);
  });
}
}  // namespace

int rcsh_env_configure_guard(rcsh_sim* s, const rcsh_guard_desc* g) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  if (!s->env_configured) return fail(RCSH_ERR_STATE, "call rcsh_env_configure first");
  if (!g) return fail(RCSH_ERR_ARG, "null guard description");
  if (g->kinds < 1 || g->kinds > kQueryKinds) return fail(RCSH_ERR_ARG, "the guard's kinds mask must select at least one of bit 0 floor, 1 self, 2 free body, and nothing else");
  if (!(g->resolution > 0.0) || !std::isfinite(g->resolution)) return fail(RCSH_ERR_ARG, "resolution must be positive and finite");
  if (env_torque_mode(s->env.mode))
    return fail(RCSH_ERR_STATE, "the collision guard guards position commands only: the environments are configured for a torque / impedance control mode");
  if (s->env.mode != RCSH_MODE_JOINTS)
    return fail(RCSH_ERR_STATE, "the collision guard guards joint-space actions only: the environments are configured for a Cartesian control mode");
  int rc = query_check(s, s->n, g->kinds, nullptr);
  if (rc) return rc;
  if (!s->d_guard) {  // the two records and the page-locked copy: both or neither
    DevBuf<void> d;
    PinBuf<char> h;
    HIP_TRY(hipMalloc(d.out(), 2 * guard_layout(s).bytes));
    HIP_TRY(hipHostMalloc(h.out(), guard_layout(s).host_bytes, hipHostMallocDefault));
    s->d_guard = std::move(d);
    s->h_guard = std::move(h);
  }
  s->guard.configured = true;
  s->guard.enabled = g->enabled != 0;
  s->guard.kinds = g->kinds;
  s->guard.resolution = g->resolution;
  s->guard.block_undecided = g->block_undecided != 0;
  s->guard.truncate = g->truncate != 0;
  return RCSH_OK;
}

int rcsh_env_guard_peek_dev(rcsh_sim* s, const double* action_dev, int32_t* result_dev, double* t_contact_dev, uint8_t* blocked_dev) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  if (!s->guard.configured) return fail(RCSH_ERR_STATE, "call rcsh_env_configure_guard first");
  if (s->env.mode != RCSH_MODE_JOINTS)
    return fail(RCSH_ERR_STATE, env_torque_mode(s->env.mode)
                                    ? "the collision guard answers for joint-space position commands only: the environments are configured for a torque / impedance control mode"
                                    : "the collision guard answers for joint-space actions only: the environments are configured for a Cartesian control mode");
  if (!action_dev || !result_dev || !t_contact_dev || !blocked_dev) return fail(RCSH_ERR_ARG, "null argument");
  return guard_launch(s, action_dev, result_dev, t_contact_dev, blocked_dev, nullptr);
}

int rcsh_env_guard_peek(rcsh_sim* s, const double* action, int32_t* result, double* t_contact, uint8_t* blocked) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  if (!s->guard.configured) return fail(RCSH_ERR_STATE, "call rcsh_env_configure_guard first");
  if (s->env.mode != RCSH_MODE_JOINTS)
    return fail(RCSH_ERR_STATE, env_torque_mode(s->env.mode)
                                    ? "the collision guard answers for joint-space position commands only: the environments are configured for a torque / impedance control mode"
                                    : "the collision guard answers for joint-space actions only: the environments are configured for a Cartesian control mode");
  if (!action) return fail(RCSH_ERR_ARG, "null action");
  const size_t n = (size_t)s->n, na = n * (size_t)s->narm;
  int rc = query_finite(action, na, "action");
  if (rc) return rc;
  const GuardRecord r = guard_record(s, 1);  // (the answers land in the guard's scratch record, not in the staging)
  StageLayout L;
  const auto da = L.in(action, na);
  guard_outputs(L, r, n, result, t_contact, blocked);
  return staged_call(s, s->d_query, L, [&](auto dev) { return guard_launch(s, dev(da), r.result, r.t_contact, r.blocked, nullptr); });
}

int rcsh_env_guard_last_dev(rcsh_sim* s, const int32_t** result_dev, const double** t_contact_dev, const uint8_t** blocked_dev) {
  REQUIRE_SIM(s);
  if (!s->guard.configured || !s->guard_stepped) return fail(RCSH_ERR_STATE, "no guarded step has run");
  const GuardRecord r = guard_record(s, 0);
  if (result_dev) *result_dev = r.result;
  if (t_contact_dev) *t_contact_dev = r.t_contact;
  if (blocked_dev) *blocked_dev = r.blocked;
  return RCSH_OK;
}

int rcsh_env_guard_last(rcsh_sim* s, int32_t* result, double* t_contact, uint8_t* blocked) {
  REQUIRE_SIM(s);
  if (!s->guard.configured || !s->guard_stepped) return fail(RCSH_ERR_STATE, "no guarded step has run");
  const size_t n = (size_t)s->n;
  if (s->guard_host_valid) {  // (rcsh_env_step brought the record along with its outputs)
    const GuardLayout G = guard_layout(s);
    const char* hg = s->h_guard.get();
    if (t_contact) std::memcpy(t_contact, hg + G.t_contact, 8 * n);
    if (result) std::memcpy(result, hg + G.result, 4 * n);
    if (blocked) std::memcpy(blocked, hg + G.blocked, n);
    return RCSH_OK;
  }
  StageLayout L;  // (nothing staged: the record is read where it lies)
  guard_outputs(L, guard_record(s, 0), n, result, t_contact, blocked);
  return staged_call(s, s->d_query, L, [](auto) { return (int)RCSH_OK; });
}

int rcsh_env_step_dev(rcsh_sim* s, const double* action_dev, const float* gripper_dev, double* obs_dev, uint8_t* info_dev,
                      double* gw_dev, int32_t* substeps_dev) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  if (!s->env_configured) return fail(RCSH_ERR_STATE, "call rcsh_env_configure first");
  if (!action_dev) return fail(RCSH_ERR_ARG, "null action");
  if (env_torque_mode(s->env.mode)) {
    if (int rc = env_torque_ready(s, "env step")) return rc;
  }
  double* task_dev = s->pending_task;
  const bool autoreset = s->autoreset.enabled;
  if (autoreset) {  // (k_episode_end reads the step's outputs: an output the caller does not ask for goes to the staging slice)
    const Staging& st = s->stage;
    if (!obs_dev) obs_dev = st.obs;
    if (!info_dev) info_dev = st.info;
    if (!gw_dev) gw_dev = st.grip_width;
    if (!task_dev && s->task.pick_cube) task_dev = st.box_task;
  }
  if (env_torque_mode(s->env.mode)) {
    // one stepping launch -- action arithmetic, target write, substeps --, then the observing pass
    int rc = env_torque_launch(s, false, nullptr, action_dev, gripper_dev, substeps_dev);
    if (!rc) rc = env_torque_observe(s, nullptr, obs_dev, info_dev, gw_dev);
    if (rc) return rc;
    return autoreset ? episode_end(s, obs_dev, info_dev, gw_dev, task_dev) : (int)RCSH_OK;
  }
  RunOp op{};
  op.apply_action = 1;
  const bool guarded = s->guard.enabled && s->env.mode == RCSH_MODE_JOINTS;  // (rcsh_env_configure refuses a Cartesian mode under a guard)
  if (guarded) {
    // the guard decides on the stream ahead of the stepping launch, which reads the verdicts as its mask (RunOp::apply_action == 2)
    const GuardRecord r = guard_record(s, 0);
    int rc = guard_launch(s, action_dev, r.result, r.t_contact, r.blocked, r.hold);
    if (rc) return rc;
    op.apply_action = 2;
    op.mask = r.hold;
  }
  if (s->env.mode != RCSH_MODE_JOINTS) {
    // Cartesian modes: wrappers' action() + IK run in their own launch, the stepping launch follows on the stream
    CartOp cop{};
    cop.env_layer = 1;
    cop.action = action_dev;
    cop.gripper = gripper_dev;
    int rc = launch_cartesian(s, cop);
    if (rc) return rc;
    op.apply_action = 0;
  }
  // RobotSimWrapper.step (reference python/rcs/envs/sim.py:49-59)
  // (Python's round(): half to even, as std::nearbyint under the default rounding mode)
  op.nsteps = s->sim.async_control ? (int32_t)std::nearbyint(1.0 / s->sim.frequency / s->dm.timestep) : -1;
  op.write_obs = obs_dev != nullptr;
  op.action = action_dev; op.gripper = gripper_dev;
  op.obs = obs_dev; op.info = info_dev; op.gripper_width = gw_dev; op.substeps = substeps_dev;
  op.task = task_dev;
  int rc = launch_run(s, op, true);
  if (rc) return rc;
  if (guarded) { s->guard_stepped = true; s->guard_host_valid = false; }
  if (guarded && s->guard.truncate && info_dev) {
    hipLaunchKernelGGL(k_guard_truncate, dim3((s->n + 63) / 64), dim3(64), 0, s->stream, info_dev, guard_record(s, 0).blocked, s->n);
    HIP_TRY(hipGetLastError());
  }
  if (autoreset) return episode_end(s, obs_dev, info_dev, gw_dev, task_dev);
  return RCSH_OK;
}

// ---- task layer of the pick-up scene: SimTaskEnvCreator = SimEnvCreator + RandomCubePos under the RobotSimWrapper +
// PickCubeSuccessWrapper on top (reference python/rcs/envs/creators.py:131-187)
int rcsh_env_configure_pick_task(rcsh_sim* s, const rcsh_pick_task_desc* t) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  if (!t) return fail(RCSH_ERR_ARG, "null task description");
  if (!s->box.present) return fail(RCSH_ERR_STATE, "the pick task needs the scene's free box: call rcsh_sim_add_free_box first");
  if (s->env_configured && env_torque_mode(s->env.mode)) return fail(RCSH_ERR_STATE, "the pick task is not built for the torque / impedance control modes");
  s->task.pick_cube = 1;
  for (int k = 0; k < 3; ++k) s->task.ee_home[k] = t->ee_home[k];
  s->task.success_z = t->success_height;
  return upload_boxtask(s);
}

int rcsh_env_reset_task_dev(rcsh_sim* s, const uint8_t* mask_dev, const double* box_qpos_dev, double* obs_dev, uint8_t* info_dev,
                            double* gw_dev) {
  REQUIRE_SIM(s); REQUIRE_ROBOT(s);
  if (!s->env_configured) return fail(RCSH_ERR_STATE, "call rcsh_env_configure first");
  if (!s->task.pick_cube) return fail(RCSH_ERR_STATE, "call rcsh_env_configure_pick_task first");
  if (!box_qpos_dev) return fail(RCSH_ERR_ARG, "null box pose");
  return env_reset_launch(s, mask_dev, box_qpos_dev, obs_dev, info_dev, gw_dev);
}

int rcsh_env_step_task_dev(rcsh_sim* s, const double* action_dev, const float* gripper_dev, double* obs_dev, uint8_t* info_dev,
                           double* gw_dev, int32_t* substeps_dev, double* task_dev) {
  REQUIRE_SIM(s);
  if (!s->task.pick_cube) return fail(RCSH_ERR_STATE, "call rcsh_env_configure_pick_task first");
  s->pending_task = task_dev;
  int rc = rcsh_env_step_dev(s, action_dev, gripper_dev, obs_dev, info_dev, gw_dev, substeps_dev);
  s->pending_task = nullptr;
  return rc;
}

namespace {
// the host forms of env.reset: with the box pose of the pick-up task's reset, or without
int env_reset_host(rcsh_sim* s, const uint8_t* mask, const double* box_qpos, double* obs, uint8_t* info, double* gw) {
  const Staging& st = s->stage;
  const uint8_t* dm = nullptr;
  int rc = upload_mask(s, mask, &dm);
  if (rc) return rc;
  if (box_qpos) {
    char* h = nullptr;
    if ((rc = pin_ready(s, h))) return rc;
    if ((rc = pin_upload(s, st.box_task, h + s->pin.box, box_qpos, sizeof(double) * s->n * kPoseWidth))) return rc;
    rc = rcsh_env_reset_task_dev(s, dm, st.box_task, st.obs, st.info, st.grip_width);
  } else {
    rc = rcsh_env_reset_dev(s, dm, st.obs, st.info, st.grip_width);
  }
  if (!rc) rc = observe_unmasked(s, mask);
  if (rc) return rc;
  return fetch_env_outputs(s, EnvOut{obs, info, gw, nullptr, nullptr}, false);
}

// the host forms of env.step; `with_task`: the pick-up task's rows are written (and fetched into out.task, if given)
int env_step_host(rcsh_sim* s, const double* action, const float* gripper, const EnvOut& out, bool with_task) {
  if (!action) return fail(RCSH_ERR_ARG, "null action");
  const Staging& st = s->stage;
  const int aw = rcsh_env_action_width(s);
  const PinLayout& L = s->pin;
  char* h = nullptr;
  int rc = fits(aw, st.action_w, "the env-step's action");
  if (!rc) rc = pin_ready(s, h);
  if (!rc) rc = pin_upload(s, st.action, h + L.action, action, sizeof(double) * s->n * aw);
  if (!rc && gripper) rc = pin_upload(s, st.grip_cmd, h + L.gripper, gripper, sizeof(float) * s->n);
  if (rc) return rc;
  s->pending_task = with_task ? st.box_task : nullptr;
  rc = rcsh_env_step_dev(s, st.action, gripper ? st.grip_cmd : nullptr, st.obs, st.info, st.grip_width, st.substeps);
  s->pending_task = nullptr;
  if (rc) return rc;
  const bool guard_record_too = s->guard.enabled && s->guard_stepped && s->h_guard;
  const bool episode_record_too = s->autoreset.enabled && s->episode_stepped && s->h_episode;
  if ((rc = fetch_env_outputs(s, out, guard_record_too, episode_record_too))) return rc;
  s->guard_host_valid = guard_record_too;
  s->episode_host_valid = episode_record_too;
  return RCSH_OK;
}
}  // namespace

int rcsh_env_reset_task(rcsh_sim* s, const uint8_t* mask, const double* box_qpos, double* obs, uint8_t* info, double* gw) {
  REQUIRE_SIM(s);
  if (!box_qpos) return fail(RCSH_ERR_ARG, "null box pose");
  return env_reset_host(s, mask, box_qpos, obs, info, gw);
}

int rcsh_env_step_task(rcsh_sim* s, const double* action, const float* gripper, double* obs, uint8_t* info, double* gw,
                       int32_t* substeps, double* task) {
  REQUIRE_SIM(s);
  if (!s->task.pick_cube) return fail(RCSH_ERR_STATE, "call rcsh_env_configure_pick_task first");
  return env_step_host(s, action, gripper, EnvOut{obs, info, gw, substeps, task}, true);
}

int rcsh_env_reset(rcsh_sim* s, const uint8_t* mask, double* obs, uint8_t* info, double* gw) {
  REQUIRE_SIM(s);
  return env_reset_host(s, mask, nullptr, obs, info, gw);
}

int rcsh_env_step(rcsh_sim* s, const double* action, const float* gripper, double* obs, uint8_t* info, double* gw, int32_t* substeps) {
  REQUIRE_SIM(s);
  return env_step_host(s, action, gripper, EnvOut{obs, info, gw, substeps, nullptr}, false);
}

// ---- depth renderer
int rcsh_sim_set_render_scene(rcsh_sim* s, const rcsh_render_scene_desc* d) {
  REQUIRE_SIM(s);
  if (!d || d->nshape < 1 || d->nshape > kMaxShapes) return fail(RCSH_ERR_ARG, "render scene: between 1 and 32 shapes");
  if (!(d->znear > 0) || !(d->zfar > d->znear)) return fail(RCSH_ERR_ARG, "render scene: need 0 < znear < zfar");
  std::vector<RenderShape> sh(d->nshape);
  for (int i = 0; i < d->nshape; ++i) {
    RenderShape& r = sh[i];
    r.shape = d->shape[i]; r.link = d->link[i]; r.plane_adr = d->plane_adr[i]; r.plane_num = d->plane_num[i];
    if (r.shape < kShapePlane || r.shape > kShapeCapsule) return fail(RCSH_ERR_ARG, "render scene: unknown shape type");
    if (r.link < kLinkFreeBody || r.link >= s->nl) return fail(RCSH_ERR_ARG, "render scene: link index out of range");
    if (r.link == kLinkFreeBody && !s->box.present) return fail(RCSH_ERR_STATE, "render scene: no free box attached");
    if (r.shape == kShapeHull && (r.plane_adr < 0 || r.plane_num < 4 || r.plane_adr + r.plane_num > d->nplanes))
      return fail(RCSH_ERR_ARG, "render scene: hull plane range out of bounds");
    for (int k = 0; k < 3; ++k) { r.pos[k] = d->pos[3 * i + k]; r.size[k] = d->size[3 * i + k]; }
    for (int k = 0; k < 9; ++k) r.rot[k] = d->rot[9 * i + k];
    for (int k = 0; k < 4; ++k) r.sphere[k] = d->sphere[4 * i + k];
  }
  // The outline method (render.h: k_hull_views): each hull's polytope edges, worked out here from its planes, and room for one view
  // record per environment and hull.  RCSH_RENDER_OUTLINE=0 keeps the plane-by-plane walk (measurements); a hull whose planes
  // do not give a clean polytope is walked plane by plane as well.
  std::vector<int32_t> edge_planes;
  std::vector<double> edge_verts;
  int64_t view_stride = 0;
  {
    const char* env = std::getenv("RCSH_RENDER_OUTLINE");
    const bool outline = !(env && env[0] == '0');
    for (int i = 0; i < d->nshape && outline; ++i) {
      RenderShape& r = sh[i];
      if (r.shape != kShapeHull) continue;
      std::vector<HullEdge> edges;
      if (!build_hull_edges(d->planes + 4 * (size_t)r.plane_adr, r.plane_num, edges, r.centre)) continue;
      r.edge_adr = (int32_t)(edge_planes.size() / 2);
      r.edge_num = (int32_t)edges.size();
      r.view_adr = view_stride;
      view_stride += hull_view_doubles(r.plane_num);
      for (const HullEdge& e : edges) {
        edge_planes.push_back(e.a); edge_planes.push_back(e.b);
        edge_verts.insert(edge_verts.end(), e.v1, e.v1 + 3);
        edge_verts.insert(edge_verts.end(), e.v2, e.v2 + 3);
      }
    }
  }
  // the new scene is built beside the old one, which stays attached and valid until the new one is complete
  const bool first_scene = !s->rbuf.frames;
  rcsh_sim::RenderBufs nb;  // (without colours: rcsh_sim_set_render_colours follows a new scene)
  const int np = d->nplanes > 0 ? d->nplanes : 1;
  HIP_TRY(hipMalloc(nb.shapes.out(), sizeof(RenderShape) * d->nshape));
  HIP_TRY(hipMalloc(nb.planes.out(), sizeof(double) * 4 * np));
  HIP_TRY(hipMalloc(nb.frames.out(), sizeof(double) * 12 * (size_t)(s->nl + 1) * s->n));
  HIP_TRY(hipMalloc(nb.wframes.out(), sizeof(double) * kShapeFrameDoubles * (size_t)(d->nshape + 1) * s->n));
  if (view_stride > 0) {
    HIP_TRY(hipMalloc(nb.edge_planes.out(), sizeof(int32_t) * edge_planes.size()));
    HIP_TRY(hipMalloc(nb.edge_verts.out(), sizeof(double) * edge_verts.size()));
    HIP_TRY(hipMalloc(nb.views.out(), sizeof(double) * (size_t)view_stride * s->n));
    HIP_TRY(hipMemcpyAsync(nb.edge_planes.get(), edge_planes.data(), sizeof(int32_t) * edge_planes.size(), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(nb.edge_verts.get(), edge_verts.data(), sizeof(double) * edge_verts.size(), hipMemcpyHostToDevice, s->stream));
  }
  HIP_TRY(hipMemcpyAsync(nb.shapes.get(), sh.data(), sizeof(RenderShape) * d->nshape, hipMemcpyHostToDevice, s->stream));
  if (d->nplanes > 0) HIP_TRY(hipMemcpyAsync(nb.planes.get(), d->planes, sizeof(double) * 4 * d->nplanes, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  // The kernels keep "the qpos the last position stage saw" (what mjData.xpos / geom_xpos derive from) only while a render
  // scene is attached.  A scene attached after some stepping starts from the current qpos instead of whatever the field held:
  // one substep's motion off for the first frame, never a stale pose.
  if (first_scene) with_layout(s, [&](auto topo) {
    using L = Lay<decltype(topo)>;
    const size_t n = (size_t)s->n;
    (void)hipMemcpyAsync(s->S.get() + (size_t)L::QPRE * n, s->S.get() + (size_t)L::QPOS * n, sizeof(double) * n * s->nl, hipMemcpyDeviceToDevice, s->stream);
    if (s->box.present)
      (void)hipMemcpyAsync(s->S.get() + (size_t)(L::BOX + kBoxPre) * n, s->S.get() + (size_t)(L::BOX + kBoxQ) * n, sizeof(double) * n * 7, hipMemcpyDeviceToDevice, s->stream);
    return 0;
  });
  HIP_TRY(hipStreamSynchronize(s->stream));
  s->rbuf = std::move(nb);  // (the old scene's buffers go here)
  s->rscene.nshape = d->nshape; s->rscene.nframes = s->nl + 1;
  s->rscene.znear = d->znear; s->rscene.zfar = d->zfar;
  s->rscene.inv_near = 1.0 / d->znear; s->rscene.inv_span = 1.0 / (1.0 / d->znear - 1.0 / d->zfar);
  s->rscene.shapes = s->rbuf.shapes.get(); s->rscene.planes = s->rbuf.planes.get(); s->rscene.colours = s->rbuf.colours.get();
  s->rscene.edge_planes = s->rbuf.edge_planes.get(); s->rscene.edge_verts = s->rbuf.edge_verts.get(); s->rscene.views = s->rbuf.views.get(); s->rscene.view_stride = view_stride;
  return RCSH_OK;
}

int rcsh_hull_edges(const double* planes, int32_t nplanes, int32_t capacity, int32_t* edge_planes, double* edge_verts, int32_t* nedges, double* centre) {
  if (!planes || !nedges || !centre || nplanes < 0 || capacity < 0) return fail(RCSH_ERR_ARG, "hull edges: null argument");
  std::vector<HullEdge> edges;
  *nedges = 0;
  if (!build_hull_edges(planes, nplanes, edges, centre)) return RCSH_OK;  // (no clean polytope: zero edges, the hull is walked plane by plane)
  *nedges = (int32_t)edges.size();
  if (!edge_planes || !edge_verts) return RCSH_OK;
  if ((int32_t)edges.size() > capacity) return fail(RCSH_ERR_ARG, "hull edges: capacity too small");
  for (size_t k = 0; k < edges.size(); ++k) {
    edge_planes[2 * k] = edges[k].a; edge_planes[2 * k + 1] = edges[k].b;
    for (int t = 0; t < 3; ++t) { edge_verts[6 * k + t] = edges[k].v1[t]; edge_verts[6 * k + 3 + t] = edges[k].v2[t]; }
  }
  return RCSH_OK;
}

int rcsh_sim_add_camera(rcsh_sim* s, const rcsh_camera_desc* c, int32_t* cam_id) {
  REQUIRE_SIM(s);
  if (!c || !cam_id) return fail(RCSH_ERR_ARG, "null camera description");
  if (c->width < 1 || c->height < 1 || !(c->fovy_deg > 0 && c->fovy_deg < 180)) return fail(RCSH_ERR_ARG, "camera: bad resolution or field of view");
  if (c->link < kLinkFreeBody || c->link >= s->nl) return fail(RCSH_ERR_ARG, "camera: link index out of range");
  RenderCam rc{};
  rc.link = c->link; rc.width = c->width; rc.height = c->height;
  for (int k = 0; k < 3; ++k) rc.pos[k] = c->pos[k];
  for (int k = 0; k < 9; ++k) rc.rot[k] = c->rot[k];
  rc.tan_half_fovy = std::tan(c->fovy_deg * 3.14159265358979323846 / 360.0);
  rc.tx = rc.tan_half_fovy * (double)c->width / (double)c->height;
  rc.two_over_w = 2.0 / c->width; rc.two_over_h = 2.0 / c->height;
  s->cams.push_back(rc);
  *cam_id = (int32_t)s->cams.size() - 1;
  return RCSH_OK;
}

int rcsh_sim_set_render_colours(rcsh_sim* s, const rcsh_render_colours* c) {
  REQUIRE_SIM(s);
  if (!s->rbuf.frames) return fail(RCSH_ERR_STATE, "no render scene: call rcsh_sim_set_render_scene first");
  if (!c || !c->colour) return fail(RCSH_ERR_ARG, "null colour table");
  const int ns = s->rscene.nshape;
  std::vector<RenderColour> col(ns);
  for (int i = 0; i < ns; ++i) {
    const double* w = c->colour + 8 * (size_t)i;
    for (int k = 0; k < 3; ++k) { col[i].rgb[k] = w[k]; col[i].rgb2[k] = w[3 + k]; }
    col[i].square = w[6]; col[i].checker = w[7];
    if (col[i].checker != 0.0 && !(col[i].square > 0)) return fail(RCSH_ERR_ARG, "render colours: checker squares need a positive edge length");
  }
  if (!s->rbuf.colours) HIP_TRY(hipMalloc(s->rbuf.colours.out(), sizeof(RenderColour) * ns));
  HIP_TRY(hipMemcpyAsync(s->rbuf.colours.get(), col.data(), sizeof(RenderColour) * ns, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  s->rscene.colours = s->rbuf.colours.get();
  RenderShade& L = s->rscene.shade;
  for (int k = 0; k < 3; ++k) {
    L.ambient[k] = c->headlight_ambient[k]; L.head_diffuse[k] = c->headlight_diffuse[k];
    L.light_dir[k] = c->light_dir[k]; L.light_diffuse[k] = c->light_diffuse[k];
    L.sky1[k] = c->sky_rgb1[k]; L.sky2[k] = c->sky_rgb2[k];
  }
  const double dn = std::sqrt(L.light_dir[0] * L.light_dir[0] + L.light_dir[1] * L.light_dir[1] + L.light_dir[2] * L.light_dir[2]);
  if (dn > 0) for (int k = 0; k < 3; ++k) L.light_dir[k] /= dn;
  return RCSH_OK;
}

int rcsh_sim_set_render_schedule(rcsh_sim* s, const int32_t* cam_ids, const double* seconds_between_calls, int32_t ncam, int32_t capacity) {
  REQUIRE_SIM(s);
  if (!s->rbuf.frames) return fail(RCSH_ERR_STATE, "no render scene: call rcsh_sim_set_render_scene first");
  if (ncam < 0 || ncam > kMaxRateCams) return fail(RCSH_ERR_ARG, "render schedule: at most 4 cameras with a frame rate");
  if (ncam > 0 && (!cam_ids || !seconds_between_calls || capacity < 1 || capacity > 256)) return fail(RCSH_ERR_ARG, "render schedule: bad arguments");
  if (ncam > 0 && s->autoreset.enabled)
    return fail(RCSH_ERR_STATE, "autoreset is enabled: rate-driven cameras under autoreset are not built (disable it with rcsh_env_configure_autoreset first)");
  for (int c = 0; c < ncam; ++c) {
    if (cam_ids[c] < 0 || cam_ids[c] >= (int)s->cams.size()) return fail(RCSH_ERR_ARG, "render schedule: unknown camera id");
    if (!(seconds_between_calls[c] > 0)) return fail(RCSH_ERR_ARG, "render schedule: the period must be positive");
  }
  HIP_TRY(hipStreamSynchronize(s->stream));
  const size_t n = (size_t)s->n, nf = (size_t)s->nl + 9;
  // The same cameras with the same periods and a larger capacity: the schedule GROWS -- the cameras' clocks and what the last
  // launch recorded stay (a host that is about to run a longer launch than the schedule was sized for -- Sim.step(k) with a
  // large k, a raised max_convergence_steps -- calls this first; re-registering must not make every camera due again).
  bool same = ncam > 0 && ncam == s->rend.ncam && capacity >= s->rend.capacity;
  for (int c = 0; same && c < ncam; ++c) same = s->rend_cam_id[c] == cam_ids[c] && s->rend.period[c] == seconds_between_calls[c];
  if (same) {
    if (capacity == s->rend.capacity) return RCSH_OK;
    DevBuf<double> snap;
    HIP_TRY(hipMalloc(snap.out(), sizeof(double) * (size_t)capacity * nf * n));
    HIP_TRY(hipMemcpy(snap.get(), s->rend.snap, sizeof(double) * (size_t)s->rend.capacity * nf * n, hipMemcpyDeviceToDevice));
    s->rend_snap = std::move(snap);
    s->rend.snap = s->rend_snap.get();
    s->rend.capacity = capacity;
    return RCSH_OK;
  }
  // another schedule, or none: the new one is built in locals, the old one stays until it is complete
  DevBuf<double> last_dev, snap;
  DevBuf<int32_t> count;
  RendCfg rend{};
  if (ncam > 0) {
    HIP_TRY(hipMalloc(last_dev.out(), sizeof(double) * kMaxRateCams * n));
    HIP_TRY(hipMalloc(snap.out(), sizeof(double) * (size_t)capacity * nf * n));
    HIP_TRY(hipMalloc(count.out(), sizeof(int32_t) * n));
    HIP_TRY(hipMemsetAsync(count.get(), 0, sizeof(int32_t) * n, s->stream));
    // register_rendering_callback (sim.cpp:160-173): last_call_timestamp = -1 / frame_rate, "so that we will directly render"
    std::vector<double> last(kMaxRateCams * n, 0.0);
    for (int c = 0; c < ncam; ++c) {
      rend.period[c] = seconds_between_calls[c];
      for (size_t e = 0; e < n; ++e) last[c * n + e] = -seconds_between_calls[c];
    }
    HIP_TRY(hipMemcpyAsync(last_dev.get(), last.data(), sizeof(double) * last.size(), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    rend.ncam = ncam;
    rend.capacity = capacity;
  }
  s->rend_last = std::move(last_dev); s->rend_snap = std::move(snap); s->rend_count = std::move(count);
  rend.last = s->rend_last.get(); rend.snap = s->rend_snap.get(); rend.count = s->rend_count.get();
  s->rend = rend;
  for (int c = 0; c < ncam; ++c) s->rend_cam_id[c] = cam_ids[c];
  s->rend_dropped = 0;
  return RCSH_OK;
}

int rcsh_render_pending(rcsh_sim* s, int32_t* count) {
  REQUIRE_SIM(s);
  if (!count) return fail(RCSH_ERR_ARG, "null output");
  if (s->rend.ncam == 0) return fail(RCSH_ERR_STATE, "no render schedule: call rcsh_sim_set_render_schedule first");
  HIP_TRY(hipMemcpyAsync(count, s->rend.count, sizeof(int32_t) * s->n, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  // more frames due in one launch than the schedule holds: the records beyond its capacity were not written (the newest are
  // lost); the stepping itself is unaffected, so this is a count for the host to warn about, not an error after the fact
  bool clamped = false;
  for (int e = 0; e < s->n; ++e)
    if (count[e] > s->rend.capacity) {
      s->rend_dropped += count[e] - s->rend.capacity;
      count[e] = s->rend.capacity;
      clamped = true;
    }
  if (clamped) {
    // the device-side counters outlive this call (observation-only launches keep them, and so does a second pending / collect
    // without a stepping launch in between): write the clamped counts back, so that an overflow is counted ONCE (advisor, round 3)
    HIP_TRY(hipMemcpyAsync(s->rend.count, count, sizeof(int32_t) * s->n, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
  }
  return RCSH_OK;
}

int rcsh_render_dropped(rcsh_sim* s, int64_t* dropped) {
  REQUIRE_SIM(s);
  if (dropped) *dropped = s->rend_dropped;
  return RCSH_OK;
}

int rcsh_camera_render_snapshot(rcsh_sim* s, int32_t cam_id, int32_t slot, uint8_t* rgb, float* depth_gl, uint16_t* depth_mm, double* cam_pose,
                                double* timestamp, uint8_t* due) {
  REQUIRE_SIM(s);
  if (s->rend.ncam == 0) return fail(RCSH_ERR_STATE, "no render schedule: call rcsh_sim_set_render_schedule first");
  if (slot < 0 || slot >= s->rend.capacity) return fail(RCSH_ERR_ARG, "snapshot slot out of range");
  int which = -1;
  for (int c = 0; c < s->rend.ncam; ++c) which = s->rend_cam_id[c] == cam_id ? c : which;
  if (which < 0) return fail(RCSH_ERR_ARG, "camera is not part of the render schedule");
  const size_t n = (size_t)s->n, nf = (size_t)s->nl + 9;
  // the frames kernel reads "the qpos the last position stage saw" and the box's pre-step pose through field offsets: point
  // it at the record instead of the state
  s->frames_src = s->rend.snap + (size_t)slot * nf * n;
  int rc = rcsh_camera_render_rgb(s, cam_id, rgb, depth_gl, depth_mm, cam_pose);
  s->frames_src = nullptr;
  if (rc) return rc;
  std::vector<double> tm(2 * n);
  HIP_TRY(hipMemcpyAsync(tm.data(), s->frames_src_base(slot) + (size_t)(s->nl + 7) * n, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  std::vector<int32_t> cnt(n);
  HIP_TRY(hipMemcpy(cnt.data(), s->rend.count, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  for (size_t e = 0; e < n; ++e) {
    const bool have = slot < cnt[e] && (((uint32_t)tm[n + e] >> which) & 1u);
    if (timestamp) timestamp[e] = tm[e];
    if (due) due[e] = have ? 1 : 0;
  }
  return RCSH_OK;
}

int rcsh_camera_render_rgb_dev(rcsh_sim* s, int32_t cam_id, uint8_t* rgb, float* depth_gl, uint16_t* depth_mm, double* cam_pose) {
  REQUIRE_SIM(s);
  if (!s->rbuf.frames) return fail(RCSH_ERR_STATE, "no render scene: call rcsh_sim_set_render_scene first");
  if (rgb && !s->rscene.colours) return fail(RCSH_ERR_STATE, "no colours: call rcsh_sim_set_render_colours first");
  if (cam_id < 0 || cam_id >= (int)s->cams.size()) return fail(RCSH_ERR_ARG, "unknown camera id");
  const RenderCam& cam = s->cams[cam_id];
  hipError_t err = hipSuccess;
  bool ok = dispatch_topology(s->narm, s->grip, [&](auto topo) {
    using T = decltype(topo);
    if (s->frames_src)  // a record of the render schedule: qpre at field 0, the box's pre-step pose behind it
      hipLaunchKernelGGL((k_link_frames<T>), dim3(grid_for(s->n)), dim3(kBlock), 0, s->stream, s->d_model.get(), s->frames_src, s->n, 0,
                         T::NL - kBoxPre, (int)s->box.present, s->rbuf.frames.get());
    else
      hipLaunchKernelGGL((k_link_frames<T>), dim3(grid_for(s->n)), dim3(kBlock), 0, s->stream, s->d_model.get(), s->S.get(), s->n,
                         (int)Lay<T>::QPRE, (int)Lay<T>::BOX, (int)s->box.present, s->rbuf.frames.get());
    err = hipGetLastError();
  });
  if (!ok) return fail(RCSH_ERR_MODEL, "no kernel instantiated for this archetype");
  if (err != hipSuccess) return fail(RCSH_ERR_DEVICE, std::string("k_link_frames launch: ") + hipGetErrorString(err));
  hipLaunchKernelGGL(k_shape_frames, dim3(grid_for(s->n * (s->rscene.nshape + 1))), dim3(kBlock), 0, s->stream, s->rscene, cam, s->rbuf.frames.get(), s->n,
                     s->rbuf.wframes.get());
  // (the rays' arithmetic type: float unless rcsh_sim_set_render_f64 asked for the instantiation that equals the restatement bit for bit)
  const dim3 grid((unsigned)(((size_t)render_wgs_per_env(cam.width, cam.height) * (size_t)s->n + 7) / 8 * 8));  // (a multiple of 8: k_render_depth numbers its workgroups per XCD)
  auto cast = [&](auto zero) {
    using F = decltype(zero);
    if (s->rscene.views)
      hipLaunchKernelGGL(k_hull_views<F>, dim3((unsigned)s->n * (unsigned)s->rscene.nshape), dim3(64), 0, s->stream, s->rscene, cam, s->rbuf.wframes.get(), s->n);
    if (rgb)
      hipLaunchKernelGGL((k_render_depth<true, F>), grid, dim3(256), 0, s->stream, s->rscene, cam, s->rbuf.wframes.get(), s->n, depth_gl, depth_mm, cam_pose, rgb);
    else
      hipLaunchKernelGGL((k_render_depth<false, F>), grid, dim3(256), 0, s->stream, s->rscene, cam, s->rbuf.wframes.get(), s->n, depth_gl, depth_mm, cam_pose,
                         (uint8_t*)nullptr);
  };
  if (s->render_f64) cast(0.0); else cast(0.0f);
  err = hipGetLastError();
  if (err != hipSuccess) return fail(RCSH_ERR_DEVICE, std::string("k_render_depth launch: ") + hipGetErrorString(err));
  return RCSH_OK;
}

int rcsh_sim_set_render_f64(rcsh_sim* s, int32_t on) {
  REQUIRE_SIM(s);
  s->render_f64 = on != 0;
  return RCSH_OK;
}

int rcsh_camera_render_dev(rcsh_sim* s, int32_t cam_id, float* depth_gl, uint16_t* depth_mm, double* cam_pose) {
  return rcsh_camera_render_rgb_dev(s, cam_id, nullptr, depth_gl, depth_mm, cam_pose);
}

int rcsh_camera_render_rgb(rcsh_sim* s, int32_t cam_id, uint8_t* rgb, float* depth_gl, uint16_t* depth_mm, double* cam_pose) {
  REQUIRE_SIM(s);
  if (cam_id < 0 || cam_id >= (int)s->cams.size()) return fail(RCSH_ERR_ARG, "unknown camera id");
  const size_t n = (size_t)s->n, px = n * s->cams[cam_id].width * s->cams[cam_id].height;
  StageLayout L;
  const auto dgl = L.out(depth_gl, px);
  const auto dmm = L.out(depth_mm, px);
  const auto dpose = L.out(cam_pose, n * kCamPoseWidth);
  const auto drgb = L.out(rgb, px * kRgbWidth);
  return staged_call(s, s->d_image, L, [&](auto dev) { return rcsh_camera_render_rgb_dev(s, cam_id, dev(drgb), dev(dgl), dev(dmm), dev(dpose)); });
}

int rcsh_camera_render(rcsh_sim* s, int32_t cam_id, float* depth_gl, uint16_t* depth_mm, double* cam_pose) {
  return rcsh_camera_render_rgb(s, cam_id, nullptr, depth_gl, depth_mm, cam_pose);
}

// ---- The all-gather's second carrier: copy engines instead of a collective kernel.
// RCCL's all-gather is a KERNEL (261-280 registers a lane in this image's librccl.so): next to a stepping wavefront of 424 registers it
// finds no SIMD to run on, so on a full batch the gather starts when the env-step ends instead of overlapping it.  Here every rank
// WRITES its block into the receive buffer of each peer (IPC-mapped) with plain asynchronous copies -- SDMA engines over xGMI, one
// stream per peer so the seven links work in parallel -- and says so with an 8-byte copy of the step's sequence number into a flag
// word of the peer.  The only thing that runs on a CU is one single wavefront of 16 registers per gather that waits for the flag words
// (k_wait_flags): it fits beside a stepping wavefront.  Same slot protocol, same entry points for posting and waiting
// (rcsh_comm_allgather_dev / rcsh_comm_wait); the receive buffers belong to the carrier (they have to be exported), see rcs_hip.h.
//   flags[kind][slot][rank]: kind 0 "ack" -- rank says its receive buffer of `slot` is free for sequence number q (its consumer is done
//   with what the buffer held); kind 1 "got" -- rank's block of sequence q has arrived in this rank's receive buffer of `slot`.
namespace {
constexpr int kCopyMaxWorld = 16;
constexpr int kCopySeqRing = 256;
struct CopyBlob {  // what a rank exports (RCSH_COMM_COPY_BLOB_BYTES >= sizeof)
  uint32_t magic, rank;
  uint64_t bytes_per_rank;
  int32_t device, pid;
  hipIpcMemHandle_t recv[2], flags;
};
static_assert(sizeof(CopyBlob) <= RCSH_COMM_COPY_BLOB_BYTES, "the blob fits what the header promises");
}  // namespace
struct CopyCarrier {
  int rank = 0, world = 1;
  size_t bytes = 0;
  DevBuf<void> recv[2];                 // [world * bytes] each, this rank's
  DevBuf<uint64_t> flags;               // [2][2][kCopyMaxWorld], this rank's (fine-grained: peers write it, a waiting wavefront reads it)
  void* peer_recv[kCopyMaxWorld][2] = {};     // views: the peers' receive buffers, IPC-mapped where opened[p] (closed by copy_carrier_free); the own rank's are recv
  uint64_t* peer_flags[kCopyMaxWorld] = {};   // views: the peers' flag words, likewise
  bool opened[kCopyMaxWorld] = {};
  Stream cs[kCopyMaxWorld];             // one copy stream per peer (own rank: the local block)
  Event cs_done[kCopyMaxWorld], acked;
  PinBuf<uint64_t> seq_ring;            // pinned: the sequence numbers the flag copies read
  uint64_t seq[2] = {0, 0};
  int ring_pos = 0;
  PinBuf<uint32_t> timeout_flag;        // pinned: a wait gave up (a peer died)
  bool connected = false;
  // how the flag words are written and waited for: stream memory operations (hipStreamWriteValue64 / hipStreamWaitValue64: the
  // command processor does both, nothing runs on a CU and nothing goes through a copy engine) with RCSH_COPY_CARRIER_FLAGS=value where
  // the device has them; by default an 8-byte copy and the waiting wavefront.
  bool stream_values = false;
  // The whole gather of a slot as ONE captured graph (the default): per post the host records an event, makes the communicator's stream
  // wait for it and launches the graph -- four calls instead of ~5 W + 4.  The sequence number then lives on the device (qdev[slot],
  // bumped by the graph's first node); the flag words are 8-byte device-to-device copies of it, the waiting wavefronts read it.
  bool use_graph = true;
  hipGraphExec_t gexec[2] = {nullptr, nullptr};  // (the graphs are destroyed by hand, first of all: copy_carrier_free)
  hipGraph_t graph[2] = {nullptr, nullptr};
  const void* gsend[2] = {nullptr, nullptr};     // view: the caller's send buffer the slot's graph was captured for
  DevBuf<uint64_t> qdev;                // [2] the slots' sequence numbers (graph form)
};
namespace {
// one wavefront: waits until the `n` words at `w` (skipping index `skip`) have all reached `q`; gives up after ~20 s
__global__ void __launch_bounds__(64) k_wait_flags(const uint64_t* w, int n, int skip, uint64_t q, uint32_t* timeout_flag) {
  const int lane = threadIdx.x;
  const unsigned long long t0 = wall_clock64();
  for (;;) {
    bool ok = true;
    if (lane < n && lane != skip) ok = __hip_atomic_load(w + lane, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) >= q;
    if (__ballot(!ok) == 0) break;
    __builtin_amdgcn_s_sleep(32);
    if (wall_clock64() - t0 > 2000000000ull) {  // (100 MHz constant clock)
      if (lane == 0) __hip_atomic_store(timeout_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      break;
    }
  }
}
// (graph form) the sequence number is read from device memory; the slot's number is bumped by the graph's first node
__global__ void __launch_bounds__(64) k_wait_flags_at(const uint64_t* w, int n, int skip, const uint64_t* qptr, uint32_t* timeout_flag) {
  const int lane = threadIdx.x;
  const uint64_t q = *qptr;
  const unsigned long long t0 = wall_clock64();
  for (;;) {
    bool ok = true;
    if (lane < n && lane != skip) ok = __hip_atomic_load(w + lane, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) >= q;
    if (__ballot(!ok) == 0) break;
    __builtin_amdgcn_s_sleep(32);
    if (wall_clock64() - t0 > 2000000000ull) {
      if (lane == 0) __hip_atomic_store(timeout_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      break;
    }
  }
}
__global__ void k_bump(uint64_t* q) { *q += 1; }
// what has an order: the graphs, then the copy streams run dry, then the peers' mappings closed; the carrier's members do the rest
void copy_carrier_free(CopyCarrier* c) {
  for (int k = 0; k < 2; ++k) {
    if (c->gexec[k]) hipGraphExecDestroy(c->gexec[k]);
    if (c->graph[k]) hipGraphDestroy(c->graph[k]);
  }
  for (int p = 0; p < c->world; ++p) {
    if (c->cs[p]) hipStreamSynchronize(c->cs[p].get());
  }
  for (int p = 0; p < c->world; ++p) {
    if (!c->opened[p]) continue;
    for (int k = 0; k < 2; ++k) if (c->peer_recv[p][k]) hipIpcCloseMemHandle(c->peer_recv[p][k]);
    if (c->peer_flags[p]) hipIpcCloseMemHandle(c->peer_flags[p]);
  }
  delete c;
}
}  // namespace

int rcsh_comm_copy_create(rcsh_sim* s, int32_t rank, int32_t world, size_t bytes_per_rank, uint8_t blob[RCSH_COMM_COPY_BLOB_BYTES]) {
  REQUIRE_SIM(s);
  if (!blob || world < 1 || world > kCopyMaxWorld || rank < 0 || rank >= world || bytes_per_rank == 0 || bytes_per_rank % 8)
    return fail(RCSH_ERR_ARG, "copy carrier: need 0 <= rank < world <= 16 and a block size that is a multiple of 8 bytes");
  if (s->comm.nccl || s->comm.copy) return fail(RCSH_ERR_STATE, "a communicator is already attached to this sim");
  rcsh_sim::Comm cm;  // stream, events and carrier are built here and attached at the end: a failure leaves the handle without any
  CopyCarrier* c = new CopyCarrier;
  cm.copy.reset(c);
  c->rank = rank; c->world = world; c->bytes = bytes_per_rank;
  for (int k = 0; k < 2; ++k) HIP_TRY(hipMalloc(c->recv[k].out(), bytes_per_rank * world));
  // (fine-grained: the words are written by copies other processes start and polled by a wavefront of this one)
  HIP_TRY(hipExtMallocWithFlags((void**)c->flags.out(), sizeof(uint64_t) * 2 * 2 * kCopyMaxWorld, hipDeviceMallocFinegrained));
  HIP_TRY(hipMemset(c->flags.get(), 0, sizeof(uint64_t) * 2 * 2 * kCopyMaxWorld));
  HIP_TRY(hipMalloc(c->qdev.out(), 2 * sizeof(uint64_t)));
  HIP_TRY(hipMemset(c->qdev.get(), 0, 2 * sizeof(uint64_t)));
  if (const char* e = std::getenv("RCSH_COPY_CARRIER_GRAPH")) c->use_graph = std::atoi(e) != 0;
  HIP_TRY(hipHostMalloc(c->seq_ring.out(), sizeof(uint64_t) * kCopySeqRing, hipHostMallocDefault));
  HIP_TRY(hipHostMalloc(c->timeout_flag.out(), sizeof(uint32_t), hipHostMallocDefault));
  *c->timeout_flag.get() = 0;
  HIP_TRY(hipStreamCreateWithFlags(cm.stream.out(), hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(cm.ready.out(), hipEventDisableTiming));
  for (int k = 0; k < 2; ++k) HIP_TRY(hipEventCreateWithFlags(cm.done[k].out(), hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(c->acked.out(), hipEventDisableTiming));
  for (int p = 0; p < world; ++p) {
    HIP_TRY(hipStreamCreateWithFlags(c->cs[p].out(), hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(c->cs_done[p].out(), hipEventDisableTiming));
  }
  {
    // (default: the 8-byte copies and ONE waiting wavefront per wait -- a wait on W - 1 words is W - 1 stream operations, and at 8 ranks the
    // host's calls per gather are what limits this carrier; both ways pass the two-process test and measure the same on one device)
    int can = 0;
    if (hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, s->device) != hipSuccess) can = 0;
    c->stream_values = false;
    if (const char* e = std::getenv("RCSH_COPY_CARRIER_FLAGS")) c->stream_values = can != 0 && std::string(e) == "value";
  }
  CopyBlob b{};
  b.magic = 0x52435348u; b.rank = (uint32_t)rank; b.bytes_per_rank = bytes_per_rank; b.device = s->device; b.pid = (int32_t)getpid();
  for (int k = 0; k < 2; ++k) HIP_TRY(hipIpcGetMemHandle(&b.recv[k], c->recv[k].get()));
  HIP_TRY(hipIpcGetMemHandle(&b.flags, c->flags.get()));
  std::memset(blob, 0, RCSH_COMM_COPY_BLOB_BYTES);
  std::memcpy(blob, &b, sizeof(b));
  cm.rank = rank; cm.world = world;
  s->comm = std::move(cm);
  return RCSH_OK;
}

int rcsh_comm_copy_connect(rcsh_sim* s, const uint8_t* blobs) {
  REQUIRE_SIM(s);
  CopyCarrier* c = s->comm.copy.get();
  if (!c) return fail(RCSH_ERR_STATE, "no copy carrier: call rcsh_comm_copy_create first");
  if (c->connected) return fail(RCSH_ERR_STATE, "the copy carrier is connected already");
  if (!blobs) return fail(RCSH_ERR_ARG, "null blobs");
  for (int p = 0; p < c->world; ++p) {
    CopyBlob b;
    std::memcpy(&b, blobs + (size_t)p * RCSH_COMM_COPY_BLOB_BYTES, sizeof(b));
    if (b.magic != 0x52435348u || (int)b.rank != p || b.bytes_per_rank != c->bytes)
      return fail(RCSH_ERR_ARG, "copy carrier: blob " + std::to_string(p) + " is not rank " + std::to_string(p) + "'s, or the ranks disagree on the block size");
    if (p == c->rank) {
      c->peer_recv[p][0] = c->recv[0].get(); c->peer_recv[p][1] = c->recv[1].get(); c->peer_flags[p] = c->flags.get();
      continue;
    }
    if (b.pid == (int32_t)getpid()) return fail(RCSH_ERR_ARG, "copy carrier: two ranks in one process (IPC handles open in another process only)");
    for (int k = 0; k < 2; ++k) HIP_TRY(hipIpcOpenMemHandle(&c->peer_recv[p][k], b.recv[k], hipIpcMemLazyEnablePeerAccess));
    void* fl = nullptr;
    HIP_TRY(hipIpcOpenMemHandle(&fl, b.flags, hipIpcMemLazyEnablePeerAccess));
    c->peer_flags[p] = (uint64_t*)fl;
    c->opened[p] = true;
  }
  c->connected = true;
  return RCSH_OK;
}

int rcsh_comm_copy_recv_buffer(rcsh_sim* s, int32_t slot, void** recv_dev) {
  REQUIRE_SIM(s);
  if (!s->comm.copy) return fail(RCSH_ERR_STATE, "no copy carrier: call rcsh_comm_copy_create first");
  if (slot < 0 || slot > 1 || !recv_dev) return fail(RCSH_ERR_ARG, "exchange slot is 0 or 1");
  *recv_dev = s->comm.copy.get()->recv[slot].get();
  return RCSH_OK;
}

namespace {
int copy_allgather(rcsh_sim* s, int32_t slot, const void* send_dev, void* recv_dev, size_t bytes_per_rank) {
  CopyCarrier* c = s->comm.copy.get();
  if (!c->connected) return fail(RCSH_ERR_STATE, "copy carrier: call rcsh_comm_copy_connect first");
  if (recv_dev != c->recv[slot].get() || bytes_per_rank != c->bytes)
    return fail(RCSH_ERR_ARG, "copy carrier: the receive buffer of a slot is the carrier's (rcsh_comm_copy_recv_buffer), the block size the one it was created with");
  if (*c->timeout_flag.get()) return fail(RCSH_ERR_DEVICE, "copy carrier: an earlier gather gave up waiting for a peer");
  const int me = c->rank, W = c->world;
  auto flag = [&](uint64_t* base, int kind, int sl, int r) { return base + ((size_t)kind * 2 + sl) * kCopyMaxWorld + r; };
  // after what the handle's stream holds so far: the env-step that wrote the send buffer, the consumer of this slot's last gather
  HIP_TRY(hipEventRecord(s->comm.ready.get(), s->stream));
  HIP_TRY(hipStreamWaitEvent(s->comm.stream.get(), s->comm.ready.get(), 0));
  if (c->use_graph && !c->stream_values) {
    if (c->gexec[slot] && c->gsend[slot] != send_dev) {  // (another send buffer: the copies' source is part of the graph)
      hipGraphExecDestroy(c->gexec[slot]); hipGraphDestroy(c->graph[slot]);
      c->gexec[slot] = nullptr; c->graph[slot] = nullptr;
    }
    if (!c->gexec[slot]) {
      uint64_t* qd = c->qdev.get() + slot;
      hipError_t ge = hipStreamBeginCapture(s->comm.stream.get(), hipStreamCaptureModeThreadLocal);
      auto g = [&](hipError_t e_) { if (ge == hipSuccess) ge = e_; };
      if (ge == hipSuccess) {
        hipLaunchKernelGGL(k_bump, dim3(1), dim3(1), 0, s->comm.stream.get(), qd);
        g(hipGetLastError());
        for (int p = 0; p < W; ++p)
          if (p != me) g(hipMemcpyAsync(flag(c->peer_flags[p], 0, slot, me), qd, sizeof(uint64_t), hipMemcpyDeviceToDevice, s->comm.stream.get()));
        if (W > 1) {
          hipLaunchKernelGGL(k_wait_flags_at, dim3(1), dim3(64), 0, s->comm.stream.get(), flag(c->flags.get(), 0, slot, 0), W, me, qd, c->timeout_flag.get());
          g(hipGetLastError());
        }
        g(hipEventRecord(c->acked.get(), s->comm.stream.get()));
        for (int p = 0; p < W; ++p) {
          g(hipStreamWaitEvent(c->cs[p].get(), c->acked.get(), 0));
          g(hipMemcpyAsync((char*)c->peer_recv[p][slot] + (size_t)me * c->bytes, send_dev, c->bytes, hipMemcpyDeviceToDevice, c->cs[p].get()));
          if (p != me) g(hipMemcpyAsync(flag(c->peer_flags[p], 1, slot, me), qd, sizeof(uint64_t), hipMemcpyDeviceToDevice, c->cs[p].get()));
          g(hipEventRecord(c->cs_done[p].get(), c->cs[p].get()));
          g(hipStreamWaitEvent(s->comm.stream.get(), c->cs_done[p].get(), 0));
        }
        if (W > 1) {
          hipLaunchKernelGGL(k_wait_flags_at, dim3(1), dim3(64), 0, s->comm.stream.get(), flag(c->flags.get(), 1, slot, 0), W, me, qd, c->timeout_flag.get());
          g(hipGetLastError());
        }
        hipGraph_t gr = nullptr;
        const hipError_t ee = hipStreamEndCapture(s->comm.stream.get(), &gr);
        if (ge == hipSuccess) ge = ee;
        if (ge == hipSuccess) ge = hipGraphInstantiate(&c->gexec[slot], gr, nullptr, nullptr, 0);
        if (ge == hipSuccess) { c->graph[slot] = gr; c->gsend[slot] = send_dev; }
        else if (gr) hipGraphDestroy(gr);
      }
      if (ge != hipSuccess) {  // (no graph on this runtime: the calls one by one, below)
        (void)hipGetLastError();
        c->use_graph = false;
        c->gexec[slot] = nullptr;
        if (c->seq[0] || c->seq[1]) return fail(RCSH_ERR_DEVICE, std::string("copy carrier: graph capture failed after gathers had run as graphs: ") + hipGetErrorString(ge));
      }
    }
    if (c->gexec[slot]) {
      ++c->seq[slot];
      HIP_TRY(hipGraphLaunch(c->gexec[slot], s->comm.stream.get()));
      HIP_TRY(hipEventRecord(s->comm.done[slot].get(), s->comm.stream.get()));
      s->comm.pending[slot] = true;
      return RCSH_OK;
    }
  }
  const uint64_t q = ++c->seq[slot];
  uint64_t* qsrc = c->seq_ring.get() + (c->ring_pos++ % kCopySeqRing);
  *qsrc = q;
  auto write_word = [&](hipStream_t st, uint64_t* dst) -> hipError_t {
    if (c->stream_values) return hipStreamWriteValue64(st, dst, q, 0);
    return hipMemcpyAsync(dst, qsrc, sizeof(uint64_t), hipMemcpyHostToDevice, st);
  };
  auto wait_words = [&](hipStream_t st, uint64_t* base) -> hipError_t {  // every peer's word of this rank's flags has reached q
    if (W < 2) return hipSuccess;
    if (c->stream_values) {
      for (int p = 0; p < W; ++p) {
        if (p == me) continue;
        const hipError_t e = hipStreamWaitValue64(st, base + p, q, hipStreamWaitValueGte, ~0ull);
        if (e != hipSuccess) return e;
      }
      return hipSuccess;
    }
    hipLaunchKernelGGL(k_wait_flags, dim3(1), dim3(64), 0, st, base, W, me, q, c->timeout_flag.get());
    return hipGetLastError();
  };
  // 1. tell every peer that this rank's receive buffer of the slot is free for q; wait until every peer has said so
  for (int p = 0; p < W; ++p)
    if (p != me) HIP_TRY(write_word(s->comm.stream.get(), flag(c->peer_flags[p], 0, slot, me)));
  HIP_TRY(wait_words(s->comm.stream.get(), flag(c->flags.get(), 0, slot, 0)));
  HIP_TRY(hipEventRecord(c->acked.get(), s->comm.stream.get()));
  // 2. the block to every peer, each over its own stream (its own link), followed by the word that says it has arrived
  for (int p = 0; p < W; ++p) {
    HIP_TRY(hipStreamWaitEvent(c->cs[p].get(), c->acked.get(), 0));
    HIP_TRY(hipMemcpyAsync((char*)c->peer_recv[p][slot] + (size_t)me * c->bytes, send_dev, c->bytes, hipMemcpyDeviceToDevice, c->cs[p].get()));
    if (p != me) HIP_TRY(write_word(c->cs[p].get(), flag(c->peer_flags[p], 1, slot, me)));
    HIP_TRY(hipEventRecord(c->cs_done[p].get(), c->cs[p].get()));
    HIP_TRY(hipStreamWaitEvent(s->comm.stream.get(), c->cs_done[p].get(), 0));  // (the send buffer is free once these have run)
  }
  // 3. the slot is gathered when every peer's block has arrived here
  HIP_TRY(wait_words(s->comm.stream.get(), flag(c->flags.get(), 1, slot, 0)));
  HIP_TRY(hipEventRecord(s->comm.done[slot].get(), s->comm.stream.get()));
  s->comm.pending[slot] = true;
  return RCSH_OK;
}
}  // namespace


// ---- RCCL behind the C-ABI.  The library is dlopen'ed so that single-GPU users neither link nor load it.
namespace {
struct Rccl {
  typedef struct { char internal[RCSH_COMM_ID_BYTES]; } UniqueId;
  int (*GetUniqueId)(UniqueId*) = nullptr;
  int (*CommInitRank)(void**, int, UniqueId, int) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  void* lib = nullptr;
  std::string why;
};
static Rccl& rccl() {
  static Rccl r;
  if (r.lib || !r.why.empty()) return r;
  for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
    r.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
    if (r.lib) break;
  }
  if (!r.lib) { r.why = std::string("librccl.so not loadable: ") + dlerror(); return r; }
  r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(r.lib, "ncclGetUniqueId");
  r.CommInitRank = (decltype(r.CommInitRank))dlsym(r.lib, "ncclCommInitRank");
  r.AllGather = (decltype(r.AllGather))dlsym(r.lib, "ncclAllGather");
  r.CommDestroy = (decltype(r.CommDestroy))dlsym(r.lib, "ncclCommDestroy");
  r.GetErrorString = (decltype(r.GetErrorString))dlsym(r.lib, "ncclGetErrorString");
  if (!r.GetUniqueId || !r.CommInitRank || !r.AllGather || !r.CommDestroy || !r.GetErrorString) r.why = "librccl.so lacks the collective entry points";
  return r;
}
void rccl_comm_destroy(void* comm) { rccl().CommDestroy(comm); }
#define RCCL_TRY(expr)                                                                                             \
  do {                                                                                                             \
    const int _e = (expr);                                                                                         \
    if (_e != 0) return fail(RCSH_ERR_DEVICE, std::string(#expr) + ": " + rccl().GetErrorString(_e));             \
  } while (0)
}  // namespace

int rcsh_comm_get_unique_id(uint8_t id[RCSH_COMM_ID_BYTES]) {
  if (!id) return fail(RCSH_ERR_ARG, "null id");
  Rccl& r = rccl();
  if (!r.why.empty()) return fail(RCSH_ERR_DEVICE, r.why);
  Rccl::UniqueId u;
  RCCL_TRY(r.GetUniqueId(&u));
  std::memcpy(id, u.internal, RCSH_COMM_ID_BYTES);
  return RCSH_OK;
}

int rcsh_comm_init(rcsh_sim* s, const uint8_t id[RCSH_COMM_ID_BYTES], int32_t rank, int32_t world) {
  REQUIRE_SIM(s);
  if (!id || world < 1 || rank < 0 || rank >= world) return fail(RCSH_ERR_ARG, "communicator: need an id and 0 <= rank < world");
  if (s->comm.nccl) return fail(RCSH_ERR_STATE, "a communicator is already attached to this sim");
  Rccl& r = rccl();
  if (!r.why.empty()) return fail(RCSH_ERR_DEVICE, r.why);
  Rccl::UniqueId u;
  std::memcpy(u.internal, id, RCSH_COMM_ID_BYTES);
  // the communicator, its stream and its events belong to THIS handle's device: a host with one process per GPU that never
  // called hipSetDevice itself (a plain C host has no reason to) must not end up with every rank on device 0
  HIP_TRY(hipSetDevice(s->device));
  // stream and events first: they cannot fail collectively, ncclCommInitRank can only be entered by all ranks or none
  rcsh_sim::Comm cm;  // (attached at the end: a failure leaves the handle without any of it)
  hipError_t he = hipStreamCreateWithFlags(cm.stream.out(), hipStreamNonBlocking);
  if (he == hipSuccess) he = hipEventCreateWithFlags(cm.ready.out(), hipEventDisableTiming);
  for (int k = 0; k < 2 && he == hipSuccess; ++k) he = hipEventCreateWithFlags(cm.done[k].out(), hipEventDisableTiming);
  if (he != hipSuccess) return fail(RCSH_ERR_DEVICE, std::string("communicator stream / events: ") + hipGetErrorString(he));
  void* comm = nullptr;
  if (const int nrc = r.CommInitRank(&comm, world, u, rank))
    return fail(RCSH_ERR_DEVICE, std::string("ncclCommInitRank: ") + (r.GetErrorString ? r.GetErrorString(nrc) : "error ") + " (" + std::to_string(nrc) + ")");
  cm.nccl.reset(comm);
  cm.rank = rank;
  cm.world = world;
  s->comm = std::move(cm);
  return RCSH_OK;
}

int rcsh_comm_rank(const rcsh_sim* s, int32_t* rank, int32_t* world) {
  if (!s) return fail(RCSH_ERR_ARG, "null sim handle");
  if (rank) *rank = s->comm.rank;
  if (world) *world = s->comm.world;
  return RCSH_OK;
}

int rcsh_comm_allgather_dev(rcsh_sim* s, int32_t slot, const void* send_dev, void* recv_dev, size_t bytes_per_rank) {
  REQUIRE_SIM(s);
  if (!s->comm.nccl && !s->comm.copy) return fail(RCSH_ERR_STATE, "no communicator: call rcsh_comm_init (or rcsh_comm_copy_create) first");
  if (!send_dev || !recv_dev) return fail(RCSH_ERR_ARG, "null buffer");
  if (slot < 0 || slot > 1) return fail(RCSH_ERR_ARG, "exchange slot is 0 or 1");
  if (s->comm.copy) return copy_allgather(s, slot, send_dev, recv_dev, bytes_per_rank);
  // after what the handle's stream holds so far (the env-step that wrote the observations), on the communicator's stream
  HIP_TRY(hipEventRecord(s->comm.ready.get(), s->stream));
  HIP_TRY(hipStreamWaitEvent(s->comm.stream.get(), s->comm.ready.get(), 0));
  RCCL_TRY(rccl().AllGather(send_dev, recv_dev, bytes_per_rank, /* ncclInt8 */ 0, s->comm.nccl.get(), s->comm.stream.get()));
  HIP_TRY(hipEventRecord(s->comm.done[slot].get(), s->comm.stream.get()));
  s->comm.pending[slot] = true;
  return RCSH_OK;
}

int rcsh_env_allgather_obs_dev(rcsh_sim* s, int32_t slot, const double* local_obs_dev, double* all_obs_dev) {
  REQUIRE_SIM(s);
  return rcsh_comm_allgather_dev(s, slot, local_obs_dev, all_obs_dev, sizeof(double) * (size_t)s->n * (kObsBase + s->narm));
}

int rcsh_comm_wait(rcsh_sim* s, int32_t slot, int32_t block_host) {
  REQUIRE_SIM(s);
  if (!s->comm.nccl && !s->comm.copy) return fail(RCSH_ERR_STATE, "no communicator: call rcsh_comm_init (or rcsh_comm_copy_create) first");
  if (slot < 0 || slot > 1) return fail(RCSH_ERR_ARG, "exchange slot is 0 or 1");
  if (!s->comm.pending[slot]) return RCSH_OK;
  if (block_host) {
    HIP_TRY(hipEventSynchronize(s->comm.done[slot].get()));
    if (s->comm.copy && *s->comm.copy.get()->timeout_flag.get()) return fail(RCSH_ERR_DEVICE, "copy carrier: gave up waiting for a peer's block (a rank died?)");
    s->comm.pending[slot] = false;  // (a stream-side wait leaves it set: a later host-side wait must still see the event)
  } else {
    // (a stream-side wait cannot see a gather give up while it is in flight; it refuses to order consumers behind a carrier that HAS
    // given up on a peer -- the pinned flag, host-readable at any time: every later wait and post fails until the carrier is rebuilt;
    // advisor, round 5)
    if (s->comm.copy && *s->comm.copy.get()->timeout_flag.get()) return fail(RCSH_ERR_DEVICE, "copy carrier: an earlier gather gave up waiting for a peer's block (a rank died?)");
    HIP_TRY(hipStreamWaitEvent(s->stream, s->comm.done[slot].get(), 0));
  }
  return RCSH_OK;
}

int rcsh_comm_destroy(rcsh_sim* s) {
  REQUIRE_SIM(s);
  if (!s->comm.nccl && !s->comm.copy) return RCSH_OK;
  hipStreamSynchronize(s->comm.stream.get());
  // the one teardown: `gone` is destroyed on return, its members in reverse -- the carrier or the communicator, the events, the stream
  rcsh_sim::Comm gone = std::move(s->comm);
  s->comm = rcsh_sim::Comm{};
  return RCSH_OK;
}


int rcsh_dev_alloc(rcsh_sim* s, size_t bytes, void** ptr) {
  REQUIRE_SIM(s);
  HIP_TRY(hipMalloc(ptr, bytes));
  return RCSH_OK;
}
int rcsh_dev_free(rcsh_sim* s, void* ptr) {
  REQUIRE_SIM(s);
  HIP_TRY(hipFree(ptr));
  return RCSH_OK;
}
int rcsh_dev_upload(rcsh_sim* s, void* dst, const void* src, size_t bytes) {
  REQUIRE_SIM(s);
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return RCSH_OK;
}
int rcsh_dev_download(rcsh_sim* s, void* dst, const void* src, size_t bytes) {
  REQUIRE_SIM(s);
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return RCSH_OK;
}

#ifdef RCSH_CHECK_TAIL
extern "C" int rcsh_debug_check_tail(unsigned long long* out16, int clear) {
  hipDeviceSynchronize();
  if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(rcsh::g_chk_tail), sizeof(unsigned long long) * 16) != hipSuccess) return 1;
  if (clear) { unsigned long long z[16] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(rcsh::g_chk_tail), z, sizeof(z)) != hipSuccess) return 1; }
  return 0;
}
#endif
#ifdef RCSH_WAVE_TIMES
extern "C" int rcsh_debug_wave_times(unsigned long long* out4x4096) {
  hipDeviceSynchronize();
  return hipMemcpyFromSymbol(out4x4096, HIP_SYMBOL(rcsh::g_wave_times), sizeof(unsigned long long) * 4 * 4096) == hipSuccess ? 0 : 1;
}
#endif
#ifdef RCSH_CHECK_TAIL
extern "C" int rcsh_debug_check_hist(unsigned long long* out64, int clear) {
  hipDeviceSynchronize();
  if (hipMemcpyFromSymbol(out64, HIP_SYMBOL(rcsh::g_chk_hist), sizeof(unsigned long long) * 64) != hipSuccess) return 1;
  if (clear) { unsigned long long z[64] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(rcsh::g_chk_hist), z, sizeof(z)) != hipSuccess) return 1; }
  return 0;
}
#endif
#ifdef RCSH_CHECK_DEBUG
extern "C" int rcsh_debug_check(int* out64, int clear) {
  if (hipMemcpyFromSymbol(out64, HIP_SYMBOL(rcsh::g_chk_dbg), sizeof(int) * 64) != hipSuccess) return 1;
  if (clear) { int z[64] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(rcsh::g_chk_dbg), z, sizeof(z)) != hipSuccess) return 1; }
  return 0;
}
extern "C" int rcsh_debug_check_f(double* out128) {
  return hipMemcpyFromSymbol(out128, HIP_SYMBOL(rcsh::g_chk_dbgf), sizeof(double) * 128) != hipSuccess;
}
extern "C" int rcsh_debug_check_cycles(unsigned long long* out16, int clear) {
  hipDeviceSynchronize();
  if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(rcsh::g_chk_cyc), sizeof(unsigned long long) * 16) != hipSuccess) return 1;
  if (clear) { unsigned long long z[16] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(rcsh::g_chk_cyc), z, sizeof(z)) != hipSuccess) return 1; }
  return 0;
}
#endif
#if defined(RCSH_CHECK_DEBUG) || defined(RCSH_PHASE_TIMING)  // (the timing tools name the slack test's example pairs with it: tools/esc_timing.py)
extern "C" int rcsh_debug_check_pairs(rcsh_sim* s, int32_t* g0g1 /* [cap][2] */, int32_t cap, int32_t* n, int32_t* nb) {
  *n = (int)s->tables.chk_pairs.size(); *nb = 0;
  for (int i = 0; i < *n && i < cap; ++i) { g0g1[2 * i] = s->cgeoms[s->tables.chk_pairs[i].g0].geom_id; g0g1[2 * i + 1] = s->cgeoms[s->tables.chk_pairs[i].g1].geom_id; }
  return 0;
}
#endif
#ifdef RCSH_PHASE_TIMING
extern "C" int rcsh_debug_slack(double* out16) {
  hipDeviceSynchronize();
  return hipMemcpyFromSymbol(out16, HIP_SYMBOL(rcsh::g_slack_dbg), sizeof(double) * 16) != hipSuccess;
}
extern "C" int rcsh_debug_team_cycles(unsigned long long* out16 /* 24 slots */) {
  hipDeviceSynchronize();
  return hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_team_cycles), sizeof(unsigned long long) * 24) == hipSuccess ? 0 : 1;
}
extern "C" int rcsh_debug_team_cycles48(unsigned long long* out48) {
  hipDeviceSynchronize();
  return hipMemcpyFromSymbol(out48, HIP_SYMBOL(g_team_cycles), sizeof(unsigned long long) * 48) == hipSuccess ? 0 : 1;
}
extern "C" int rcsh_debug_team_cycles96(unsigned long long* out96, int clear_max) {
  hipDeviceSynchronize();
  if (hipMemcpyFromSymbol(out96, HIP_SYMBOL(g_team_cycles), sizeof(unsigned long long) * 96) != hipSuccess) return 1;
  if (clear_max) {  // (the maxima are per window)
    unsigned long long z = 0;
    hipMemcpyToSymbol(HIP_SYMBOL(g_team_cycles), &z, sizeof(z), sizeof(z) * 66);
    hipMemcpyToSymbol(HIP_SYMBOL(g_team_cycles), &z, sizeof(z), sizeof(z) * 68);
  }
  return 0;
}
extern "C" int rcsh_debug_round_hist(unsigned long long* out4) {  // hull rounds with 1, 2, 3, 4 pairs since the library was loaded
  hipDeviceSynchronize();
  return hipMemcpyFromSymbol(out4, HIP_SYMBOL(g_round_hist), sizeof(unsigned long long) * 4) == hipSuccess ? 0 : 1;
}
extern "C" int rcsh_debug_team_cycles64(unsigned long long* out64) {
  hipDeviceSynchronize();
  return hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_team_cycles), sizeof(unsigned long long) * 64) == hipSuccess ? 0 : 1;
}
#endif

int rcsh_debug_dump_model(rcsh_sim* s, void* buf, size_t cap, size_t* size) {
  REQUIRE_SIM(s);
  if (size) *size = sizeof(DevModel);
  if (buf && cap >= sizeof(DevModel)) std::memcpy(buf, &s->dm, sizeof(DevModel));
  return RCSH_OK;
}

int rcsh_prof_enable(rcsh_sim* s, int32_t enable) {
  REQUIRE_SIM(s);
  if (enable && s->ev_start.empty()) {
    std::vector<Event> start(kProfRing), stop(kProfRing);  // (attached when all of them exist)
    for (int i = 0; i < kProfRing; ++i) {
      HIP_TRY(hipEventCreate(start[i].out()));
      HIP_TRY(hipEventCreate(stop[i].out()));
    }
    s->ev_start = std::move(start);
    s->ev_stop = std::move(stop);
  }
  s->prof = enable != 0;
  s->prof_region = enable < 0;
  s->prof_region_launches = 0;
  s->prof_every = enable > 1 ? enable : 1;
  s->prof_seen = 0;
  s->prof_pending = 0; s->prof_ms = 0; s->prof_launches = 0;
  return RCSH_OK;
}
int rcsh_prof_read(rcsh_sim* s, double* total_ms, int64_t* launches) {
  REQUIRE_SIM(s);
  if (s->prof_region) {
    float ms = 0.f;
    if (s->prof_region_launches > 0) {
      HIP_TRY(hipEventRecord(s->ev_stop[0].get(), s->stream));
      HIP_TRY(hipEventSynchronize(s->ev_stop[0].get()));
      HIP_TRY(hipEventElapsedTime(&ms, s->ev_start[0].get(), s->ev_stop[0].get()));
    }
    if (total_ms) *total_ms = ms;
    if (launches) *launches = s->prof_region_launches;
    s->prof_region_launches = 0;
    return RCSH_OK;
  }
  int rc = prof_flush(s);
  if (rc) return rc;
  if (total_ms) *total_ms = s->prof_ms;
  if (launches) *launches = s->prof_launches;
  return RCSH_OK;
}

}  // extern "C"
