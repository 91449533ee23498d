// model_host.h -- host-side copy of the scene tables and the finalisation entry points.
#pragma once
#include <string>
#include <vector>

#include "../../include/rcs_hip.h"
#include "contact_types.h"
#include "dyn.h"
#include "model.h"

namespace rcsh {

// Deep copy of rcsh_model_desc (the caller's arrays need not outlive rcsh_sim_create).
struct HostModel {
  int nbody = 0, njnt = 0, nu = 0, ntendon = 0, nwrap = 0, neq = 0, nsite = 0;
  double timestep = 0.002;
  double gravity[3] = {0, 0, -9.81};
  std::vector<int32_t> body_parentid, body_jntadr, body_jntnum;
  std::vector<double> body_pos, body_quat, body_ipos, body_iquat, body_mass, body_inertia, body_gravcomp;
  std::vector<int32_t> jnt_type, jnt_bodyid, jnt_limited, jnt_actfrclimited, jnt_actgravcomp;
  std::vector<double> jnt_pos, jnt_axis, jnt_range, jnt_margin, jnt_solref, jnt_solimp, jnt_actfrcrange;
  std::vector<double> dof_armature, dof_damping, dof_frictionloss, dof_solref, dof_solimp, qpos0;
  std::vector<int32_t> tendon_adr, tendon_num, wrap_objid;
  std::vector<double> wrap_prm;
  std::vector<int32_t> eq_obj1id, eq_obj2id, eq_active0;
  std::vector<double> eq_data, eq_solref, eq_solimp;
  std::vector<int32_t> actuator_trntype, actuator_trnid, actuator_biastype, actuator_ctrllimited, actuator_forcelimited;
  std::vector<double> actuator_gear, actuator_gainprm, actuator_biasprm, actuator_ctrlrange, actuator_forcerange;
  std::vector<int32_t> site_bodyid;
  std::vector<double> site_pos, site_quat;
  int ngeom = 0, nmeshvert = 0;
  std::vector<int32_t> geom_type, geom_bodyid, geom_contype, geom_conaffinity, geom_vertadr, geom_vertnum;
  std::vector<double> geom_pos, geom_quat, geom_size, geom_friction, mesh_vert;
  void copy_from(const rcsh_model_desc& d);
};

// Contact detection tables: sample points (hull vertices, box corners, capsule / sphere centres with a radius) of
// every collision geom riding on a moving link, in link coordinates, tested against the scene's static plane.
struct CollisionPoints {
  std::vector<double> xyzr;       // [npts][4]
  std::vector<int32_t> geom;      // [npts] geom id the point belongs to
  std::vector<int32_t> link_adr;  // [nl + 1] points of link i are [link_adr[i], link_adr[i+1])
  std::vector<double> link_sphere;  // [nl][4] bounding sphere (centre, radius) of link i's points, link frame
  std::vector<double> link_aabb;    // [nl][6] bounding box of link i's points (radii included), link frame: centre, half extents
  bool has_plane = false;
  int plane_geom = -1;
  double plane_n[3] = {0, 0, 1};
  double plane_d = 0;             // plane: n . x = d
};
std::string build_collision_points(const HostModel& h, CollisionPoints& out);

// The robot's collision geoms for the contact phase (contact_team.h), in geom order; `verts` are the hull vertices they
// index (geom frame).  Class bits are filled in later from the SimRobot / SimGripper configurations.
std::string build_contact_table(const HostModel& h, const DevModel& m, int plane_geom, std::vector<ContactGeom>& geoms, std::vector<double>& verts,
                                std::string& overflow /* geoms left out of the table because of a capacity limit: why (empty: none) */,
                                std::vector<int>* dropped = nullptr /* their mjModel geom ids */);

// ---- collision tables: everything the kernels' collision tests read that is fixed between two changes of the geoms' class bits.
// Pure functions of the model -- no device, no environment variable -- so that the bounds the certificate rests on can be tested on a CPU
// (tests/test_collision_tables_cpu.py).

// link i's parent: i - 1 along the arm; both fingers hang off the arm's last link; -1: the world
inline int parent_link(int link, int narm) { return link < narm ? link - 1 : narm - 1; }

// A collision geom's bounding box in the frame of its link (the world's, for a geom welded to it): centre, half extents along the
// geom's axes, and those axes (the geom's frame in the link's, row-major).  Hull: the box of its vertices; box: its size; capsule:
// (r, r, r + half length).  THE rule: the pair records, the check's per-geom tables, the levers and the static geoms' world box use it.
struct GeomBox {
  double c[3], h[3], rot[9];
};
GeomBox geom_box(const ContactGeom& g);

constexpr int kSelfStageVertsHost = 304;  // contact_team.h: kSelfStageVerts (device code; rcs_hip.hip asserts that the two agree)
// The additive slack of every hinge lever (metres per radian, on top of the 1 % factor).  A chain from a hinge to a geom holds at most
// one slide, whose stroke the lever includes: so the levers also hold for a slide up to kLeverSlack PAST its stroke.  The collision
// guard leans on that (rcs_hip.hip guard_launch: kGuardSlideTol).
constexpr double kLeverSlack = 1e-3;

struct CollisionTables {
  std::vector<SelfPair> pairs;        // the admitted geom pairs a collision callback reacts to (cls != 0): the contact phase's self-collision pairs
  std::vector<SelfPair> chk_pairs;    // ALL admitted geom pairs, by body pair, at most kMaxCheckPairs of them ...
  std::vector<CheckEntry> chk_ent;    // ... and their packed entries (CheckTable::ent)
  std::vector<CheckGeom> chk_geoms;   // the geoms' boxes in their links' frames (CheckTable::geoms)
  int chk_unchecked = 0;              // admitted pairs past kMaxCheckPairs: neither checked at the end of a launch nor resolved as self contacts
  float link_lever[kLevGeom + 12 * 32] = {0};  // CheckTable::lev: [joint][link], then per GEOM [joint][geom] (kLevGeom)
  // The launch-invariant contents of Params::coll / ctab / chk (every byte defined, pointers null).  The launch fills in the device
  // pointers, ctab.ngeom, ctab.plane_mu and chk.pad.  ctab.self_lever holds the per-joint levers (no second copy of them).
  CollTable coll;
  ContactTable ctab;
  CheckTable chk;
};
// A scene without collision geoms gets the sample points' part of `coll` and the plane alone: no pairs, levers zero.
void build_collision_tables(const HostModel& h, const DevModel& m, const CollisionPoints& cp, const std::vector<ContactGeom>& cgeoms,
                            const std::vector<double>& cverts, CollisionTables& out);
// the pieces, for the tests: is the pair (a geom welded to the world, a geom of the arm's first link) out of reach in every pose?
bool never_touch_across_first_hinge(const DevModel& m, const std::vector<double>& cverts, const ContactGeom& a, const ContactGeom& b);

// The pairs the collision and clearance queries cover for `kinds` (kQueryFloor | kQuerySelf | kQueryBox), THE definition: the kernels
// test floor_bits / box_bits (QueryArgs) and the check's table, rcsh_clearance_pairs reports `ids`, a pair mask is indexed by it.
// Order: the floor pairs in geom order (geoms the plane admits, on a link, solid: a hull without vertices reports nothing), chk_pairs
// as the table lists them, the free body's pairs in geom order (solid geoms whose contype / conaffinity meets the box's, 1).  ids are
// mjModel geom ids in MuJoCo's order within a contact: the free box (a box) before a hull, after a capsule, after a robot box.
// A group `kinds` leaves out, or whose plane / free body (box_geom < 0) the scene lacks, is empty and its bits are 0.
struct QueryPairs {
  std::vector<int32_t> ids;  // [count][2]
  uint32_t floor_bits = 0, box_bits = 0;  // bit g: table geom g is in the first / the last group
  int count() const { return (int)ids.size() / 2; }
};
// with_ids false: the bits alone (what a launch needs; no list is built).
QueryPairs build_query_pairs(const HostModel& h, const CollisionPoints& cp, const std::vector<ContactGeom>& cgeoms,
                             const std::vector<SelfPair>& chk_pairs, int box_geom, int kinds, bool with_ids = true);

// Edges of the convex polytope { x : n_i . x <= d_i } a drawn hull is given as (render.h: the ray caster finds a hull's outline
// as seen from the camera among them).  Each edge: the two planes that meet in it and its end points.  `centre`: a point
// inside (the mean of the polytope's vertices).  false: the planes do not bound a polytope this routine can vouch for
// (fewer than 4 faces, unbounded, or Euler's formula V - E + F = 2 fails on what it found) -- the caller draws the hull
// without the outline then.
struct HullEdge {
  int32_t a, b;
  double v1[3], v2[3];
};
bool build_hull_edges(const double* planes, int nplanes, std::vector<HullEdge>& edges, double centre[3]);

// Calls fn(Topo<NARM, GRIP>{}) for the compiled archetype matching (narm, grip); false if none does.
template <class F>
bool dispatch_topology(int narm, bool grip, F&& fn) {
#ifdef RCSH_DEV_ONLY_XARM7  // (development builds: the 7-dof arm without gripper alone)
  if (narm == 7 && !grip) { fn(Topo<7, false>{}); return true; }
  return false;
#endif
  if (narm == 7 && grip) { fn(Topo<7, true>{}); return true; }
#ifndef RCSH_DEV_ONLY_FR3  // (development builds define it: the FR3 + hand archetype alone, minutes -> seconds)
  if (narm == 7 && !grip) { fn(Topo<7, false>{}); return true; }
  if (narm == 6 && !grip) { fn(Topo<6, false>{}); return true; }
  if (narm == 5 && grip) { fn(Topo<5, true>{}); return true; }
#endif
  return false;
}

// solimp / solref in the kernels' form (mj_makeImpedance's clamps; time constant floored at 2 timesteps)
Imp make_imp(const double* solimp);
void make_kb(const double* solref, const double* solimp, double timestep, double& K, double& B);

// Returns "" on success, else the reason the scene is rejected.  act_slot[u] = ctrl slot of mj actuator u.
std::string finalize_model(const HostModel& h, DevModel& m, std::vector<int>& act_slot);
std::string attach_robot_frames(const HostModel& h, DevModel& m, int site, int base_body);

}  // namespace rcsh
