// collision_tables_main.cpp -- runs the collision-table builder (csrc/model.cpp: build_collision_tables) and the queries' pair-set
// builder (build_query_pairs, for kinds = 1, 2, 4, 7) on one scene, on the CPU, and prints the tables as JSON (tests/test_collision_tables_cpu.py).  The scene is model.inc, written by tools/export_model_c.py:
//
//   python tools/export_model_c.py scene.xml > model.inc
//   g++ -std=c++17 -I. -I<csrc> collision_tables_main.cpp <csrc>/model.cpp -o collision_tables && ./collision_tables
#include <cstdio>
#include <cstring>

#include "model_host.h"

#include "model.inc"

using namespace rcsh;

namespace {

void arr(const char* name, const double* v, int n, const char* end = ",\n") {
  std::printf("\"%s\": [", name);
  for (int i = 0; i < n; ++i) std::printf("%s%.17g", i ? ", " : "", v[i]);
  std::printf("]%s", end);
}
void pairs_json(const char* name, const std::vector<SelfPair>& v) {
  std::printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); ++i)
    std::printf("%s[%d, %d, %d, %d, %d, %d]", i ? ", " : "", v[i].g0, v[i].g1, v[i].l0, v[i].l1, v[i].cls, v[i].joints);
  std::printf("],\n");
}

}  // namespace

int main() {
  rcsh_model_desc d;
  std::memset(&d, 0, sizeof(d));
  fill_model(&d);
  HostModel hm;
  hm.copy_from(d);
  DevModel dm;
  std::memset(&dm, 0, sizeof(dm));
  std::vector<int> act_slot;
  std::string why = finalize_model(hm, dm, act_slot);
  if (!why.empty()) { std::fprintf(stderr, "finalize_model: %s\n", why.c_str()); return 1; }
  CollisionPoints cp;
  why = build_collision_points(hm, cp);
  if (!why.empty()) { std::fprintf(stderr, "build_collision_points: %s\n", why.c_str()); return 1; }
  std::vector<ContactGeom> cgeoms;
  std::vector<double> cverts;
  std::string overflow;
  why = build_contact_table(hm, dm, cp.has_plane ? cp.plane_geom : -1, cgeoms, cverts, overflow);
  if (!why.empty() || !overflow.empty()) { std::fprintf(stderr, "build_contact_table: %s%s\n", why.c_str(), overflow.c_str()); return 1; }
  // the class bits, as rcsh_sim_add_robot and rcsh_sim_add_gripper (csrc/rcs_hip.hip) set them
  auto mark = [&](const int32_t* ids, int n, int bit) {
    for (int c = 0; c < n; ++c)
      for (auto& cg : cgeoms)
        if (cg.geom_id == ids[c]) cg.cls |= bit;
  };
  mark(m_arm_geoms, N_ARM_GEOMS, 1);
  mark(m_gripper_geoms, N_GRIPPER_GEOMS, 16);
  for (int c = 0; c < N_GRIPPER_GEOMS; ++c) {
    bool ignored = false;
    for (int q = 0; q < N_IGNORED_GEOMS; ++q) ignored = ignored || m_ignored_geoms[q] == m_gripper_geoms[c];
    if (!ignored) mark(&m_gripper_geoms[c], 1, 2);
  }
  mark(m_finger_geoms, N_FINGER_GEOMS, 4);
  mark(m_ignored_geoms, N_IGNORED_GEOMS, 8);

  CollisionTables t;
  build_collision_tables(hm, dm, cp, cgeoms, cverts, t);

  const int ng = (int)cgeoms.size();
  std::printf("{\"narm\": %d, \"nl\": %d, \"lever_slack\": %.17g, \"stage_verts\": %d, \"max_check_pairs\": %d, \"lev_geom\": %d,\n", dm.narm, dm.nl,
              kLeverSlack, kSelfStageVertsHost, kMaxCheckPairs, kLevGeom);
  std::printf("\"jtype\": [");
  for (int j = 0; j < dm.nl; ++j) std::printf("%s%d", j ? ", " : "", dm.jtype[j]);
  std::printf("],\n");
  arr("range", &dm.range[0][0], 2 * dm.nl);
  arr("qpos0", dm.qpos0, dm.nl);
  std::printf("\"geoms\": [\n");
  for (int g = 0; g < ng; ++g) {
    const ContactGeom& cg = cgeoms[g];
    const GeomBox bx = geom_box(cg);
    std::printf("{\"geom_id\": %d, \"link\": %d, \"type\": %d, \"cls\": %d, \"vert_adr\": %d, \"vert_num\": %d, ", cg.geom_id, cg.link, cg.type, cg.cls,
                cg.vert_adr, cg.vert_num);
    arr("pos", cg.pos, 3, ", "); arr("rot", cg.rot, 9, ", "); arr("size", cg.size, 3, ", ");
    arr("box_c", bx.c, 3, ", "); arr("box_h", bx.h, 3, ", "); arr("box_rot", bx.rot, 9, ", ");
    arr("gh", t.chk.gh[g], 3, ", "); arr("chk_c", t.chk_geoms[g].c, 3, ", "); arr("chk_rot", t.chk_geoms[g].rot, 9, "");
    std::printf(", \"glink\": %d, \"gtype\": %d}%s\n", t.chk.glink[g], t.chk.gtype[g], g + 1 < ng ? "," : "");
  }
  std::printf("],\n\"never_touch\": [");
  bool first = true;
  for (int i = 0; i < ng; ++i)
    for (int j = i + 1; j < ng; ++j)
      if (never_touch_across_first_hinge(dm, cverts, cgeoms[i], cgeoms[j])) {
        std::printf("%s[%d, %d]", first ? "" : ", ", cgeoms[i].geom_id, cgeoms[j].geom_id);
        first = false;
      }
  std::printf("],\n");
  pairs_json("pairs", t.pairs);  // [g0, g1, l0, l1, cls, joints]; g0 / g1 index "geoms"
  pairs_json("chk_pairs", t.chk_pairs);
  std::printf("\"chk_ent\": [");  // [g0, g1, 1 + common ancestor link, rsum]
  for (size_t i = 0; i < t.chk_ent.size(); ++i) {
    const uint32_t e = t.chk_ent[i].geoms;
    std::printf("%s[%u, %u, %u, %.9g]", i ? ", " : "", e & 255u, (e >> 8) & 255u, (e >> 16) & 255u, (double)t.chk_ent[i].rsum);
  }
  std::printf("],\n\"chk_unchecked\": %d, \"ctab_npair\": %d, \"chk_npair\": %d, \"chk_ngeom\": %d,\n", t.chk_unchecked, t.ctab.npair, t.chk.npair, t.chk.ngeom);
  // the queries' pair set (build_query_pairs) per kinds mask, as for a scene whose free body is geom `ngeom` (rcsh_sim_add_free_box: the
  // scene's last geom, split off the articulated tables)
  std::printf("\"plane_geom\": %d, \"box_geom\": %d, \"query_pairs\": {", cp.has_plane ? cp.plane_geom : -1, hm.ngeom);
  for (int kinds : {1, 2, 4, 7}) {
    const QueryPairs P = build_query_pairs(hm, cp, cgeoms, t.chk_pairs, hm.ngeom, kinds);
    std::printf("%s\"%d\": {\"floor_bits\": %u, \"box_bits\": %u, \"ids\": [", kinds == 1 ? "" : ", ", kinds, P.floor_bits, P.box_bits);
    for (int i = 0; i < P.count(); ++i) std::printf("%s[%d, %d]", i ? ", " : "", P.ids[2 * i], P.ids[2 * i + 1]);
    std::printf("]}");
  }
  std::printf("},\n");
  arr("self_lever", t.ctab.self_lever, 12);
  std::vector<double> lev(t.link_lever, t.link_lever + sizeof(t.link_lever) / sizeof(float));
  arr("link_lever", lev.data(), (int)lev.size(), "}\n");
  return 0;
}
