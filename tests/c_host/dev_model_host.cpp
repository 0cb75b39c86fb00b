// A stand-alone host of csrc/dev_model.h (no libmpcr, nothing launched, no
// GPU opened): reads packed model blobs (mpcr_model_t, .mpcrm), compiles each
// one's device model and tables with the default options and writes
// <blob>.dev: int32 sizeof(DevModel), int32 wide; the DevModel bytes with the
// pointer fields zeroed; then the tables, each as an int64 element count and
// its raw elements (hull_vert, hull_info, hull_adjv, hull_head, hull_lut,
// face_plane, face_vinfo, vert_finfo, cone_cell, cone_face).  A refused model
// prints "REFUSED <blob> <code> <message>" and writes no file.  --layout
// prints "name offset bytes type" of the DevModel fields the test reads.
// Built with the address and undefined-behaviour sanitizers and run by
// tests/test_dev_model.py.
//   dev_model_host --layout | <model.mpcrm>...
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../manipulator_mujoco_amd/csrc/dev_model.h"

using namespace mpcr;

#define FIELDS(X)                                                                                                      \
  X(nbody, i) X(njnt, i) X(nq, i) X(nv, i) X(ngeom, i) X(npair, i) X(neq, i) X(nslot, i) X(nctrl, i) X(ntree, i)       \
  X(hande_body, i) X(tcp_body, i) X(disableflags, i) X(jump_rounds, i) X(nu, i) X(neqrow, i) X(integrator, i)          \
  X(has_spring, i) X(cvx_base, i) X(coll_rows, i) X(cvx_joint, i) X(w2_lead_max, i) X(timestep, f)                     \
  X(body_kind, i) X(body_anc, i) X(body_jnt, i) X(body_tree, i) X(body_dofmask, u) X(body_submask, u)                  \
  X(body_bpos, f) X(body_bquat, f) X(body_ipos, f) X(body_mass, f) X(tree_mass, f)                                     \
  X(jnt_type, i) X(jnt_qposadr, i) X(jnt_dofadr, i) X(jnt_body, i) X(jnt_limited, i) X(jnt_pos, f) X(jnt_axis, f)      \
  X(jnt_range, f) X(jnt_margin, f) X(jnt_qpos0, f)                                                                     \
  X(dof_body, i) X(dof_jnt, i) X(dof_kind, i) X(dof_sub, i) X(dof_chainmask, u) X(dof_submask, u) X(blk_n, i)          \
  X(blane_dof, i) X(mc_n, i) X(mc_c0, i) X(dof_invweight0, f)                                                          \
  X(geom_body, i) X(geom_type, i) X(geom_pos, f) X(geom_quat, f) X(geom_size, f)                                       \
  X(pair_g1, i) X(pair_g2, i) X(pair_func, i) X(pair_jinfo, i) X(pair_condim, i) X(pair_friction, f)                   \
  X(pair_margin, f) X(pair_diag, f) X(pair_cmu, f)                                                                     \
  X(eq_type, i) X(eq_j1, i) X(eq_j2, i) X(eq_b1, i) X(eq_b2, i) X(eq_data, f) X(eq_diag, f) X(eqrow_eq, i)             \
  X(eqrow_k, i) X(geom_hulladr, i) X(geom_hullnum, i) X(geom_lutadr, i) X(geom_faceadr, i) X(geom_facenum, i)          \
  X(geom_coneadr, i)

template <class T>
static bool put(FILE* o, const std::vector<T>& v) {
  const int64_t n = (int64_t)v.size();
  return fwrite(&n, sizeof(n), 1, o) == 1 && (n == 0 || fwrite(v.data(), sizeof(T), v.size(), o) == v.size());
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "--layout")) {
#define X(name, type) printf(#name " %zu %zu " #type "\n", offsetof(DevModel, name), sizeof(DevModel::name));
    FIELDS(X)
#undef X
    return 0;
  }
  for (int a = 1; a < argc; a++) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 3; }
    std::vector<mpcr_model_t> m(1);
    const size_t got = fread(m.data(), 1, sizeof(mpcr_model_t), f);
    fclose(f);
    if (got != sizeof(mpcr_model_t) || m[0].magic != MPCR_MODEL_MAGIC || m[0].version != MPCR_MODEL_VERSION) {
      fprintf(stderr, "%s is not a v%d model blob\n", argv[a], MPCR_MODEL_VERSION);
      return 4;
    }
    std::vector<DevModel> d(1);
    DevTables t;
    std::string err;
    if (int rc = compile_dev_model(m[0], DevOptions(), d[0], t, err)) {
      printf("REFUSED %s %d %s\n", argv[a], rc, err.c_str());
      continue;
    }
    const int32_t head[2] = {(int32_t)sizeof(DevModel), (int32_t)needs_wide(m[0], d[0])};
    d[0].hull_vert = d[0].hull_adjv = d[0].hull_lut = d[0].hull_head = d[0].face_plane = nullptr;
    d[0].hull_info = d[0].face_vinfo = d[0].vert_finfo = d[0].cone_cell = nullptr;
    d[0].face_vert = d[0].vert_face = d[0].cone_face = nullptr;
    d[0].prof = nullptr;
    const std::string out = std::string(argv[a]) + ".dev";
    FILE* o = fopen(out.c_str(), "wb");
    if (!o || fwrite(head, sizeof(head), 1, o) != 1 || fwrite(d.data(), sizeof(DevModel), 1, o) != 1 ||
        !put(o, t.hull_vert) || !put(o, t.hull_info) || !put(o, t.hull_adjv) || !put(o, t.hull_head) ||
        !put(o, t.hull_lut) || !put(o, t.face_plane) || !put(o, t.face_vinfo) || !put(o, t.vert_finfo) ||
        !put(o, t.cone_cell) || !put(o, t.cone_face))
      return 6;
    fclose(o);
    printf("%s nbody=%d ngeom=%d wide=%d\n", argv[a], d[0].nbody, d[0].ngeom, head[1]);
  }
  return 0;
}
