// A stand-alone host of what csrc/dev_model.h and csrc/rollout.h hold for the
// static geom poses as a call input (no libmpcr, nothing launched, no GPU
// opened).  For every packed model blob (mpcr_model_t, .mpcrm) named on the
// command line it checks
//   - model_geom_poses(): the rows of static geoms are, bit for bit, what
//     build_dev_model puts into DevModel::geom_pos / geom_quat (x y z 0 | qw
//     qx qy qz), a moving geom's row is 0 0 0 0 | 1 0 0 0, the count is
//     DevModel::ngeom;
//   - is_static and the id map against geom_bodyid / body_weldid, and against
//     DevModel::geom_body;
//   - every output is nullable and the count does not depend on them;
//   - a copy with one static geom moved ((0.05, -0.04, 0.02) m, yaw 0.3 rad in
//     its body's frame) gives another row for that geom, the same bits in
//     every other row, and still the device model's bits;
//   - has_state() is true for a geom-pose pointer alone
// and prints one "OK <blob> ngeom=.. nstatic=.." line, or "FAIL <blob>: why"
// with exit status 1.  --layout prints "name offset bytes" of DevModel fields,
// "sizeof <bytes>" and "stateargs <bytes>".  Built with the address and
// undefined-behaviour sanitizers and run by tests/test_geom_pose_lib.py.
//   geom_pose_host --layout | <model.mpcrm>...
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../manipulator_mujoco_amd/csrc/dev_model.h"
#include "../../manipulator_mujoco_amd/csrc/rollout.h"

using namespace mpcr;

static_assert(sizeof(StateArgs) == 56, "StateArgs: 56 of par's 80 bytes");
static_assert(offsetof(StateArgs, ctrl) == 32 && offsetof(StateArgs, geom_pose) == 40 &&
                  offsetof(StateArgs, geom_stride) == 48 && offsetof(StateArgs, geom_step_stride) == 52,
              "the geom-pose fields follow ctrl");

#define FIELDS(X)                                                                                                      \
  X(nbody) X(nu) X(integrator) X(timestep) X(body_kind) X(body_mass) X(jnt_type) X(jnt_qpos0) X(dof_body) X(mc_c0)     \
  X(dof_invweight0) X(qpos_init) X(geom_body) X(geom_rbound) X(pair_g1) X(pair_jinfo) X(pair_diag) X(eq_type)          \
  X(eqrow_k) X(dof_stiffness) X(dof_actfrc) X(act_ntrn) X(act_moment) X(act_gain) X(act_bias) X(act_frc) X(impl_D)     \
  X(geom_hulladr) X(hull_vert) X(hull_head) X(geom_faceadr) X(face_plane) X(cone_face) X(ctrl_qposadr) X(cone)         \
  X(pair_cmu) X(body_visc) X(ten_body) X(ten_pos) X(ten_invw) X(act_ctrlrange) X(geom_pos) X(geom_quat)

static int fail(const char* blob, const std::string& why) {
  printf("FAIL %s: %s\n", blob, why.c_str());
  return 1;
}

static bool compile(const mpcr_model_t& m, std::vector<DevModel>& d, std::string& err) {
  DevTables t;
  d.assign(1, DevModel());
  return compile_dev_model(m, DevOptions(), d[0], t, err) == 0;
}

struct Rows {
  int ng = 0;
  std::vector<float> block;
  std::vector<int> id, fixed;
};

static bool rows_of(const mpcr_model_t& m, Rows& r) {
  r.ng = model_geom_poses(m, nullptr, nullptr, nullptr);
  if (r.ng < 0) return false;
  r.block.assign(8 * (size_t)r.ng + 1, -7.f);  // one guard float behind the block
  r.id.assign(r.ng + 1, -7);
  r.fixed.assign(r.ng + 1, -7);
  return model_geom_poses(m, r.block.data(), r.id.data(), r.fixed.data()) == r.ng;
}

// the block's static rows against the device model's arrays, bit for bit
static std::string against_dev(const mpcr_model_t& m, const Rows& r, const DevModel& d) {
  if (r.ng != d.ngeom) return "count " + std::to_string(r.ng) + " != DevModel::ngeom " + std::to_string(d.ngeom);
  if (r.block[8 * (size_t)r.ng] != -7.f || r.id[r.ng] != -7 || r.fixed[r.ng] != -7) return "wrote past ngeom rows";
  for (int i = 0; i < r.ng; i++) {
    const float* row = &r.block[8 * (size_t)i];
    const int g = r.id[i];
    const std::string at = " (row " + std::to_string(i) + ")";
    if (g < 0 || g >= m.ngeom) return "model geom id out of range" + at;
    const int b = m.geom_bodyid[g];
    const bool fixed = b == 0 || m.body_weldid[b] == 0;  // welded to the world: no joint up the chain
    if ((r.fixed[i] != 0) != fixed) return "is_static disagrees with body_weldid" + at;
    if ((d.geom_body[i] < 0) != fixed) return "is_static disagrees with DevModel::geom_body" + at;
    if (d.geom_type[i] != m.geom_type[g]) return "the id map does not name the device model's geom" + at;
    if (fixed) {
      const float zero = 0.f;
      if (memcmp(row, d.geom_pos[i], 12) || memcmp(row + 3, &zero, 4) || memcmp(row + 4, d.geom_quat[i], 16))
        return "static row differs from geom_pos / geom_quat" + at;
      const double n = sqrt((double)row[4] * row[4] + (double)row[5] * row[5] + (double)row[6] * row[6] +
                            (double)row[7] * row[7]);
      if (fabs(n - 1.0) > 1e-6) return "static row's quaternion is not unit" + at;
    } else {
      const float want[8] = {0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
      if (memcmp(row, want, sizeof(want))) return "moving geom's row is not 0 0 0 0 | 1 0 0 0" + at;
    }
  }
  // the map is a bijection onto the geoms the pairs name
  int gmap[MPCR_MAX_GEOM];
  if (pair_geom_map(m, gmap) != r.ng) return "pair_geom_map count";
  for (int i = 0; i < r.ng; i++)
    if (gmap[r.id[i]] != i) return "id map is not pair_geom_map's inverse";
  return "";
}

static int check(const char* blob, const std::vector<mpcr_model_t>& mv) {
  const mpcr_model_t& m = mv[0];
  std::vector<DevModel> d, d2;
  std::string err;
  if (!compile(m, d, err)) return fail(blob, "refused: " + err);
  Rows r;
  if (!rows_of(m, r)) return fail(blob, "model_geom_poses failed");
  std::string why = against_dev(m, r, d[0]);
  if (!why.empty()) return fail(blob, why);
  // each output on its own
  {
    std::vector<float> b(8 * (size_t)r.ng + 1);
    std::vector<int> id(r.ng + 1), fx(r.ng + 1);
    if (model_geom_poses(m, b.data(), nullptr, nullptr) != r.ng || model_geom_poses(m, nullptr, id.data(), nullptr) != r.ng ||
        model_geom_poses(m, nullptr, nullptr, fx.data()) != r.ng)
      return fail(blob, "count depends on the outputs asked for");
    if (memcmp(b.data(), r.block.data(), 32 * (size_t)r.ng) || memcmp(id.data(), r.id.data(), 4 * (size_t)r.ng) ||
        memcmp(fx.data(), r.fixed.data(), 4 * (size_t)r.ng))
      return fail(blob, "an output depends on the others");
  }
  int nstatic = 0, moved = -1;
  for (int i = 0; i < r.ng; i++) {
    nstatic += r.fixed[i] != 0;
    // move the last static geom that is not the world body's (a table, an obstacle), else the world's
    if (r.fixed[i] && (moved < 0 || m.geom_bodyid[r.id[i]] != 0)) moved = i;
  }
  if (moved >= 0) {
    std::vector<mpcr_model_t> cv(mv);
    mpcr_model_t& c = cv[0];
    const int g = r.id[moved];
    c.geom_pos[g][0] += 0.05; c.geom_pos[g][1] -= 0.04; c.geom_pos[g][2] += 0.02;
    const double yaw[4] = {cos(0.15), 0, 0, sin(0.15)};
    double q[4];
    step_detail::qmul(q, yaw, c.geom_quat[g]);
    memcpy(c.geom_quat[g], q, sizeof(q));
    if (!compile(c, d2, err)) return fail(blob, "moved copy refused: " + err);
    Rows r2;
    if (!rows_of(c, r2)) return fail(blob, "model_geom_poses failed on the moved copy");
    why = against_dev(c, r2, d2[0]);
    if (!why.empty()) return fail(blob, "moved copy: " + why);
    for (int i = 0; i < r.ng; i++) {
      const bool same = memcmp(&r.block[8 * (size_t)i], &r2.block[8 * (size_t)i], 32) == 0;
      if (i == moved ? same : !same)
        return fail(blob, i == moved ? "the moved geom's row did not change" : "another row changed with the moved geom");
    }
    if (r2.id != r.id || r2.fixed != r.fixed) return fail(blob, "the move changed the id map");
  }
  printf("OK %s ngeom=%d nstatic=%d\n", blob, r.ng, nstatic);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  // a geom-pose pointer alone selects the STATE kernels; without a device parameter block nothing does
  {
    static const float dummy[8] = {};
    RolloutArgs a;
    memset(&a, 0, sizeof(a));
    a.dpar = dummy;
    a.blk.st = StateArgs{nullptr, nullptr, 0, 0, 0, nullptr, nullptr, 0, 0};
    if (has_state(a)) { printf("FAIL has_state: true without any block\n"); return 1; }
    a.blk.st = StateArgs{nullptr, nullptr, 0, 0, 0, nullptr, dummy, 16, 8};
    if (!has_state(a)) { printf("FAIL has_state: false for geom_pose alone\n"); return 1; }
    const StateArgs s = a.blk.st;
    if (s.geom_pose != dummy || s.geom_stride != 16 || s.geom_step_stride != 8 || s.ctrl || s.start || s.final_state) {
      printf("FAIL StateArgs: round trip\n");
      return 1;
    }
    a.dpar = nullptr;
    if (has_state(a)) { printf("FAIL has_state: true without dpar\n"); return 1; }
  }
  if (!strcmp(argv[1], "--layout")) {
#define X(name) printf(#name " %zu %zu\n", offsetof(DevModel, name), sizeof(DevModel::name));
    FIELDS(X)
#undef X
    printf("sizeof %zu 0\n", sizeof(DevModel));
    printf("stateargs %zu 0\n", sizeof(StateArgs));
    return 0;
  }
  int bad = 0;
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
    bad |= check(argv[a], m);
  }
  return bad;
}
