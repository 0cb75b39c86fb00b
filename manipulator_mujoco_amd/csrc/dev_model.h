// dev_model.h -- the device-model compiler: from a checked model blob
// (mpcr_model_t) to the fp32 DevModel (mpcr_device.h) and the host images of
// the tables its pointers name (hull records, support start table, faces,
// cone cells).  Plain host code: it includes rollout.h for DevModel, SmemW and
// W2_LEAD_MAX (so it needs the HIP headers for their vector types) but calls
// no HIP runtime function, reads no environment variable and reports errors
// as an MPCR_E* code with the message in a caller's string.  engine.hip's
// mpcr_engine_create uploads what it builds; tests/test_dev_model.py runs it
// on the CPU under the address / undefined-behaviour sanitizers.
#pragma once
#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mpcr.h"
#include "model_frames.h"
#include "rollout.h"

namespace mpcr {

// what mpcr_engine_create reads of the environment and the process for the
// compiler, at engine creation
struct DevOptions {
  int newton_reuse = 1;             // MPCR_NEWTON_REUSE (0: the kernel's first Newton iteration recomputes)
  int narrow_eager = 0;             // MPCR_NARROW_EAGER (1: contact geometry on every lane, not only the emitting ones)
  int lane_work = 1;                // MPCR_LANE_WORK (0: the single-arm step's former one-lane / repeated work)
  int m_slab = 0;                   // MPCR_M_SLAB (tests: the HBM-slab path on a model that fits)
  int w2_lead_max = W2_LEAD_MAX;    // MPCR_W2_LEAD_MAX
  uint64_t start_scramble = 0;      // mpcr_set_hull_start_scramble's seed (0: the extreme vertices)
};

// host images of the tables DevModel's pointers name (empty: the model has none)
struct DevTables {
  std::vector<float4> hull_vert, hull_adjv, hull_head, hull_lut;
  std::vector<int2> hull_info;
  std::vector<float4> face_plane;
  std::vector<int2> face_vinfo, vert_finfo, cone_cell;
  std::vector<int> cone_face;
};

inline int dev_fail(std::string& err, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
inline int dev_fail(std::string& err, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  err = buf;
  return code;
}

// ---- support start table (model v9: built here from hull_vert, not packed) ----
// Per hull and cube-map cell (6 faces x R x R, convex_mpr.h lut_cell order) the
// vertex extreme along the cell centre, in fp64.  The cells of a hull run in
// scan order, each climbing the hull graph (strict ascent) from the previous
// cell's vertex -- neighbouring cells mostly share one, so a cell costs a
// round or two -- and then taking the lowest index among the exactly tied
// maxima reachable along tied edges.  Any vertex of the hull would do as a
// start: the kernel's tie walk makes its supports start-independent
// (tests/test_gpu_parity.py), so R is a speed choice, and the extreme vertex
// keeps the climbs short and lets the engine mark cells exact.
inline uint64_t mix64(uint64_t x) {  // splitmix64 finaliser
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

template <class F>
void for_each_hull_parallel(const std::vector<int>& hulls, F&& f) {
  const int nt = (int)std::min<size_t>(hulls.size(), std::max(1u, std::min(16u, std::thread::hardware_concurrency())));
  if (nt <= 1) {
    for (int g : hulls) f(g);
    return;
  }
  std::atomic<int> next{0};
  std::vector<std::thread> pool;
  for (int t = 0; t < nt; t++)
    pool.emplace_back([&] {
      for (int i; (i = next.fetch_add(1)) < (int)hulls.size();) f(hulls[i]);
    });
  for (auto& t : pool) t.join();
}

// geom_adr[ngeom]: each geom's first cell (-1: no hull); returns the cell
// count.  cells (nullable): the global vertex of every cell; scramble != 0
// names a hashed vertex of the hull instead (the start-independence tests).
inline int64_t hull_start_table(const mpcr_model_t& m, int R, uint64_t scramble, int32_t* geom_adr,
                                int32_t* cells) {
  const int64_t nc = 6LL * R * R;
  int64_t n = 0;
  std::vector<int> hulls;
  std::vector<int64_t> first(m.ngeom, -1);
  for (int g = 0; g < m.ngeom; g++)
    if (m.geom_hulladr[g] >= 0 && m.geom_hullnum[g] > 0) {
      first[g] = n;
      n += nc;
      hulls.push_back(g);
    }
  if (geom_adr)
    for (int g = 0; g < m.ngeom; g++) geom_adr[g] = (int32_t)first[g];
  if (!cells) return n;
  std::vector<double> cen(R);
  for (int i = 0; i < R; i++) cen[i] = -1.0 + (2.0 * i + 1.0) / R;
  for_each_hull_parallel(hulls, [&](int g) {
    const int a = m.geom_hulladr[g], na = m.geom_hullnum[g];
    int32_t* out = cells + first[g];
    if (scramble) {
      for (int64_t c = 0; c < nc; c++) out[c] = a + (int)(mix64(scramble ^ ((uint64_t)g << 40) ^ (uint64_t)c) % na);
      return;
    }
    std::vector<int> tied;
    int v = a;
    for (int64_t c = 0; c < nc; c++) {
      const int f = (int)(c / ((int64_t)R * R)), iu = (int)((c / R) % R), iv = (int)(c % R), ax = f / 2;
      double d[3];
      d[ax] = (f & 1) ? -1.0 : 1.0;
      d[(ax + 1) % 3] = cen[iu];
      d[(ax + 2) % 3] = cen[iv];
      auto val = [&](int u) { return m.hull_vert[u][0] * d[0] + m.hull_vert[u][1] * d[1] + m.hull_vert[u][2] * d[2]; };
      double best = val(v);
      for (;;) {
        int nb = v;
        for (int k = m.hull_adjadr[v]; k < m.hull_adjadr[v] + m.hull_adjnum[v]; k++) {
          const int u = m.hull_adj[k];
          const double du = val(u);
          if (du > best) { best = du; nb = u; }
        }
        if (nb == v) break;
        v = nb;
      }
      tied.assign(1, v);
      int lo = v;
      for (size_t i = 0; i < tied.size() && tied.size() < 256; i++)
        for (int k = m.hull_adjadr[tied[i]]; k < m.hull_adjadr[tied[i]] + m.hull_adjnum[tied[i]]; k++) {
          const int u = m.hull_adj[k];
          if (val(u) == best && std::find(tied.begin(), tied.end(), u) == tied.end()) {
            tied.push_back(u);
            lo = std::min(lo, u);
          }
        }
      out[c] = lo;
    }
  });
  return n;
}

// exact[c] = 1 when cell c's start vertex is the support of every direction
// in the cell: the kernel's climb from it would end where it starts (no
// neighbour beats it, and no hint vertex beats the start), so the kernel skips
// the hint load and the climb -- bitwise the same support point, one
// dependent load instead of two or more.  A cube-map cell is the convex cone
// of its 4 corner rays and the directions a hull vertex is extreme for are a
// convex cone, bounded by its neighbours: the start vertex beats each
// neighbour by more than the margin along each corner ray (fp32 coordinates,
// as the kernel reads them), so along every direction of the cell.  The
// margin, max(1e-6 m, 32 FLT_EPSILON max|x|), scales with the hull's extent:
// the kernel's fp32 projections err by a few ulp of the largest coordinate
// (~1e-8 m on the gripper's cm-sized hulls, whose margin stays 1e-6 m;
// tests/test_hull_lut.py checks sampled directions on metre-sized hulls).
inline void hull_exact_cells(const mpcr_model_t& m, int R, const int32_t* geom_adr, const int32_t* cells,
                             uint8_t* exact) {
  constexpr double kExactGap = 1e-6;
  std::vector<int> hulls;
  for (int g = 0; g < m.ngeom; g++)
    if (geom_adr[g] >= 0) hulls.push_back(g);
  auto xf = [&](int v, int k) { return (double)(float)m.hull_vert[v][k]; };
  for_each_hull_parallel(hulls, [&](int g) {
    double gap_min = kExactGap;
    for (int v = m.geom_hulladr[g]; v < m.geom_hulladr[g] + m.geom_hullnum[g]; v++)
      gap_min = std::max(gap_min, 32.0 * FLT_EPSILON * std::sqrt(xf(v, 0) * xf(v, 0) + xf(v, 1) * xf(v, 1) + xf(v, 2) * xf(v, 2)));
    for (int64_t c = 0, nc = 6LL * R * R; c < nc; c++) {
      const int v = cells[geom_adr[g] + c];
      const int f = (int)(c / ((int64_t)R * R)), iu = (int)((c / R) % R), iv = (int)(c % R), ax = f / 2;
      bool ok = true;
      for (int du = 0; du < 2 && ok; du++)
        for (int dv = 0; dv < 2 && ok; dv++) {
          double d[3];
          d[ax] = (f & 1) ? -1.0 : 1.0;
          d[(ax + 1) % 3] = -1.0 + 2.0 * (iu + du) / R;
          d[(ax + 2) % 3] = -1.0 + 2.0 * (iv + dv) / R;
          const double dn = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
          for (int k = m.hull_adjadr[v]; k < m.hull_adjadr[v] + m.hull_adjnum[v] && ok; k++) {
            const int u = m.hull_adj[k];
            const double gap = (xf(v, 0) - xf(u, 0)) * d[0] + (xf(v, 1) - xf(u, 1)) * d[1] + (xf(v, 2) - xf(u, 2)) * d[2];
            ok = gap > gap_min * dn;
          }
        }
      exact[geom_adr[g] + c] = ok;
    }
  });
}

// The narrow variant (16-wide solves, 16 bodies, 24 collision geoms, Euler,
// joint equalities only) covers the single-arm scenes; anything else runs the
// wide one (dual-arm class).
inline bool needs_wide(const mpcr_model_t& m, const DevModel& d) {
  if (m.nv > 16 || d.nbody > 16 || d.ngeom > 24 || m.nq > MPCR_N_NQ || m.nu > 0 || d.has_spring ||
      m.integrator != MPCR_INT_EULER || m.cone != MPCR_CONE_PYRAMIDAL || m.nten > 0 || m.viscosity != 0)
    return true;
  for (int e = 0; e < m.neq; e++)
    if (m.eq_type[e] != MPCR_EQ_JOINT) return true;
  for (int p = 0; p < m.npair; p++)
    if (m.pair_func[p] == MPCR_COL_CONVEX || m.pair_func[p] == MPCR_COL_PLANE_CONVEX) return true;
  return false;
}

// An actuator's control as the kernel multiplies it into the gain: clamped to
// the model's range where it limits the control, rounded to fp32 (the kernel
// clamps a call's control block to DevModel::act_ctrlrange the same way).
inline float clamped_ctrl(const mpcr_model_t& m, int a, double ctrl) {
  if (m.act_ctrllimited[a]) ctrl = std::fmin(std::fmax(ctrl, m.act_ctrlrange[a][0]), m.act_ctrlrange[a][1]);
  return (float)ctrl;
}

// d force / d vel of actuator a through its gain, per unit of control: what
// of implicitfast's D depends on the control.
inline double act_gain_dvel(const mpcr_model_t& m, int a) {
  return m.act_gaintype[a] == MPCR_GAIN_AFFINE ? m.act_gainprm[a][2] : 0.0;
}

// implicitfast: D = -qDeriv = damping + sum_a (-dforce/dvel) m m^T, nv x nv
// row-major in fp64 (the device model rounds it), at the clamped controls
// ctrl[nu].  Built once per engine on the host.
inline void implicit_D(const mpcr_model_t& m, const float* ctrl, std::vector<double>& D) {
  const bool no_passive = m.disableflags & MPCR_DSBL_PASSIVE;
  D.assign((size_t)m.nv * m.nv, 0.0);
  for (int i = 0; i < m.nv; i++) D[(size_t)i * m.nv + i] = no_passive ? 0.0 : m.dof_damping[i];
  for (int a = 0; a < m.nu; a++) {
    double dv = 0;
    if (m.act_biastype[a] == MPCR_BIAS_AFFINE) dv += m.act_biasprm[a][2];
    if (m.act_gaintype[a] == MPCR_GAIN_AFFINE) dv += act_gain_dvel(m, a) * (double)ctrl[a];
    for (int k = 0; k < m.act_ntrn[a]; k++)
      for (int l = 0; l < m.act_ntrn[a]; l++)
        D[(size_t)m.act_dof[a][k] * m.nv + m.act_dof[a][l]] -= dv * m.act_moment[a][k] * m.act_moment[a][l];
  }
}

// Whether the engine's D (above) would change with the controls: an
// implicitfast model with a velocity-dependent gain.  Such a model cannot take
// its controls as a call input or have them replaced in a plant, because D is
// not rebuilt (no bundled model is one).
inline bool implicit_D_reads_ctrl(const mpcr_model_t& m) {
  if (m.integrator != MPCR_INT_IMPLICITFAST) return false;
  for (int a = 0; a < m.nu; a++)
    if (act_gain_dvel(m, a) != 0.0) return true;
  return false;
}

// World pose of static geom g (its body is welded to the world: f.dmap < 0)
// as the kernel reads it: the body's constant world frame composed with the
// geom's local pose in fp64, rounded once.  pos[0..2], quat[0..3].  The device
// model's geom_pos / geom_quat rows and a call's geom-pose block
// (model_geom_poses) both come from here.
inline void static_geom_pose(const mpcr_model_t& m, const ModelFrames& f, int g, float* pos, float* quat) {
  const int b = m.geom_bodyid[g];
  double r[3], q[4];
  step_detail::rot(r, f.wquat[b], m.geom_pos[g]);
  step_detail::qmul(q, f.wquat[b], m.geom_quat[g]);
  for (int k = 0; k < 3; k++) pos[k] = (float)(f.wpos[b][k] + r[k]);
  for (int k = 0; k < 4; k++) quat[k] = (float)q[k];
}

// The model's own geom-pose block (rollout.h StateArgs::geom_pose): per
// collision geom, in the device model's order (pair_geom_map), x y z 0 | qw qx
// qy qz for a static geom and zeros | 1 0 0 0 for a moving one (never read).
// block[ng][8], model_geom_id[ng], is_static[ng], each nullable; returns ng,
// or -1 when the model exceeds the blob's capacities.
inline int model_geom_poses(const mpcr_model_t& m, float* block, int* model_geom_id, int* is_static) {
  ModelFrames f;
  if (model_frames(m, f) != 0) return -1;
  int gmap[MPCR_MAX_GEOM];
  const int ng = pair_geom_map(m, gmap);
  for (int g = 0; g < m.ngeom; g++) {
    const int i = gmap[g];
    if (i < 0) continue;
    const bool fixed = f.dmap[m.geom_bodyid[g]] < 0;
    if (model_geom_id) model_geom_id[i] = g;
    if (is_static) is_static[i] = fixed;
    if (!block) continue;
    float* row = block + 8 * (size_t)i;
    for (int k = 0; k < 8; k++) row[k] = 0.f;
    row[4] = 1.f;
    if (fixed) static_geom_pose(m, f, g, row, row + 4);
  }
  return ng;
}

// The robot-masked contact slots (cost_c's, a call's slot-weight block): slot
// pair_slotadr[p] + c, c < pair_ncon[p], belongs to pair p; its two geoms in
// the device model's geom order (model_geom_poses' rows).  geom1[nslot],
// geom2[nslot], pair[nslot], each nullable; returns nslot, or -1 when a masked
// pair's slots fall outside it.  Host only.
inline int model_slots(const mpcr_model_t& m, int* geom1, int* geom2, int* pair) {
  int gmap[MPCR_MAX_GEOM];
  pair_geom_map(m, gmap);
  for (int p = 0; p < m.npair; p++) {
    const int sa = m.pair_slotadr[p];
    if (sa < 0) continue;
    if (sa + m.pair_ncon[p] > m.nslot) return -1;
    for (int c = 0; c < m.pair_ncon[p]; c++) {
      if (geom1) geom1[sa + c] = gmap[m.pair_geom1[p]];
      if (geom2) geom2[sa + c] = gmap[m.pair_geom2[p]];
      if (pair) pair[sa + c] = p;
    }
  }
  return m.nslot;
}

// Fills d (its table pointers stay null: mpcr_engine_create sets them to the
// uploaded DevTables) or returns the refusal's code with its message in err.
// lutadr[ngeom]: hull_start_table's geom_adr.
inline int build_dev_model(const mpcr_model_t& m, const int32_t* lutadr, const DevOptions& opt, DevModel& d,
                           std::string& err) {
  std::memset(&d, 0, sizeof(d));
  // moving bodies, static poses, folded frames, trees, dof kinds (model_frames.h)
  ModelFrames f;
  if (model_frames(m, f) != 0) return dev_fail(err, MPCR_EMODEL, "model exceeds blob capacity");
  const int* dmap = f.dmap;
  const int nb = f.nbody;
  if (nb > DX_NB) return dev_fail(err, MPCR_EMODEL, "%d moving bodies > %d", nb, DX_NB);
  if (m.nv > DX_NV) return dev_fail(err, MPCR_EMODEL, "nv=%d > %d (kernel solve width)", m.nv, DX_NV);
  if (m.nq > DX_NQ || m.njnt > DX_NJ || m.neq > DX_NEQ || m.nctrl > DX_NCTRL)
    return dev_fail(err, MPCR_EMODEL, "model sizes exceed device capacity");
  const bool no_passive = m.disableflags & MPCR_DSBL_PASSIVE;
  d.nbody = nb;
  d.njnt = m.njnt;
  d.nq = m.nq;
  d.nv = m.nv;
  d.neq = m.neq;
  d.nslot = m.nslot;
  d.nctrl = m.nctrl;
  d.iterations = m.iterations;
  d.ls_iterations = m.ls_iterations;
  d.disableflags = m.disableflags | (opt.newton_reuse ? 0 : DEV_NO_NEWTON_REUSE) |
                   (opt.narrow_eager ? DEV_NARROW_EAGER : 0) | (opt.lane_work ? 0 : DEV_NO_LANE_WORK);
  d.timestep = (float)m.timestep;
  d.tolerance = (float)m.tolerance;
  d.ls_tolerance = (float)m.ls_tolerance;
  d.meaninertia = (float)m.meaninertia;
  const bool no_grav = m.disableflags & MPCR_DSBL_GRAVITY;
  for (int k = 0; k < 3; k++) d.gravity[k] = no_grav ? 0.f : (float)m.gravity[k];
  for (int i = 0; i < nb; i++) {
    const int b = f.id[i], njnt = m.body_jntnum[b], j = f.jnt[i];
    if (njnt > 1) return dev_fail(err, MPCR_EMODEL, "body %d has %d joints (1 supported)", b, njnt);
    if (j >= 0 && m.jnt_type[j] == MPCR_JNT_BALL) return dev_fail(err, MPCR_EMODEL, "ball joints not supported");
    d.body_jnt[i] = j;
    d.body_kind[i] = f.kind[i];
    d.body_anc[i] = f.anc[i];
    for (int k = 0; k < 3; k++) d.body_bpos[i][k] = (float)f.bpos[i][k];
    for (int k = 0; k < 4; k++) d.body_bquat[i][k] = (float)f.bquat[i][k];
    for (int k = 0; k < 3; k++) d.body_ipos[i][k] = (float)m.body_ipos[b][k];
    double R[9];
    step_detail::q2m(R, m.body_iquat[b]);
    double I[9];
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++)
        I[3 * r + c] = R[3 * r] * m.body_inertia[b][0] * R[3 * c] + R[3 * r + 1] * m.body_inertia[b][1] * R[3 * c + 1] +
                       R[3 * r + 2] * m.body_inertia[b][2] * R[3 * c + 2];
    d.body_Iloc[i][0] = (float)I[0]; d.body_Iloc[i][1] = (float)I[4]; d.body_Iloc[i][2] = (float)I[8];
    d.body_Iloc[i][3] = (float)I[1]; d.body_Iloc[i][4] = (float)I[2]; d.body_Iloc[i][5] = (float)I[5];
    d.body_mass[i] = (float)m.body_mass[b];
    d.body_gravcomp[i] = no_passive ? 0.f : (float)m.body_gravcomp[b];
    d.body_invw[i] = (float)m.body_invweight0[b][0];
    d.body_dofmask[i] = m.body_dofmask[b];
    const int t = f.tree[i];
    if (t >= DX_NTREE) return dev_fail(err, MPCR_EMODEL, "too many kinematic trees");
    d.body_tree[i] = t;
    d.tree_mass[t] += (float)m.body_mass[b];
  }
  d.ntree = f.ntree;
  // inertia-box viscosity (mj_inertiaBoxFluidModel, density 0): the body's
  // equivalent box gives the diameter d = mean side
  if (m.viscosity > 0 && !no_passive)
    for (int b = 1; b < m.nbody; b++) {
      const int i = dmap[b];
      const double mass = m.body_mass[b];
      if (i < 0 || mass < 1e-15) continue;
      double diam = 0;
      for (int k = 0; k < 3; k++) {
        double x = m.body_inertia[b][(k + 1) % 3] + m.body_inertia[b][(k + 2) % 3] - m.body_inertia[b][k];
        diam += std::sqrt((x > 1e-15 ? x : 1e-15) / mass * 6) / 3;
      }
      d.body_visc[i][0] = (float)(-3 * M_PI * diam * m.viscosity);
      d.body_visc[i][1] = (float)(-M_PI * diam * diam * diam * m.viscosity);
    }
  // spatial tendons: site bodies and positions
  if (m.nten > DX_NTEN) return dev_fail(err, MPCR_EMODEL, "%d spatial tendons > %d", m.nten, DX_NTEN);
  d.nten = m.nten;
  for (int t = 0; t < m.nten; t++) {
    for (int k = 0; k < 2; k++) {
      const int st = m.ten_site[t][k], b = m.site_bodyid[st];
      if (dmap[b] >= 0) {
        d.ten_body[t][k] = dmap[b];
        for (int c = 0; c < 3; c++) d.ten_pos[t][k][c] = (float)m.site_pos[st][c];
      } else {
        double r[3];
        step_detail::rot(r, f.wquat[b], m.site_pos[st]);
        d.ten_body[t][k] = -1;
        for (int c = 0; c < 3; c++) d.ten_pos[t][k][c] = (float)(f.wpos[b][c] + r[c]);
      }
    }
    d.ten_limited[t] = m.ten_limited[t];
    for (int k = 0; k < 2; k++) { d.ten_range[t][k] = (float)m.ten_range[t][k]; d.ten_solref[t][k] = (float)m.ten_solref[t][k]; }
    for (int k = 0; k < 5; k++) d.ten_solimp[t][k] = (float)m.ten_solimp[t][k];
    d.ten_margin[t] = (float)m.ten_margin[t];
    d.ten_invw[t] = (float)m.ten_invweight0[t];
  }
  d.cone = m.cone;
  d.impratio = (float)m.impratio;
  for (int t = 0; t < d.ntree; t++)
    if (d.tree_mass[t] <= 0) d.tree_mass[t] = 1.f;
  int rounds = 0;
  while ((1 << rounds) < f.maxdepth) rounds++;
  d.jump_rounds = rounds;
  // subtree masks (device body indices)
  for (int b = 1; b < m.nbody; b++) {
    if (dmap[b] < 0) continue;
    for (int a = b; a > 0; a = m.body_parentid[a])
      if (dmap[a] >= 0) d.body_submask[dmap[a]] |= 1u << dmap[b];
  }
  // joints
  for (int j = 0; j < m.njnt; j++) {
    d.jnt_type[j] = m.jnt_type[j];
    d.jnt_qposadr[j] = m.jnt_qposadr[j];
    d.jnt_dofadr[j] = m.jnt_dofadr[j];
    d.jnt_body[j] = dmap[m.jnt_bodyid[j]];
    d.jnt_limited[j] = m.jnt_limited[j];
    for (int k = 0; k < 3; k++) { d.jnt_pos[j][k] = (float)m.jnt_pos[j][k]; d.jnt_axis[j][k] = (float)m.jnt_axis[j][k]; }
    for (int k = 0; k < 2; k++) { d.jnt_range[j][k] = jnt_range_f(m, j, k); d.jnt_solref[j][k] = (float)m.jnt_solref[j][k]; }
    for (int k = 0; k < 5; k++) d.jnt_solimp[j][k] = (float)m.jnt_solimp[j][k];
    d.jnt_margin[j] = jnt_margin_f(m, j);
    d.jnt_qpos0[j] = (float)m.qpos0[m.jnt_qposadr[j]];
  }
  // dofs
  for (int i = 0; i < m.nv; i++) {
    int j = m.dof_jntid[i];
    int b = m.dof_bodyid[i];
    d.dof_body[i] = dmap[b];
    d.dof_jnt[i] = j;
    int sub = i - m.jnt_dofadr[j];
    d.dof_kind[i] = f.dof_kind[i];
    d.dof_sub[i] = f.dof_sub[i];
    uint32_t cm = 0;
    for (int a = i; a >= 0; a = m.dof_parentid[a]) cm |= 1u << a;
    d.dof_chainmask[i] = cm;
    int p = m.body_parentid[b];
    uint32_t pm = p > 0 ? m.body_dofmask[p] : 0u;
    if (m.jnt_type[j] == MPCR_JNT_FREE) {
      int d0 = m.jnt_dofadr[j];
      d.dof_velmask[i] = sub < 3 ? 0u : (pm | (7u << d0));
    } else {
      d.dof_velmask[i] = m.body_dofmask[b] & ~(1u << i);
    }
    d.dof_armature[i] = (float)m.dof_armature[i];
    d.dof_damping[i] = no_passive ? 0.f : (float)m.dof_damping[i];
    d.dof_invweight0[i] = dof_invweight_f(m, i);
  }
  for (int i = 0; i < m.nv; i++) d.dof_submask[i] = d.dof_body[i] >= 0 ? d.body_submask[d.dof_body[i]] : 0u;
  {  // blocked Cholesky layout: tree t's k-th dof (ascending) at lane 16 t + k
    int cnt[DX_NTREE] = {0}, mx = 0;
    bool ok = true;
    for (int l = 0; l < 64; l++) d.blane_dof[l] = -1;
    for (int i = 0; i < m.nv && ok; i++) {
      const int b = d.dof_body[i], t = b >= 0 ? d.body_tree[b] : -1;
      if (t < 0 || t >= DX_NTREE || cnt[t] >= 16) { ok = false; break; }
      d.blane_dof[16 * t + cnt[t]++] = i;
      mx = std::max(mx, cnt[t]);
    }
    d.blk_n = !ok ? 0 : (mx <= 8 ? 8 : 16);
    // rows spanning two trees keep Newton's H dense: equalities (joint: the
    // two joints' trees; connect: the two bodies', static = none) and tendons
    auto tree_of_body = [&](int b) { return b > 0 && dmap[b] >= 0 ? d.body_tree[dmap[b]] : -1; };
    auto cross = [](int t1, int t2) { return t1 >= 0 && t2 >= 0 && t1 != t2; };
    d.eq_cross = 0;
    for (int e = 0; e < m.neq; e++) {
      if (m.eq_type[e] == MPCR_EQ_JOINT) {
        const int j1 = m.eq_obj1[e], j2 = m.eq_obj2[e];
        if (j2 >= 0 && cross(tree_of_body(m.jnt_bodyid[j1]), tree_of_body(m.jnt_bodyid[j2]))) d.eq_cross = 1;
      } else if (m.eq_type[e] == MPCR_EQ_CONNECT) {
        if (cross(tree_of_body(m.eq_obj1[e]), tree_of_body(m.eq_obj2[e]))) d.eq_cross = 1;
      } else {
        d.eq_cross = 1;
      }
    }
    for (int t = 0; t < m.nten; t++)
      if (cross(tree_of_body(m.site_bodyid[m.ten_site[t][0]]), tree_of_body(m.site_bodyid[m.ten_site[t][1]])))
        d.eq_cross = 1;
  }
  {  // compact mass matrix (dual-arm image, SmemT::Mc): each tree's dofs contiguous
    int ts[DX_NTREE], te[DX_NTREE];
    bool ok = true;
    for (int t = 0; t < DX_NTREE; t++) ts[t] = te[t] = -1;
    for (int i = 0; i < m.nv && ok; i++) {
      const int b = d.dof_body[i], t = b >= 0 ? d.body_tree[b] : -1;
      if (t < 0 || t >= DX_NTREE) { ok = false; break; }
      if (ts[t] < 0) ts[t] = i;
      else if (te[t] != i) ok = false;  // a tree's dofs interleaved with another's
      te[t] = i + 1;
    }
    for (int i = 0; i < m.nv && ok; i++) {
      const int t = d.body_tree[d.dof_body[i]];
      d.mc_c0[i] = std::min(ts[t] & ~3, SmemW::NVW - SmemW::MCW);  // the window stays inside the NVW columns
      if (te[t] - d.mc_c0[i] > SmemW::MCW) ok = false;
    }
    d.mc_n = ok && m.nv * SmemW::MCW <= SmemW::MC ? m.nv : 0;
    if (opt.m_slab) d.mc_n = 0;  // tests: the HBM-slab path on a model that fits
    // the two-wave lead flush's pair limit; a lower one (tests) sends more steps to the dealt flush
    d.w2_lead_max = std::max(-1, std::min(W2_LEAD_MAX, opt.w2_lead_max));
  }
  for (int i = 0; i < m.nq; i++) d.qpos_init[i] = (float)m.qpos_init[i];
  for (int i = 0; i < m.nv; i++) d.qvel_init[i] = (float)m.qvel_init[i];
  // collision geoms referenced by pairs
  int gmap[MPCR_MAX_GEOM];
  const int ng = pair_geom_map(m, gmap);
  if (ng > DX_NG || ng > WAVE) return dev_fail(err, MPCR_EMODEL, "%d collision geoms > %d", ng, DX_NG < WAVE ? DX_NG : WAVE);
  d.ngeom = ng;
  for (int g = 0; g < m.ngeom; g++) {
    int i = gmap[g];
    if (i < 0) continue;
    int b = m.geom_bodyid[g];
    d.geom_type[i] = m.geom_type[g];
    d.geom_rbound[i] = (float)m.geom_rbound[g];
    d.geom_hulladr[i] = m.geom_hulladr[g];
    d.geom_hullnum[i] = m.geom_hullnum[g];
    d.geom_lutadr[i] = lutadr[g];
    d.geom_faceadr[i] = m.geom_faceadr[g];
    d.geom_facenum[i] = m.geom_faceadr[g] >= 0 ? m.geom_facenum[g] : 0;
    d.geom_cornadr[i] = m.geom_cornadr[g];
    for (int k = 0; k < 3; k++) d.geom_size[i][k] = (float)m.geom_size[g][k];
    if (dmap[b] >= 0) {
      d.geom_body[i] = dmap[b];
      for (int k = 0; k < 3; k++) d.geom_pos[i][k] = (float)m.geom_pos[g][k];
      for (int k = 0; k < 4; k++) d.geom_quat[i][k] = (float)m.geom_quat[g][k];
    } else {  // static geom: store its world pose
      d.geom_body[i] = -1;
      static_geom_pose(m, f, g, d.geom_pos[i], d.geom_quat[i]);
    }
  }
  // pairs
  if (m.npair > DX_NP) return dev_fail(err, MPCR_EMODEL, "too many pairs");
  if (m.nslot > DX_NSLOT) return dev_fail(err, MPCR_EMODEL, "%d masked slots > %d", m.nslot, DX_NSLOT);
  d.npair = m.npair;
  d.cvx_base = m.npair;
  for (int p = m.npair - 1; p >= 0; p--)
    if (m.pair_func[p] >= MPCR_COL_CONVEX) d.cvx_base = p;
  for (int p = d.cvx_base; p < m.npair; p++)
    if (m.pair_func[p] < MPCR_COL_CONVEX) return dev_fail(err, MPCR_EMODEL, "convex pairs must be sorted last");
  if (m.npair - d.cvx_base > 512) return dev_fail(err, MPCR_EMODEL, "%d general-convex pairs > 512", m.npair - d.cvx_base);
  d.coll_rows = m.npair <= WAVE;  // DevModel::coll_rows: a light collision phase
  for (int p = 0; p < m.npair; p++)
    if (m.pair_func[p] == MPCR_COL_BOX_BOX) d.coll_rows = 0;
  d.cvx_joint = 1;  // DevModel::cvx_joint: no convex pair carries a cost slot
  for (int p = d.cvx_base; p < m.npair; p++)
    if (m.pair_slotadr[p] >= 0) d.cvx_joint = 0;
  if (m.nhullv > 32767) return dev_fail(err, MPCR_EMODEL, "hull vertex table exceeds 16-bit hints");
  for (int p = 0; p < m.npair; p++) {
    int g1 = m.pair_geom1[p], g2 = m.pair_geom2[p];
    d.pair_g1[p] = gmap[g1];
    d.pair_g2[p] = gmap[g2];
    d.pair_func[p] = m.pair_func[p];
    if (m.pair_func[p] == MPCR_COL_BOX_BOX && m.pair_slotadr[p] >= 0)
      return dev_fail(err, MPCR_EMODEL, "robot-masked box-box pairs are not supported by the kernel");
    d.pair_ncon[p] = m.pair_ncon[p];
    d.pair_slotadr[p] = m.pair_slotadr[p];
    d.pair_condim[p] = m.pair_condim[p];
    d.pair_friction[p] = (float)m.pair_friction[p];
    d.pair_cmu[p] = (float)(m.pair_friction[p] / std::sqrt(m.impratio > 0 ? m.impratio : 1.0));
    if (m.pair_condim[p] != 1 && m.pair_condim[p] != 3) return dev_fail(err, MPCR_EMODEL, "condim %d not supported", m.pair_condim[p]);
    d.pair_margin[p] = pair_margin_f(m, p);
    for (int k = 0; k < 2; k++) d.pair_solref[p][k] = (float)m.pair_solref[p][k];
    for (int k = 0; k < 5; k++) d.pair_solimp[p][k] = (float)m.pair_solimp[p][k];
    d.pair_diag[p] = (float)(m.body_invweight0[m.geom_bodyid[g1]][0] + m.body_invweight0[m.geom_bodyid[g2]][0]);
    const int b1 = d.geom_body[d.pair_g1[p]], b2 = d.geom_body[d.pair_g2[p]];
    d.pair_jinfo[p] = make_int4(b1 >= 0 ? (int)d.body_dofmask[b1] : 0, b2 >= 0 ? (int)d.body_dofmask[b2] : 0,
                                b1 >= 0 ? d.body_tree[b1] : 0, b2 >= 0 ? d.body_tree[b2] : 0);
  }
  // equalities: joint (1 row) and connect (3 rows), rows in model order
  int nrow = 0;
  for (int e = 0; e < m.neq; e++) {
    d.eq_type[e] = m.eq_type[e];
    for (int k = 0; k < 5; k++) d.eq_solimp[e][k] = (float)m.eq_solimp[e][k];
    for (int k = 0; k < 2; k++) d.eq_solref[e][k] = (float)m.eq_solref[e][k];
    if (m.eq_type[e] == MPCR_EQ_JOINT) {
      d.eq_j1[e] = m.eq_obj1[e];
      d.eq_j2[e] = m.eq_obj2[e];
      for (int k = 0; k < 5; k++) d.eq_data[e][k] = (float)m.eq_data[e][k];
      d.eq_diag[e] = eq_diag_f(m, e);
      if (nrow + 1 > DX_NEQROW) return dev_fail(err, MPCR_EMODEL, "too many equality rows");
      d.eqrow_eq[nrow] = e; d.eqrow_k[nrow] = 0; nrow++;
    } else if (m.eq_type[e] == MPCR_EQ_CONNECT) {
      for (int side = 0; side < 2; side++) {
        int b = side ? m.eq_obj2[e] : m.eq_obj1[e];
        const double* a = m.eq_data[e] + 3 * side;
        int db = b > 0 ? dmap[b] : -1;
        (side ? d.eq_b2 : d.eq_b1)[e] = db;
        double pw[3] = {a[0], a[1], a[2]};
        if (db < 0) {  // static body: anchor in world once
          double r[3];
          step_detail::rot(r, f.wquat[b], a);
          for (int k = 0; k < 3; k++) pw[k] = f.wpos[b][k] + r[k];
        }
        for (int k = 0; k < 3; k++) d.eq_data[e][4 * side + k] = (float)pw[k];
      }
      d.eq_diag[e] = eq_diag_f(m, e);
      if (nrow + 3 > DX_NEQROW) return dev_fail(err, MPCR_EMODEL, "too many equality rows");
      for (int k = 0; k < 3; k++) { d.eqrow_eq[nrow] = e; d.eqrow_k[nrow] = k + 1; nrow++; }
    } else {
      return dev_fail(err, MPCR_EMODEL, "equality type %d not supported (joint, connect)", m.eq_type[e]);
    }
  }
  d.neqrow = nrow;
  // springs
  for (int i = 0; i < m.nv; i++) {
    int j = m.dof_jntid[i];
    d.dof_qposadr[i] = m.jnt_qposadr[j];
    if (!no_passive && (m.jnt_type[j] == MPCR_JNT_HINGE || m.jnt_type[j] == MPCR_JNT_SLIDE) &&
        m.jnt_stiffness[j] != 0) {
      d.dof_stiffness[i] = (float)m.jnt_stiffness[j];
      d.dof_springref[i] = (float)m.jnt_springref[j];
      d.has_spring = 1;
    }
    d.dof_actfrc[i][0] = -3e38f;
    d.dof_actfrc[i][1] = 3e38f;
    if (m.jnt_actfrclimited[j]) {
      d.dof_actfrc[i][0] = (float)m.jnt_actfrcrange[j][0];
      d.dof_actfrc[i][1] = (float)m.jnt_actfrcrange[j][1];
    }
  }
  // actuators (the model's own control: clamped once here)
  if (m.nu > DX_NU) return dev_fail(err, MPCR_EMODEL, "%d actuators > %d", m.nu, DX_NU);
  d.nu = m.nu;
  for (int a = 0; a < m.nu; a++) {
    d.act_ntrn[a] = m.act_ntrn[a];
    for (int k = 0; k < m.act_ntrn[a]; k++) {
      int v = m.act_dof[a][k];
      d.act_dof[a][k] = v;
      d.act_qadr[a][k] = m.act_qadr[a][k];
      d.act_moment[a][k] = (float)m.act_moment[a][k];
      if (d.dof_actn[v] >= 2) return dev_fail(err, MPCR_EMODEL, "more than 2 actuators on dof %d", v);
      d.dof_acta[v][d.dof_actn[v]] = a;
      d.dof_actm[v][d.dof_actn[v]] = (float)m.act_moment[a][k];
      d.dof_actn[v]++;
    }
    d.act_gaffine[a] = m.act_gaintype[a] == MPCR_GAIN_AFFINE;
    d.act_baffine[a] = m.act_biastype[a] == MPCR_BIAS_AFFINE;
    for (int k = 0; k < 3; k++) { d.act_gain[a][k] = (float)m.act_gainprm[a][k]; d.act_bias[a][k] = (float)m.act_biasprm[a][k]; }
    d.act_gain[a][3] = clamped_ctrl(m, a, m.act_ctrl[a]);
    d.act_ctrlrange[a][0] = m.act_ctrllimited[a] ? (float)m.act_ctrlrange[a][0] : -3e38f;
    d.act_ctrlrange[a][1] = m.act_ctrllimited[a] ? (float)m.act_ctrlrange[a][1] : 3e38f;
    d.act_frc[a][0] = m.act_forcelimited[a] ? (float)m.act_forcerange[a][0] : -3e38f;
    d.act_frc[a][1] = m.act_forcelimited[a] ? (float)m.act_forcerange[a][1] : 3e38f;
  }
  // implicitfast: D = -qDeriv = damping + sum_a (-dforce/dvel) m m^T (fp64, then rounded)
  d.integrator = m.integrator;
  if (m.integrator == MPCR_INT_IMPLICITFAST) {
    float ctrl[DX_NU];
    for (int a = 0; a < m.nu; a++) ctrl[a] = d.act_gain[a][3];
    std::vector<double> D;
    implicit_D(m, ctrl, D);
    for (int i = 0; i < m.nv; i++)
      for (int j = 0; j < m.nv; j++) d.impl_D[i][j] = (float)D[(size_t)i * m.nv + j];
    d.impl_cross = 0;  // a transmission across trees keeps the implicit solve dense
    for (int i = 0; i < m.nv; i++)
      for (int j = 0; j < m.nv; j++)
        if (D[(size_t)i * m.nv + j] != 0.0 && d.body_tree[d.dof_body[i]] != d.body_tree[d.dof_body[j]]) d.impl_cross = 1;
  } else if (m.integrator != MPCR_INT_EULER) {
    return dev_fail(err, MPCR_EMODEL, "integrator %d not supported (Euler, implicitfast)", m.integrator);
  }
  // planner ids
  d.hande_body = m.hande_body >= 0 ? dmap[m.hande_body] : -1;
  d.tcp_body = -1;
  if (m.tcp_site >= 0) {
    d.tcp_body = dmap[m.site_bodyid[m.tcp_site]];
    for (int k = 0; k < 3; k++) d.tcp_pos[k] = (float)m.site_pos[m.tcp_site][k];
  }
  for (int k = 0; k < m.nctrl; k++) { d.ctrl_qposadr[k] = m.ctrl_qposadr[k]; d.ctrl_dofadr[k] = m.ctrl_dofadr[k]; }
  return MPCR_OK;
}

// The hull records (vertices, graph, per-vertex heads) and the support start
// table of a model with hull vertices; lutadr / nlut: hull_start_table's
// geom_adr and cell count.
inline int build_hull_tables(const mpcr_model_t& h, const int32_t* lutadr, int64_t nlut, uint64_t scramble,
                             DevTables& t, std::string& err) {
  if (h.nhullv > 65535)
    return dev_fail(err, MPCR_EINVAL, "%d hull vertices: the climb records hold 16-bit vertex indices", h.nhullv);
  std::vector<float4>&hv = t.hull_vert, &ha = t.hull_adjv, &hh = t.hull_head, &hl = t.hull_lut;
  std::vector<int2>& hi = t.hull_info;
  hv.resize(h.nhullv);
  hi.resize(h.nhullv);
  ha.resize(h.nhulla);
  hh.resize((size_t)h.nhullv * 8);
  auto bitsf = [](int bits) {
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
  };
  // neighbour record: xyz | index | degree << 16 -- the chosen neighbour's
  // own adjacency is then addressed without another dependent load
  auto rec = [&](int u) {
    return make_float4((float)h.hull_vert[u][0], (float)h.hull_vert[u][1], (float)h.hull_vert[u][2],
                       bitsf(u | (h.hull_adjnum[u] << 16)));
  };
  for (int k = 0; k < h.nhulla; k++) ha[k] = rec(h.hull_adj[k]);
  const float nan = std::numeric_limits<float>::quiet_NaN();
  for (int v = 0; v < h.nhullv; v++) {
    hv[v] = make_float4((float)h.hull_vert[v][0], (float)h.hull_vert[v][1], (float)h.hull_vert[v][2],
                        bitsf(h.hull_adjnum[v]));
    hi[v] = make_int2(h.hull_adjadr[v], h.hull_adjnum[v]);
    for (int j = 0; j < 8; j++)  // NaN pads never beat the current vertex
      hh[(size_t)v * 8 + j] = j < h.hull_adjnum[v] ? rec(h.hull_adj[h.hull_adjadr[v] + j]) : make_float4(nan, nan, nan, bitsf(-1));
  }
  // the support start table, exact cells flagged in bit 15 of the record's
  // index half (vertex indices are < 32768; hull_exact_cells)
  std::vector<int32_t> cells(nlut);
  std::vector<uint8_t> exact(nlut);
  hull_start_table(h, MPCR_LUT_R, scramble, nullptr, cells.data());
  hull_exact_cells(h, MPCR_LUT_R, lutadr, cells.data(), exact.data());
  hl.resize(nlut);
  for (int64_t c = 0; c < nlut; c++) {
    const int v = cells[c];
    hl[c] = rec(v);
    if (exact[c]) hl[c].w = bitsf(v | 0x8000 | (h.hull_adjnum[v] << 16));
  }
  return MPCR_OK;
}

// Face planes, polygons and vertex incidence of a model with faces, and the
// cone-cell table; writes d.geom_coneadr.
inline void build_face_tables(const mpcr_model_t& h, DevModel& d, DevTables& t) {
  std::vector<float4>& fp = t.face_plane;
  std::vector<int2>&fv = t.face_vinfo, &vf = t.vert_finfo;
  fp.resize(h.nface);
  fv.resize(h.nface);
  vf.resize(h.nhullv);
  for (int f = 0; f < h.nface; f++) {
    fp[f] = make_float4((float)h.face_plane[f][0], (float)h.face_plane[f][1], (float)h.face_plane[f][2],
                        (float)h.face_plane[f][3]);
    fv[f] = make_int2(h.face_vadr[f], h.face_vnum[f]);
  }
  for (int v = 0; v < h.nhullv; v++) vf[v] = make_int2(h.vert_faceadr[v], h.vert_facenum[v]);
  // the polyhedron manifold's cone table: per geom with faces and per
  // cube-map cell of the local direction (CONE_R x CONE_R per cube face, the
  // kernel's cone_cell order) every face whose outward normal lies within
  // acos(CONE_COS) + the cell's angular radius + 0.01 rad of the cell centre
  // -- a superset of the faces the kernel's cone test accepts for any
  // direction in the cell (fp32 cell assignment included), ascending, so the
  // scan of a cell's list compacts the same candidates in the same order as a
  // scan of all the geom's faces
  std::vector<int2>& ccell = t.cone_cell;
  std::vector<int>& cface = t.cone_face;
  const double thr0 = std::acos(CONE_COS) + 0.01;
  for (int i = 0; i < d.ngeom; i++) {
    d.geom_coneadr[i] = -1;
    const int fa = d.geom_faceadr[i], fnum = d.geom_facenum[i];
    if (fa < 0 || fnum <= 0) continue;
    d.geom_coneadr[i] = (int)ccell.size();
    for (int c = 0; c < CONE_CELLS; c++) {
      const int fc = c / (CONE_R * CONE_R), iu = (c / CONE_R) % CONE_R, iv = c % CONE_R;
      const int ax = fc / 2;
      const double sa = (fc & 1) ? -1.0 : 1.0;
      auto dir = [&](double u, double v, double out[3]) {
        out[ax] = sa; out[(ax + 1) % 3] = u; out[(ax + 2) % 3] = v;
        const double nn = std::sqrt(out[0] * out[0] + out[1] * out[1] + out[2] * out[2]);
        for (int k = 0; k < 3; k++) out[k] /= nn;
      };
      const double u0 = -1.0 + 2.0 * iu / CONE_R, u1 = -1.0 + 2.0 * (iu + 1) / CONE_R;
      const double v0 = -1.0 + 2.0 * iv / CONE_R, v1 = -1.0 + 2.0 * (iv + 1) / CONE_R;
      double ctr[3], cr[3];
      dir(0.5 * (u0 + u1), 0.5 * (v0 + v1), ctr);
      double rad = 0.0;
      for (double u : {u0, u1})
        for (double v : {v0, v1}) {
          dir(u, v, cr);
          const double cd = ctr[0] * cr[0] + ctr[1] * cr[1] + ctr[2] * cr[2];
          rad = std::max(rad, std::acos(std::min(1.0, cd)));
        }
      const double cth = std::cos(thr0 + rad);
      const int start = (int)cface.size();
      for (int f = fa; f < fa + fnum; f++) {
        const double* fp = h.face_plane[f];
        const double fn = std::sqrt(fp[0] * fp[0] + fp[1] * fp[1] + fp[2] * fp[2]);
        if (fn > 0 && (fp[0] * ctr[0] + fp[1] * ctr[1] + fp[2] * ctr[2]) / fn >= cth) cface.push_back(f);
      }
      ccell.push_back(make_int2(start, (int)cface.size() - start));
    }
  }
  if (cface.empty()) cface.push_back(0);
  if (ccell.empty()) ccell.push_back(make_int2(0, 0));
}

// The whole compile: the device model, then the tables it points to.
inline int compile_dev_model(const mpcr_model_t& m, const DevOptions& opt, DevModel& d, DevTables& t,
                             std::string& err) {
  std::vector<int32_t> lutadr(std::max(1, m.ngeom));
  const int64_t nlut = hull_start_table(m, MPCR_LUT_R, 0, lutadr.data(), nullptr);
  if (int rc = build_dev_model(m, lutadr.data(), opt, d, err)) return rc;
  if (m.nhullv > 0)
    if (int rc = build_hull_tables(m, lutadr.data(), nlut, opt.start_scramble, t, err)) return rc;
  if (m.nface > 0) build_face_tables(m, d, t);
  return MPCR_OK;
}

}  // namespace mpcr
