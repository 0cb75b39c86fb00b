// step_table.h -- what the single-arm rollout kernels read of the model every
// step, laid out once per engine: one contiguous 16-byte-aligned record per
// lane and phase (kinematics by body, motion subspaces by dof, constraint-row
// parameters by constraint source) with the dependent indices resolved and
// the constants that depend on the model and the timestep alone already
// evaluated (in double, rounded once to fp32).
//
// Plain host C++ (no HIP): build_step_table() runs at engine creation
// (engine.hip) and in a stand-alone CPU test (tests/test_step_table.py).  The
// table is uploaded directly behind the device model (DevModel) in the same
// allocation; the narrow kernels reach it as (const StepTable*)(model + 1),
// so neither DevModel nor the launch arguments change.  (A pointer field in
// DevModel would say so in the types, but any change of sizeof(DevModel) or of
// the launch arguments changes the dual-arm unit's device code: the model
// pointer's launder scales by that size, the kernel metadata carries the
// argument size.  engine.hip's mpcr_engine_create is the one place a device
// model is allocated.)  The bodies, frames, trees and dof kinds come from
// model_frames() (model_frames.h), which the device model's builder
// (dev_model.h build_dev_model) reads too, as it does the row values both
// hold; tests/test_dev_model.py compares the two results on the CPU.
// Behind the table, in the same allocation, lie the load records
// (StepRecords, build_step_records(); tests/test_step_records.py): model
// constants gathered so that a lane reaches them in one level of loads.
//
// Device indices as in dev_model.h build_dev_model: moving bodies (not welded
// to the world) in model order, pairs / joints / equalities by their model
// index.  (The geoms have no records: a geom's rotation matrix evaluated in
// double has exact zeros where the kernel's fp32 q2m leaves 6e-8, which moves
// the ties of axis-aligned box contacts and with them the planner scene's
// parity -- DESIGN.md, "Measured and not kept".)
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "model_frames.h"

namespace mpcr {

constexpr int ST_NB = 32, ST_NV = 32, ST_NP = 768, ST_NJ = 32, ST_NEQ = 8;  // = DX_* (mpcr_device.h)
// rows of StepTable::row: pairs, then joints (limit rows), then equalities
constexpr int ST_ROW_PAIR = 0, ST_ROW_JNT = ST_NP, ST_ROW_EQ = ST_NP + ST_NJ, ST_NROW = ST_NP + ST_NJ + ST_NEQ;
// the kernel's constants (rollout.h kMinVal / kMinImp / kMaxImp)
constexpr float ST_MINVAL = 1e-15f, ST_MINIMP = 0.0001f, ST_MAXIMP = 0.9999f;

// StepTable::flags
enum { ST_ANCHOR0 = 1 };  // every hinge / slide joint sits at its body's origin (jnt_pos = 0): no anchor terms
// StepRow::flags
enum {
  ST_POW2 = 1,     // solimp power == 2 (the default): y = x^2 / mid | 1 - (1 - x)^2 / (1 - mid)
  ST_POW1 = 2,     // power == 1: y = x
  ST_LIMITED = 4,  // joint rows: a limited hinge / slide joint
  ST_CONDIM1 = 8   // pair rows: frictionless contact (one row)
};
// kinematics, by moving body (quads of 4 floats; 144 B)
struct alignas(16) StepBody {
  int32_t kind, anc, qposadr;  // ST_BK_*; first moving ancestor (-1: none); the joint's qpos address (-1: weld)
  float qpos0;                 // the joint's reference position
  float bquat[4];              // pre-joint local (or, under a static parent, world) orientation
  float bpos[3], pad0;         // and position
  float axis[3], pad1;         // hinge: joint axis in the body frame; slide: R(bquat) axis, the direction in the parent frame
  float ipos[3], pad2;         // centre of mass in the body frame
  float jpos[3], pad3;         // hinge anchor in the body frame             } read only when some joint sits
  float R[3][4];               // rows of the rotation matrix of bquat      } off its body's origin (no ST_ANCHOR0)
};
// motion subspaces, by dof (48 B)
struct alignas(16) StepDof {
  int32_t body, kind, tree, sub;  // kind: 0 hinge 1 slide 2 free translation 3 free rotation; sub: free axis 0..2
  float axis[3], pad0;            // the joint's axis and anchor in the body frame
  float jpos[3], pad1;
};
// constraint-row parameters, by constraint source (64 B)
struct alignas(16) StepRow {
  float dmin, dmax, iwidth, mid;  // clamped solimp d0 / dwidth, 1 / width
  float imid, i1mid, K, B;        // 1 / mid, 1 / (1 - mid); aref = -B vel - K imp (pos - margin)
  float margin, diag;             // pair: margin - gap, invweight sum x (1 + mu^2 unless condim 1)
  int32_t flags;
  float power;
  float range[2];                 // joint rows: limits, qpos address, dof address (dofadr: not read by the
  int32_t qposadr, dofadr;        // kernel; it fills the quad and the tests compare it with the device model's)
};

// quad 3 of a pair's StepRow (in place of range / qposadr / dofadr, which
// only joint rows have): the contact Jacobian's constants
struct alignas(16) StepPairJ {
  uint32_t mask1, mask2;  // dof masks of the two geoms' bodies (static body: 0)
  int32_t trees;          // tree of body 1 | tree of body 2 << 8 (static body: 0) | frictionless (condim 1) << 16
  float mu;               // friction
};

struct alignas(16) StepTable {
  int32_t flags, nbody, pad[2];  // nbody: for the tests, not read by the kernel
  StepBody body[ST_NB];
  StepDof dof[ST_NV];
  StepRow row[ST_NROW];
};

// The load records: model constants a lane otherwise reaches through a chain
// of dependent loads (index -> index -> value), gathered so that the lane
// fetches them in one level, the loads issued together and waited for once.
// A second struct directly behind the table in the same allocation,
// (const StepRecords*)(table + 1), with its own builder: the table's layout
// and build_step_table()'s signature stay.
// collision set-up, by pair (64 B): the cull, the narrow phase's head and
// the contact emission
struct alignas(16) StepPairSetup {
  int32_t func, slotadr, g1, g2;  // narrow-phase function, first masked slot (-1: none), collision geoms
  int32_t types;                  // geom type 1 | geom type 2 << 8 | contact slots << 16
  float rbound1, rbound2, margin; // bounding radii, margin - gap
  float size1[3], pad0;           // the geoms' sizes
  float size2[3], pad1;
};
// joint equality, by equality (48 B)
struct alignas(16) StepEq {
  int32_t qadr1, dadr1, qadr2, dadr2;  // the joints' qpos and dof addresses; no second joint: -1, -1
  float qpos0_1, qpos0_2, c0, c1;      // reference positions (no second joint: 0), polynomial coefficients
  float c2, c3, c4, pad;
};
struct alignas(16) StepRecords {
  StepPairSetup pair[ST_NP];
  StepEq eq[ST_NEQ];
};

namespace step_detail {
inline double clampd(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

// the parameters of one constraint source from its solref / solimp
inline void row_params(StepRow& r, const double solref[2], const double solimp[5], double timestep, int disableflags) {
  double dmin = clampd(solimp[0], (double)ST_MINIMP, (double)ST_MAXIMP);
  double dmax = clampd(solimp[1], (double)ST_MINIMP, (double)ST_MAXIMP);
  double width = solimp[2], mid = solimp[3];
  const double power = solimp[4];
  // a flat impedance (the kernel's early return 0.5 (dmin + dmax)): stored as
  // dmin = dmax = that value with 1 / width = 0, so the general path returns it
  const bool flat = (float)dmin == (float)dmax || (float)width <= ST_MINVAL;
  double iwidth = 1.0 / width, imid = 1.0 / mid, i1mid = 1.0 / (1.0 - mid);
  if (flat) {
    dmin = dmax = 0.5 * ((double)(float)dmin + (double)(float)dmax);
    iwidth = 0.0; mid = 0.5; imid = 2.0; i1mid = 2.0;
  }
  // the reference acceleration's stiffness and damping (d = the clamped dmax
  // of the solimp as given, also for a flat impedance)
  const double d = clampd(solimp[1], (double)ST_MINIMP, (double)ST_MAXIMP);
  double tc = solref[0];
  const double dr = solref[1];
  double K, B;
  if ((float)tc > 0.f) {
    if (!(disableflags & MPCR_DSBL_REFSAFE) && tc < 2.0 * timestep) tc = 2.0 * timestep;
    K = 1.0 / (d * d * tc * tc * dr * dr);
    B = 2.0 / (d * tc);
  } else {
    K = -tc / (d * d);
    B = -dr / d;
  }
  r.dmin = (float)dmin; r.dmax = (float)dmax; r.iwidth = (float)iwidth; r.mid = (float)mid;
  r.imid = (float)imid; r.i1mid = (float)i1mid; r.K = (float)K; r.B = (float)B;
  r.power = (float)power;
  r.flags = flat ? ST_POW1 : ((float)power == 2.f ? ST_POW2 : ((float)power == 1.f ? ST_POW1 : 0));
}
}  // namespace step_detail

// Fills t from the model.  Returns 0, or -1 when the model exceeds the
// table's capacities (the engine has then already refused it).
inline int build_step_table(const mpcr_model_t& m, StepTable& t) {
  using namespace step_detail;
  memset(&t, 0, sizeof(t));
  if (m.nbody > MPCR_MAX_BODY || m.njnt > ST_NJ || m.nv > ST_NV || m.npair > ST_NP || m.neq > ST_NEQ)
    return -1;
  ModelFrames f;
  if (model_frames(m, f) != 0 || f.nbody > ST_NB) return -1;
  t.nbody = f.nbody;
  bool anchor0 = true;
  for (int i = 0; i < f.nbody; i++) {
    StepBody& r = t.body[i];
    const int b = f.id[i], j = f.jnt[i];
    r.kind = f.kind[i];
    r.anc = f.anc[i];
    r.qposadr = j >= 0 ? m.jnt_qposadr[j] : -1;
    r.qpos0 = j >= 0 ? (float)m.qpos0[m.jnt_qposadr[j]] : 0.f;
    double R[9];
    q2m(R, f.bquat[i]);
    for (int k = 0; k < 4; k++) r.bquat[k] = (float)f.bquat[i][k];
    for (int k = 0; k < 3; k++) {
      r.bpos[k] = (float)f.bpos[i][k];
      r.ipos[k] = (float)m.body_ipos[b][k];
      for (int c = 0; c < 3; c++) r.R[k][c] = (float)R[3 * k + c];
    }
    if (r.kind == ST_BK_HINGE || r.kind == ST_BK_SLIDE) {
      for (int k = 0; k < 3; k++) {
        const double* a = m.jnt_axis[j];
        r.axis[k] = r.kind == ST_BK_HINGE ? (float)a[k] : (float)(R[3 * k] * a[0] + R[3 * k + 1] * a[1] + R[3 * k + 2] * a[2]);
        r.jpos[k] = (float)m.jnt_pos[j][k];
        if (r.jpos[k] != 0.f) anchor0 = false;
      }
    }
  }
  t.flags = anchor0 ? ST_ANCHOR0 : 0;
  // dofs
  for (int i = 0; i < m.nv; i++) {
    StepDof& r = t.dof[i];
    const int j = m.dof_jntid[i];
    r.body = f.dmap[m.dof_bodyid[i]];
    r.kind = f.dof_kind[i];
    r.tree = r.body >= 0 ? f.tree[r.body] : -1;
    r.sub = f.dof_sub[i];
    for (int k = 0; k < 3; k++) { r.axis[k] = (float)m.jnt_axis[j][k]; r.jpos[k] = (float)m.jnt_pos[j][k]; }
  }
  // constraint sources
  for (int p = 0; p < m.npair; p++) {
    StepRow& r = t.row[ST_ROW_PAIR + p];
    row_params(r, m.pair_solref[p], m.pair_solimp[p], m.timestep, m.disableflags);
    const double mu = m.pair_friction[p];
    const double invw = m.body_invweight0[m.geom_bodyid[m.pair_geom1[p]]][0] +
                        m.body_invweight0[m.geom_bodyid[m.pair_geom2[p]]][0];
    r.margin = pair_margin_f(m, p);
    r.diag = (float)(pair_frictionless(m, p) ? invw : invw * (1.0 + mu * mu));
    if (pair_frictionless(m, p)) r.flags |= ST_CONDIM1;
    // quad 3 of a pair row (StepPairJ): with ST_CONDIM1 all the rows phase
    // reads by pair
    StepPairJ q;
    const int b1 = f.dmap[m.geom_bodyid[m.pair_geom1[p]]], b2 = f.dmap[m.geom_bodyid[m.pair_geom2[p]]];
    q.mask1 = b1 >= 0 ? m.body_dofmask[f.id[b1]] : 0u;
    q.mask2 = b2 >= 0 ? m.body_dofmask[f.id[b2]] : 0u;
    q.trees = (b1 >= 0 ? f.tree[b1] : 0) | (b2 >= 0 ? f.tree[b2] : 0) << 8 | (pair_frictionless(m, p) ? 1 << 16 : 0);
    q.mu = (float)m.pair_friction[p];
    static_assert(sizeof(q) == 16 && offsetof(StepRow, range) == 48 && sizeof(StepRow) == 64, "quad 3");
    memcpy(reinterpret_cast<char*>(&r) + 48, &q, sizeof(q));
  }
  for (int j = 0; j < m.njnt; j++) {
    StepRow& r = t.row[ST_ROW_JNT + j];
    row_params(r, m.jnt_solref[j], m.jnt_solimp[j], m.timestep, m.disableflags);
    r.margin = jnt_margin_f(m, j);
    r.diag = dof_invweight_f(m, m.jnt_dofadr[j]);
    if (jnt_limit_row(m, j)) r.flags |= ST_LIMITED;
    r.range[0] = jnt_range_f(m, j, 0);
    r.range[1] = jnt_range_f(m, j, 1);
    r.qposadr = m.jnt_qposadr[j];
    r.dofadr = m.jnt_dofadr[j];
  }
  for (int e = 0; e < m.neq; e++) {
    StepRow& r = t.row[ST_ROW_EQ + e];
    row_params(r, m.eq_solref[e], m.eq_solimp[e], m.timestep, m.disableflags);
    r.margin = 0.f;
    r.diag = eq_diag_f(m, e);
    r.qposadr = r.dofadr = -1;
  }
  return 0;
}

// Fills r from the model: every value by the expression build_dev_model
// (dev_model.h) has for the array the record replaces.  Returns 0, or -1 when
// the model exceeds the capacities.
inline int build_step_records(const mpcr_model_t& m, StepRecords& r) {
  memset(&r, 0, sizeof(r));
  if (m.npair > ST_NP || m.neq > ST_NEQ || m.njnt > ST_NJ || m.ngeom > MPCR_MAX_GEOM) return -1;
  int gmap[MPCR_MAX_GEOM];
  pair_geom_map(m, gmap);
  for (int p = 0; p < m.npair; p++) {
    StepPairSetup& s = r.pair[p];
    const int g1 = m.pair_geom1[p], g2 = m.pair_geom2[p];
    s.func = m.pair_func[p];
    s.slotadr = m.pair_slotadr[p];
    s.g1 = gmap[g1];
    s.g2 = gmap[g2];
    s.types = (m.geom_type[g1] & 255) | (m.geom_type[g2] & 255) << 8 | m.pair_ncon[p] << 16;
    s.rbound1 = (float)m.geom_rbound[g1];
    s.rbound2 = (float)m.geom_rbound[g2];
    s.margin = pair_margin_f(m, p);
    for (int k = 0; k < 3; k++) { s.size1[k] = (float)m.geom_size[g1][k]; s.size2[k] = (float)m.geom_size[g2][k]; }
  }
  for (int e = 0; e < m.neq; e++) {
    StepEq& q = r.eq[e];
    q.qadr1 = q.dadr1 = q.qadr2 = q.dadr2 = -1;
    if (m.eq_type[e] != MPCR_EQ_JOINT) continue;  // (connect: dual-arm kernels only)
    const int j1 = m.eq_obj1[e], j2 = m.eq_obj2[e];
    if (j1 < 0 || j1 >= m.njnt || j2 >= m.njnt) return -1;
    q.qadr1 = m.jnt_qposadr[j1];
    q.dadr1 = m.jnt_dofadr[j1];
    q.qpos0_1 = (float)m.qpos0[m.jnt_qposadr[j1]];
    if (j2 >= 0) {
      q.qadr2 = m.jnt_qposadr[j2];
      q.dadr2 = m.jnt_dofadr[j2];
      q.qpos0_2 = (float)m.qpos0[m.jnt_qposadr[j2]];
    }
    q.c0 = (float)m.eq_data[e][0]; q.c1 = (float)m.eq_data[e][1]; q.c2 = (float)m.eq_data[e][2];
    q.c3 = (float)m.eq_data[e][3]; q.c4 = (float)m.eq_data[e][4];
  }
  return 0;
}

}  // namespace mpcr
