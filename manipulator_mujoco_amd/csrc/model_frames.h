// model_frames.h -- the one derivation of what the step table (step_table.h)
// and the device model (dev_model.h) both need of the model's kinematic
// structure: which bodies move, where the static ones stand, each moving
// body's joint, ancestor, folded pre-joint pose, depth and tree, and the dof
// kinds.  Also the few model values both structures store, one function each,
// so neither builder has a formula of its own for them.  Plain host C++ (no
// HIP); tests/test_step_table.py and tests/test_dev_model.py run it on the CPU.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/mpcr_model.h"

namespace mpcr {

// body kinds (mpcr_device.h BK_*)
enum { ST_BK_FREE = 1, ST_BK_HINGE = 2, ST_BK_SLIDE = 3, ST_BK_WELD = 4 };

namespace step_detail {
inline void qmul(double r[4], const double a[4], const double b[4]) {
  const double t[4] = {a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                       a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                       a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
                       a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]};
  memcpy(r, t, sizeof(t));
}
inline void q2m(double m[9], const double q[4]) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  m[0] = 1 - 2 * (y * y + z * z); m[1] = 2 * (x * y - w * z); m[2] = 2 * (x * z + w * y);
  m[3] = 2 * (x * y + w * z); m[4] = 1 - 2 * (x * x + z * z); m[5] = 2 * (y * z - w * x);
  m[6] = 2 * (x * z - w * y); m[7] = 2 * (y * z + w * x); m[8] = 1 - 2 * (x * x + y * y);
}
inline void rot(double r[3], const double q[4], const double v[3]) {
  double m[9];
  q2m(m, q);
  for (int i = 0; i < 3; i++) r[i] = m[3 * i] * v[0] + m[3 * i + 1] * v[1] + m[3 * i + 2] * v[2];
}
}  // namespace step_detail

// Moving bodies (not welded to the world) are numbered in model order; the
// per-body arrays below are indexed by that number and sized by the blob's
// capacity, so any model a blob can hold fits (the builders refuse what
// exceeds their own capacities).
struct ModelFrames {
  int nbody, ntree, maxdepth;                              // moving bodies, kinematic trees, deepest chain
  int dmap[MPCR_MAX_BODY];                                 // model body -> moving body (-1: static)
  double wpos[MPCR_MAX_BODY][3], wquat[MPCR_MAX_BODY][4];  // by model body: a static body's constant world pose
  int id[MPCR_MAX_BODY];                                   // moving body -> model body
  int kind[MPCR_MAX_BODY];                                 // ST_BK_*
  int anc[MPCR_MAX_BODY];                                  // first moving ancestor (-1: static parent, or a free body)
  int jnt[MPCR_MAX_BODY];                                  // the body's (first) joint, -1: none
  int depth[MPCR_MAX_BODY], tree[MPCR_MAX_BODY];           // 1 + ancestors; trees in order of first appearance
  double bpos[MPCR_MAX_BODY][3], bquat[MPCR_MAX_BODY][4];  // pre-joint local pose, a static parent's world pose folded in
  int dof_kind[MPCR_MAX_DOF], dof_sub[MPCR_MAX_DOF];       // 0 hinge 1 slide 2 free translation 3 free rotation; free axis 0..2
};

// Returns 0, or -1 when the counts exceed the blob's own capacities.
inline int model_frames(const mpcr_model_t& m, ModelFrames& f) {
  using namespace step_detail;
  memset(&f, 0, sizeof(f));
  if (m.nbody < 1 || m.nbody > MPCR_MAX_BODY || m.nv < 0 || m.nv > MPCR_MAX_DOF) return -1;
  f.dmap[0] = -1;
  f.wquat[0][0] = 1;
  for (int b = 1; b < m.nbody; b++) {
    f.dmap[b] = m.body_weldid[b] != 0 ? f.nbody++ : -1;
    if (f.dmap[b] >= 0) { f.id[f.dmap[b]] = b; continue; }
    const int p = m.body_parentid[b];
    double r[3];
    rot(r, f.wquat[p], m.body_pos[b]);
    for (int k = 0; k < 3; k++) f.wpos[b][k] = f.wpos[p][k] + r[k];
    qmul(f.wquat[b], f.wquat[p], m.body_quat[b]);
    const double n = sqrt(f.wquat[b][0] * f.wquat[b][0] + f.wquat[b][1] * f.wquat[b][1] +
                          f.wquat[b][2] * f.wquat[b][2] + f.wquat[b][3] * f.wquat[b][3]);
    for (int k = 0; k < 4; k++) f.wquat[b][k] /= n;
  }
  int roots[MPCR_MAX_BODY];
  for (int i = 0; i < f.nbody; i++) {
    const int b = f.id[i], p = m.body_parentid[b];
    const int j = m.body_jntnum[b] ? m.body_jntadr[b] : -1;
    f.jnt[i] = j;
    f.kind[i] = j < 0 ? ST_BK_WELD
                      : (m.jnt_type[j] == MPCR_JNT_FREE ? ST_BK_FREE
                                                        : (m.jnt_type[j] == MPCR_JNT_HINGE ? ST_BK_HINGE : ST_BK_SLIDE));
    if (f.dmap[p] < 0) {  // static parent: its constant world pose folded in
      double w[3];
      rot(w, f.wquat[p], m.body_pos[b]);
      for (int k = 0; k < 3; k++) f.bpos[i][k] = f.wpos[p][k] + w[k];
      qmul(f.bquat[i], f.wquat[p], m.body_quat[b]);
      f.anc[i] = -1;
    } else {
      memcpy(f.bpos[i], m.body_pos[b], sizeof(f.bpos[i]));
      memcpy(f.bquat[i], m.body_quat[b], sizeof(f.bquat[i]));
      f.anc[i] = f.dmap[p];
    }
    if (f.kind[i] == ST_BK_FREE) f.anc[i] = -1;
    f.depth[i] = f.anc[i] < 0 ? 1 : f.depth[f.anc[i]] + 1;
    f.maxdepth = f.depth[i] > f.maxdepth ? f.depth[i] : f.maxdepth;
    int t = -1;
    for (int k = 0; k < f.ntree; k++)
      if (roots[k] == m.body_rootid[b]) t = k;
    if (t < 0) { roots[f.ntree] = m.body_rootid[b]; t = f.ntree++; }
    f.tree[i] = t;
  }
  for (int i = 0; i < m.nv; i++) {
    const int j = m.dof_jntid[i], sub = i - m.jnt_dofadr[j];
    f.dof_kind[i] = m.jnt_type[j] == MPCR_JNT_HINGE ? 0 : (m.jnt_type[j] == MPCR_JNT_SLIDE ? 1 : (sub < 3 ? 2 : 3));
    f.dof_sub[i] = sub < 3 ? sub : sub - 3;
  }
  return 0;
}

// Collision geoms (those a pair names) are numbered in order of first
// appearance over the pairs: gmap[model geom] = collision geom or -1.
// Returns their number.
inline int pair_geom_map(const mpcr_model_t& m, int gmap[MPCR_MAX_GEOM]) {
  for (int g = 0; g < MPCR_MAX_GEOM; g++) gmap[g] = -1;
  int ng = 0;
  for (int p = 0; p < m.npair; p++)
    for (int g : {m.pair_geom1[p], m.pair_geom2[p]})
      if (gmap[g] < 0) gmap[g] = ng++;
  return ng;
}

// Values the step table's rows and the device model both hold (the integer
// addresses jnt_qposadr / jnt_dofadr are copied as they are).
inline float pair_margin_f(const mpcr_model_t& m, int p) { return (float)(m.pair_margin[p] - m.pair_gap[p]); }
inline bool pair_frictionless(const mpcr_model_t& m, int p) { return m.pair_condim[p] == 1; }
inline bool jnt_limit_row(const mpcr_model_t& m, int j) {  // a limited hinge / slide joint
  return m.jnt_limited[j] && (m.jnt_type[j] == MPCR_JNT_SLIDE || m.jnt_type[j] == MPCR_JNT_HINGE);
}
inline float jnt_range_f(const mpcr_model_t& m, int j, int k) { return (float)m.jnt_range[j][k]; }
inline float jnt_margin_f(const mpcr_model_t& m, int j) { return (float)m.jnt_margin[j]; }
inline float dof_invweight_f(const mpcr_model_t& m, int i) { return (float)m.dof_invweight0[i]; }
inline float eq_diag_f(const mpcr_model_t& m, int e) {  // joint: the joints' dofs; connect: the bodies; else 0
  double diag = 0;
  if (m.eq_type[e] == MPCR_EQ_JOINT) {
    diag = m.dof_invweight0[m.jnt_dofadr[m.eq_obj1[e]]];
    if (m.eq_obj2[e] >= 0) diag += m.dof_invweight0[m.jnt_dofadr[m.eq_obj2[e]]];
  } else if (m.eq_type[e] == MPCR_EQ_CONNECT) {
    diag = m.body_invweight0[m.eq_obj1[e]][0] + m.body_invweight0[m.eq_obj2[e]][0];
  }
  return (float)diag;
}

}  // namespace mpcr
