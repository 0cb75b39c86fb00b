// convex_mpr.h -- convex support functions (hull climb, ties, start table) and Minkowski
// portal refinement of the dual-arm rollout kernels.
#pragma once
#include "../../include/mpcr_model.h"  // MPCR_LUT_R (the engine's hull start table)
#include "rollout.h"
#include "rollout_instruments.h"
#include "wave.h"
#include "vecmath.h"

namespace mpcr {

// ---------------------------------------------------------------------------
// general convex narrow phase (dual-arm class only): support functions of
// sphere / capsule / cylinder / box / mesh convex hull and Minkowski portal
// refinement, the same algorithm and tolerances as the oracle's mpr()
// (libccd MPR; one penetration contact per pair)

// gap tolerance (oracle MPR_TOL): MuJoCo's ccd_tolerance (round 3; 1e-5 before)
constexpr float kMprTol = 1e-6f;
constexpr int kMprIter = 50;  // MuJoCo's ccd_iterations cap
constexpr float kMprEps = 1.1920929e-07f;
__device__ __forceinline__ bool mpr_zero(float x) { return fabsf(x) < kMprEps; }

// Ties in the support mapping resolve as in the oracle's support(): a box /
// capsule / cylinder axis with |l_k| < kSupTie |l| contributes 0 (its face or
// segment centre: MuJoCo's mju_sign(0) = 0, widened to the fp32 rounding of a
// component that is exactly zero in fp64), and the hull climb moves to the
// neighbour that beats the current vertex the most (strictly; kSupBand > 0
// would make it the first within that many metres).
constexpr float kSupTie = 1e-6f;  // < 0: MuJoCo's mju_sign (only an exact zero is a tie)
// hull support ties (round 6, oracle HULL_TIE): vertices within this many
// metres of the climb's end are tied with it (hull_tie); 0 = the plain climb
constexpr float kHullTie = 1e-7f;
constexpr float kSupBand = 0.f;  // MuJoCo's strict climb (round 3; 1e-5 before)
__device__ __forceinline__ float tie_sign(float lk, float ln) {
  if (kSupTie < 0.f) return lk > 0.f ? 1.f : (lk < 0.f ? -1.f : 0.f);
  return fabsf(lk) < kSupTie * ln ? 0.f : (lk >= 0.f ? 1.f : -1.f);
}

// examine the neighbours of vertex v along l (unit): one must beat bn (the
// current vertex + band, then the chosen neighbour + band); -1 if none.
// Neighbour records carry (index | degree << 16), so the next round's loads
// need no lookup: the first 8 neighbours (90 % of hull vertices have <= 8)
// sit in v's NaN-padded head block (addressed by v alone, 8 independent
// loads), the rest of a longer list in hull_adjv after one hull_info load.
// Hull support ties (round 6, the oracle's hull_tie): a round also keeps
// the lowest-index neighbour within kHullTie of the current vertex (tkey:
// index << 16 | degree, the record's w bits rotated; ~0u: none).  The round
// that ends the climb thus names the climb end's lowest tied neighbour, and
// sup_finish walks on to it while one is lower (tie_round).
__device__ __forceinline__ void climb_scan(const float4 (&w)[8], const float l[3], float& bn, float4& hv, int& nb,
                                           float lo, uint32_t& tkey) {
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const float du = w[j].x * l[0] + w[j].y * l[1] + w[j].z * l[2];  // NaN pads never win
    const uint32_t wb = __float_as_uint(w[j].w);
    if (du >= lo) tkey = min(tkey, __builtin_amdgcn_alignbit(wb, wb, 16));
    if (du > bn) { bn = du + kSupBand; nb = __float_as_int(w[j].w); hv = w[j]; }
  }
}
__device__ __forceinline__ int climb_round(const DevModel* __restrict__ m, int v, int deg, const float l[3],
                                           float& best, float4& hv, uint32_t& tkey) {
  int nb = -1;
  float bn = best + kSupBand;
  const float lo = best - kHullTie;
  tkey = ~0u;
  float4 w[8];
#pragma unroll
  for (int j = 0; j < 8; j++) w[j] = m->hull_head[(size_t)v * 8 + j];
  climb_scan(w, l, bn, hv, nb, lo, tkey);
  if (deg > 8) {
    const int a = m->hull_info[v].x, last = a + deg - 1;
    for (int k0 = a + 8; k0 <= last; k0 += 8) {
#pragma unroll
      for (int j = 0; j < 8; j++) w[j] = m->hull_adjv[min(k0 + j, last)];  // repeats of the last never win twice
      climb_scan(w, l, bn, hv, nb, lo, tkey);
    }
  }
  if (nb >= 0) best = bn - kSupBand;
  return nb;
}

// The support of a hull on a tie.  When the direction is normal (to
// ~kHullTie) to an edge or a face of the hull, every vertex of it is a
// maximum, and which one the climb reaches depends on where it started (the
// start table's cell, the pair's hint) and on the last bits of the dot
// products (fp32 and fp64 pick differently).  From the climb's end v the
// support walks to the lowest-index neighbour within kHullTie of v's value
// while that neighbour's index is lower: the tie's lowest index from
// whichever of its vertices the climb reached (the oracle's hull_tie), so a
// start table's resolution stays a performance choice, not a parity change
// (tests/test_hull_ties.py).  One walk round, out of line with scalar
// arguments (its call's spills stay on this path; inlined, or folded into
// the climb loop, the walk cost the hot climb registers or time): v's
// coordinates and the key of its lowest tied neighbour.
struct TieStep { float x, y, z; uint32_t tkey; };  // v's coordinates, its lowest tied neighbour's key
__device__ __noinline__ TieStep tie_round(const DevModel* __restrict__ m, int v, int deg, float lo, float l0,
                                          float l1, float l2) {
  uint32_t tkey = ~0u;
  const float l[3] = {l0, l1, l2};
  float4 w[8];
  const float4 x = m->hull_vert[v];
#pragma unroll
  for (int j = 0; j < 8; j++) w[j] = m->hull_head[(size_t)v * 8 + j];  // the head block's loads in flight together
  float bn = 3e38f;  // (no neighbour is climbed to)
  float4 hv;
  int nb;
  climb_scan(w, l, bn, hv, nb, lo, tkey);
  if (deg > 8) {
    const int a = m->hull_info[v].x, last = a + deg - 1;
    for (int k0 = a + 8; k0 <= last; k0 += 8) {
#pragma unroll
      for (int j = 0; j < 8; j++) w[j] = m->hull_adjv[min(k0 + j, last)];
      climb_scan(w, l, bn, hv, nb, lo, tkey);
    }
  }
  return TieStep{x.x, x.y, x.z, tkey};
}

// cube-map cell of a local direction (the engine's start table order,
// engine.hip hull_start_table; oracle lut_cell): major axis (lowest on ties), its sign, the other two components
// (cyclic order) over |l_axis| in MPCR_LUT_R bins
template <int R = MPCR_LUT_R>
__device__ __forceinline__ int lut_cell(const float l[3]) {
  const float a0 = fabsf(l[0]), a1 = fabsf(l[1]), a2 = fabsf(l[2]);
  const int ax = (a0 >= a1 && a0 >= a2) ? 0 : (a1 >= a2 ? 1 : 2);
  const float lax = ax == 0 ? l[0] : (ax == 1 ? l[1] : l[2]);
  const float lu = ax == 0 ? l[1] : (ax == 1 ? l[2] : l[0]);
  const float lv = ax == 0 ? l[2] : (ax == 1 ? l[0] : l[1]);
  const float la = fabsf(lax);
  if (!(la > 0.f)) return 0;
  const int iu = min(max((int)floorf((lu / la + 1.f) * 0.5f * R), 0), R - 1);
  const int iv = min(max((int)floorf((lv / la + 1.f) * 0.5f * R), 0), R - 1);
  return (2 * ax + (lax < 0.f ? 1 : 0)) * R * R + iu * R + iv;
}

// hint: hull vertex the previous query on this geom ended at (-1: none); the
// climb starts there (successive MPR directions are close)
// org (nullable): the result relative to org, with (geom centre - org)
// formed first -- MPR works relative to the second geom's centre, so the
// Minkowski points carry cm-scale rounding instead of world-scale (1 m) rounding
//
// A query runs in two parts so a caller can put two of them in flight
// together (MPR's support pair: round 5): sup_start issues the first loads
// of a mesh query -- the start table cell of the direction and the hint
// vertex, independent of each other (the hint's index is clamped to the
// hull: a query without one loads the hull's first vertex and ignores it) --
// and sup_finish consumes them: the hint if it beats the table vertex, then
// the climb (none from an exact cell, engine.hip).  Same values and
// comparisons as one call, so bitwise the same support point.
struct SupQ {
  float l[3], lu[3], ln;
  float4 hv, hh;
  int type, la;
};
// a geom's per-query constants (type, table, first hull vertex), loaded once
// per MPR run instead of in front of every support query
struct GeomQ { int type, la, h0; };
__device__ __forceinline__ GeomQ geom_q(const DevModel* __restrict__ m, int g) {
  GeomQ q{m->geom_type[g], m->geom_lutadr[g], m->geom_hulladr[g]};
  asm volatile("" : "+v"(q.type), "+v"(q.la), "+v"(q.h0));  // kept in registers, not re-loaded per query
  return q;
}
template <class S>
__device__ __forceinline__ void sup_start(const DevModel* __restrict__ m, const S& s, int g, const float dir[3],
                                          int hint, SupQ& q, const GeomQ* gq = nullptr) {
  const float* R = s.gxmat[g];
  mtv(q.l, R, dir);
  q.ln = sqrtf(dot3(q.l, q.l));
  q.type = gq ? gq->type : m->geom_type[g];
  if (q.type == 7) {
    const float il = q.ln > 0.f ? 1.f / q.ln : 0.f;
    q.lu[0] = q.l[0] * il; q.lu[1] = q.l[1] * il; q.lu[2] = q.l[2] * il;
    q.la = gq ? gq->la : m->geom_lutadr[g];
    const int h0 = gq ? gq->h0 : m->geom_hulladr[g];
    q.hv = q.la >= 0 ? m->hull_lut[q.la + lut_cell(q.l)] : m->hull_vert[h0];
    q.hh = m->hull_vert[hint >= 0 ? hint : h0];
  }
}
// MPCR_SAT_TIES 1: the SAT's value-only queries walk the ties too (A/B of
// the start independence, tools/scramble_check.py)
#ifndef MPCR_SAT_TIES
#define MPCR_SAT_TIES 0
#endif
template <class S>
// ties = false: the caller uses the support value only (the SAT's
// separations), which any tied vertex gives to within kHullTie
__device__ __forceinline__ void sup_finish(const DevModel* __restrict__ m, const S& s, int g, SupQ& q, float out[3],
                                           int& hint, const float* org, bool ties = true) {
  const float* R = s.gxmat[g];
  const float* sz = m->geom_size[g];
  const float* l = q.l;
  const float ln = q.ln;
  const int type = q.type;
  float p[3] = {0.f, 0.f, 0.f};
  if (type == 2 || type == 3) {  // sphere, capsule
    if (ln > 0.f) { p[0] = sz[0] * l[0] / ln; p[1] = sz[0] * l[1] / ln; p[2] = sz[0] * l[2] / ln; }
    if (type == 3) p[2] += tie_sign(l[2], ln) * sz[1];
  } else if (type == 5) {  // cylinder
    const float r = sqrtf(l[0] * l[0] + l[1] * l[1]);
    if (r > fmaxf(kSupTie, 0.f) * ln) { p[0] = sz[0] * l[0] / r; p[1] = sz[0] * l[1] / r; }
    p[2] = tie_sign(l[2], ln) * sz[1];
  } else if (type == 6) {  // box
    p[0] = tie_sign(l[0], ln) * sz[0];
    p[1] = tie_sign(l[1], ln) * sz[1];
    p[2] = tie_sign(l[2], ln) * sz[2];
  } else if (type == 7) {  // mesh hull: steepest ascent on the vertex graph
    // start: the table vertex of l's cube-map cell, or the hint (where the
    // previous query on this pair ended) when it beats that by the band
    const float* lu = q.lu;
    float4 hv = q.hv;
    const int hw = __float_as_int(hv.w);
    int v = q.la >= 0 ? (hw & 0x7fff) : m->geom_hulladr[g];
    if (!(q.la >= 0 && (hw & 0x8000))) {  // not an exact cell (engine.hip): the hint, then the climb
      int deg = q.la >= 0 ? (hw >> 16) : hw;
      float best = hv.x * lu[0] + hv.y * lu[1] + hv.z * lu[2];
      if (hint >= 0) {
        const float4 hh = q.hh;
        const float bh = hh.x * lu[0] + hh.y * lu[1] + hh.z * lu[2];
        // (on equal values the hint: after a tie walk it is the tie's lowest
        // index, so the climb then ends where it starts, with no walk)
        if (bh >= best + kSupBand) { v = hint; hv = hh; deg = __float_as_int(hh.w); best = bh; }
      }
      uint32_t tkey = ~0u;
      for (int guard = 0; guard < 4096; guard++) {
        PROF_COUNT(m, 19);
        const int nb = climb_round(m, v, deg, lu, best, hv, tkey);
        if (nb < 0) break;
        v = nb & 0xffff;
        deg = nb >> 16;
      }
      if (kHullTie > 0.f && ties && (int)(tkey >> 16) < v) {  // a lower-index tied neighbour: walk (hull_tie)
        const float lo = best - kHullTie;
        for (int guard = 0; guard < 64 && (int)(tkey >> 16) < v; guard++) {
          v = tkey >> 16;
          const TieStep ts = tie_round(m, v, tkey & 0xffff, lo, lu[0], lu[1], lu[2]);
          hv.x = ts.x; hv.y = ts.y; hv.z = ts.z;
          tkey = ts.tkey;
        }
      }
    }
    p[0] = hv.x; p[1] = hv.y; p[2] = hv.z;
    hint = v;
  }
  mv(out, R, p);
  if (org) {
    out[0] += s.gxpos[g][0] - org[0]; out[1] += s.gxpos[g][1] - org[1]; out[2] += s.gxpos[g][2] - org[2];
  } else {
    out[0] += s.gxpos[g][0]; out[1] += s.gxpos[g][1]; out[2] += s.gxpos[g][2];
  }
}
template <class S>
__device__ __forceinline__ void support_geom(const DevModel* __restrict__ m, const S& s, int g, const float dir[3],
                                             float out[3], int& hint, const float* org = nullptr, bool ties = true) {
  SupQ q;
  sup_start(m, s, g, dir, hint, q);
  sup_finish(m, s, g, q, out, hint, org, ties);
}

struct MprPt { float v[3], a[3], b[3]; };

template <class S>
__device__ __forceinline__ void mpr_support(const DevModel* __restrict__ m, const S& s, int g1, int g2,
                                            const float dir[3], MprPt& o, int (&hint)[2], float* trace = nullptr,
                                            const GeomQ* gq = nullptr) {
  const float nd[3] = {-dir[0], -dir[1], -dir[2]};
  SupQ q1, q2;  // both queries' first loads in flight together
  PROF_COUNT(m, 20);
  sup_start(m, s, g1, dir, hint[0], q1, gq);
  sup_start(m, s, g2, nd, hint[1], q2, gq ? gq + 1 : nullptr);
  sup_finish(m, s, g1, q1, o.a, hint[0], s.gxpos[g2]);  // relative to g2's centre
  sup_finish(m, s, g2, q2, o.b, hint[1], s.gxpos[g2]);
  o.v[0] = o.a[0] - o.b[0]; o.v[1] = o.a[1] - o.b[1]; o.v[2] = o.a[2] - o.b[2];
  if (trace) {
    const int q = (int)trace[47];
    if (q < 32) { trace[48 + 2 * q] = (float)hint[0]; trace[49 + 2 * q] = (float)hint[1]; trace[47] = (float)(q + 1); }
  }
}
__device__ __forceinline__ void nrm3(float v[3]) {
  const float n = sqrtf(dot3(v, v));
  if (n > 0.f) { v[0] /= n; v[1] /= n; v[2] /= n; }
}
__device__ __forceinline__ void mpr_dir(const MprPt p[4], float dir[3]) {
  float a[3] = {p[2].v[0] - p[1].v[0], p[2].v[1] - p[1].v[1], p[2].v[2] - p[1].v[2]};
  float b[3] = {p[3].v[0] - p[1].v[0], p[3].v[1] - p[1].v[1], p[3].v[2] - p[1].v[2]};
  cross(dir, a, b);
  nrm3(dir);
}
__device__ __forceinline__ bool mpr_reach(const MprPt p[4], const MprPt& v4, const float dir[3], float tol) {
  const float d4 = dot3(v4.v, dir);
  const float t = fminf(d4 - dot3(p[1].v, dir), fminf(d4 - dot3(p[2].v, dir), d4 - dot3(p[3].v, dir)));
  return t < tol;
}
__device__ __forceinline__ void mpr_expand(MprPt p[4], const MprPt& v4) {
  float x[3];
  cross(x, v4.v, p[0].v);
  if (dot3(p[1].v, x) > 0.f) {
    if (dot3(p[2].v, x) > 0.f) p[1] = v4; else p[3] = v4;
  } else {
    if (dot3(p[3].v, x) > 0.f) p[2] = v4; else p[1] = v4;
  }
}
__device__ __forceinline__ void tri_closest(const float a[3], const float b[3], const float c[3], float out[3]) {
  float ab[3], ac[3], ap[3], bp[3], cp[3];
#pragma unroll
  for (int k = 0; k < 3; k++) { ab[k] = b[k] - a[k]; ac[k] = c[k] - a[k]; ap[k] = -a[k]; bp[k] = -b[k]; cp[k] = -c[k]; }
  const float d1 = dot3(ab, ap), d2 = dot3(ac, ap);
  if (d1 <= 0.f && d2 <= 0.f) { out[0] = a[0]; out[1] = a[1]; out[2] = a[2]; return; }
  const float d3 = dot3(ab, bp), d4 = dot3(ac, bp);
  if (d3 >= 0.f && d4 <= d3) { out[0] = b[0]; out[1] = b[1]; out[2] = b[2]; return; }
  const float vc = d1 * d4 - d3 * d2;
  if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {
    const float t = d1 / (d1 - d3);
    out[0] = a[0] + t * ab[0]; out[1] = a[1] + t * ab[1]; out[2] = a[2] + t * ab[2];
    return;
  }
  const float d5 = dot3(ab, cp), d6 = dot3(ac, cp);
  if (d6 >= 0.f && d5 <= d6) { out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; return; }
  const float vb = d5 * d2 - d1 * d6;
  if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {
    const float t = d2 / (d2 - d6);
    out[0] = a[0] + t * ac[0]; out[1] = a[1] + t * ac[1]; out[2] = a[2] + t * ac[2];
    return;
  }
  const float va = d3 * d6 - d5 * d4;
  if (va <= 0.f && (d4 - d3) >= 0.f && (d5 - d6) >= 0.f) {
    const float t = (d4 - d3) / ((d4 - d3) + (d5 - d6));
#pragma unroll
    for (int k = 0; k < 3; k++) out[k] = b[k] + t * (c[k] - b[k]);
    return;
  }
  // face region: the plane projection n (n.a) / |n|^2 (the oracle's
  // tri_closest): the barycentric a + v ab + w ac cancels catastrophically in
  // fp32 for MPR's cm-sized final portal around a sub-mm penetration
  float n[3];
  cross(n, ab, ac);
  const float sc = dot3(n, a) / dot3(n, n);
#pragma unroll
  for (int k = 0; k < 3; k++) out[k] = n[k] * sc;
  (void)va; (void)vb; (void)vc;
}

// returns true and (depth, dir g1 -> g2, pos) when the geoms overlap.
// Zero tests are geometric and in metres, identical in the oracle: libccd's
// are absolute DBL_EPSILON tests on lengths, areas and volumes alike, which
// in fp32 call two cm-scale vectors parallel (|v0 x v1|^2 ~ 1e-8 < eps);
// here a length is zero below kMprEps (1.2e-7 m, fp32 resolution of world
// coordinates), two vectors are parallel when one passes within kMprEps of
// the other's line, and a point lies on a plane within kMprEps of it.
template <class S>
__device__ bool mpr_lane(const DevModel* __restrict__ m, const S& s, int g1, int g2, float& depth, float dir[3],
                         float pos[3], int (&hint)[2], float* trace = nullptr) {
  MprPt p[4], v4;
  float va[3], vb[3], dd;
  const float tol = kMprTol;
  const GeomQ gqa[2] = {geom_q(m, g1), geom_q(m, g2)};
  const GeomQ* const gq = gqa;
  // point x off the plane through the origin with (unnormalised) normal c by more than kMprEps
  auto off_plane = [](float x, const float c[3]) { return fabsf(x) >= kMprEps * sqrtf(dot3(c, c)); };
#pragma unroll
  for (int k = 0; k < 3; k++) {  // the frame of the Minkowski points: origin at g2's centre
    p[0].a[k] = s.gxpos[g1][k] - s.gxpos[g2][k];
    p[0].b[k] = 0.f;
    p[0].v[k] = p[0].a[k];
  }
  if (mpr_zero(p[0].v[0]) && mpr_zero(p[0].v[1]) && mpr_zero(p[0].v[2])) p[0].v[0] += 10.f * kMprEps;
  dir[0] = -p[0].v[0]; dir[1] = -p[0].v[1]; dir[2] = -p[0].v[2];
  nrm3(dir);
  mpr_support(m, s, g1, g2, dir, p[1], hint, trace, gq);
  dd = dot3(p[1].v, dir);
  if (mpr_zero(dd) || dd < 0.f) return false;
  cross(dir, p[0].v, p[1].v);
  {
    const float thr = kMprEps * (sqrtf(dot3(p[0].v, p[0].v)) + sqrtf(dot3(p[1].v, p[1].v)));
    if (dot3(dir, dir) < thr * thr) {  // v1 on the ray from v0 through the origin
#pragma unroll
      for (int k = 0; k < 3; k++) pos[k] = 0.5f * (p[1].a[k] + p[1].b[k]) + s.gxpos[g2][k];
      if (mpr_zero(p[1].v[0]) && mpr_zero(p[1].v[1]) && mpr_zero(p[1].v[2])) {
        depth = 0.f;
        dir[0] = dir[1] = dir[2] = 0.f;
      } else {
        dir[0] = p[1].v[0]; dir[1] = p[1].v[1]; dir[2] = p[1].v[2];
        depth = sqrtf(dot3(dir, dir));
        nrm3(dir);
      }
      return true;
    }
  }
  nrm3(dir);
  mpr_support(m, s, g1, g2, dir, p[2], hint, trace, gq);
  dd = dot3(p[2].v, dir);
  if (mpr_zero(dd) || dd < 0.f) return false;
#pragma unroll
  for (int k = 0; k < 3; k++) { va[k] = p[1].v[k] - p[0].v[k]; vb[k] = p[2].v[k] - p[0].v[k]; }
  cross(dir, va, vb);
  nrm3(dir);
  if (dot3(dir, p[0].v) > 0.f) {
    const MprPt t = p[1]; p[1] = p[2]; p[2] = t;
    dir[0] = -dir[0]; dir[1] = -dir[1]; dir[2] = -dir[2];
  }
  for (int guard = 0;; guard++) {
    if (guard > kMprIter) return false;
    mpr_support(m, s, g1, g2, dir, p[3], hint, trace, gq);
    dd = dot3(p[3].v, dir);
    if (mpr_zero(dd) || dd < 0.f) return false;
    bool cont = false;
    cross(va, p[1].v, p[3].v);
    dd = dot3(va, p[0].v);
    if (dd < 0.f && off_plane(dd, va)) { p[2] = p[3]; cont = true; }
    if (!cont) {
      cross(va, p[3].v, p[2].v);
      dd = dot3(va, p[0].v);
      if (dd < 0.f && off_plane(dd, va)) { p[1] = p[3]; cont = true; }
    }
    if (trace) trace[9] = (float)guard;
    if (!cont) break;
#pragma unroll
    for (int k = 0; k < 3; k++) { va[k] = p[1].v[k] - p[0].v[k]; vb[k] = p[2].v[k] - p[0].v[k]; }
    cross(dir, va, vb);
    nrm3(dir);
  }
  for (int it = 0;; it++) {
    if (trace) trace[10] = (float)it;
    mpr_dir(p, dir);
    dd = dot3(dir, p[1].v);
    if (mpr_zero(dd) || dd > 0.f) break;
    mpr_support(m, s, g1, g2, dir, v4, hint, trace, gq);
    dd = dot3(v4.v, dir);
    if (!(mpr_zero(dd) || dd > 0.f) || mpr_reach(p, v4, dir, tol) || it > kMprIter) return false;
    mpr_expand(p, v4);
  }
  for (int it = 0;; it++) {
    if (trace) trace[11] = (float)it;
    mpr_dir(p, dir);
    mpr_support(m, s, g1, g2, dir, v4, hint, trace, gq);
    if (mpr_reach(p, v4, dir, tol) || it > kMprIter) break;
    mpr_expand(p, v4);
  }
  if (trace)
    for (int i = 0; i < 4; i++)
      for (int k = 0; k < 3; k++) {
        trace[12 + 9 * i + k] = p[i].v[k];
        trace[12 + 9 * i + 3 + k] = p[i].a[k];
        trace[12 + 9 * i + 6 + k] = p[i].b[k];
      }
  float w[3];
  tri_closest(p[1].v, p[2].v, p[3].v, w);
  depth = sqrtf(dot3(w, w));
  if (mpr_zero(depth)) { dir[0] = dir[1] = dir[2] = 0.f; }
  else { dir[0] = w[0] / depth; dir[1] = w[1] / depth; dir[2] = w[2] / depth; }
  float pd[3], b[4], x[3];
  {
    float e1[3] = {p[2].v[0] - p[1].v[0], p[2].v[1] - p[1].v[1], p[2].v[2] - p[1].v[2]};
    float e2[3] = {p[3].v[0] - p[1].v[0], p[3].v[1] - p[1].v[1], p[3].v[2] - p[1].v[2]};
    cross(pd, e1, e2);  // portal normal, |pd| = twice the portal's area
  }
  cross(x, p[2].v, p[3].v); b[0] = dot3(x, p[1].v);
  cross(x, p[3].v, p[2].v); b[1] = dot3(x, p[0].v);
  cross(x, p[0].v, p[1].v); b[2] = dot3(x, p[3].v);
  cross(x, p[2].v, p[1].v); b[3] = dot3(x, p[0].v);
  float sum = b[0] + b[1] + b[2] + b[3];
  // sum = 6 x the tetrahedron's volume: degenerate when v0 lies within kMprEps of the portal's plane
  if (!off_plane(sum, pd) || sum < 0.f) {
    nrm3(pd);
    b[0] = 0.f;
    cross(x, p[2].v, p[3].v); b[1] = dot3(x, pd);
    cross(x, p[3].v, p[1].v); b[2] = dot3(x, pd);
    cross(x, p[1].v, p[2].v); b[3] = dot3(x, pd);
    sum = b[1] + b[2] + b[3];
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    float pa = 0.f, pb = 0.f;
#pragma unroll
    for (int i = 0; i < 4; i++) { pa += b[i] * p[i].a[k]; pb += b[i] * p[i].b[k]; }
    pos[k] = 0.5f * (pa + pb) / sum + s.gxpos[g2][k];
  }
  return true;
}

}  // namespace mpcr
