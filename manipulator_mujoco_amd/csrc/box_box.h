// box_box.h -- the wave-cooperative box-box narrow phase of the rollout kernel.
#pragma once
#include "rollout.h"
#include "wave.h"
#include "vecmath.h"
#include "narrow_lane.h"

namespace mpcr {

// Box-box, wave-cooperative (one pair, all 64 lanes, uniform control flow):
// lanes 0..14 evaluate the 15 separating axes, the reference-face clipping
// (Sutherland-Hodgman against the 4 side planes) runs with one lane per
// polygon edge and ballot compaction, the >4 selection is done on uniform
// values.  Same definitions and orders as the oracle's col_box_box.
// Appends up to 4 contacts to the active list.  Must be called by all lanes.
template <class S>
__device__ __forceinline__ void box_box_wave(const DevModel* __restrict__ m, S& s, int p, int lane) {
  const int g1 = m->pair_g1[p], g2 = m->pair_g2[p];
  const float margin = m->pair_margin[p];
  float x1[3], x2[3], axA[3][3], axB[3][3], t[3], ha[3], hb[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    x1[c] = s.gxpos[g1][c];
    x2[c] = s.gxpos[g2][c];
    t[c] = x2[c] - x1[c];
    ha[c] = m->geom_size[g1][c];
    hb[c] = m->geom_size[g2][c];
  }
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int c = 0; c < 3; c++) { axA[i][c] = s.gxmat[g1][3 * c + i]; axB[i][c] = s.gxmat[g2][3 * c + i]; }
  // ---- separating axes, one per lane
  float L[3] = {0.f, 0.f, 1.f}, sep = -3e38f;
  bool valid = false;
  // (per-lane axes read from the LDS frames by index: no select chains)
  if (lane < 6) {
    const float* R = s.gxmat[lane < 3 ? g1 : g2];
    const int ia = lane < 3 ? lane : lane - 3;
#pragma unroll
    for (int c = 0; c < 3; c++) L[c] = R[3 * c + ia];
    valid = true;
  } else if (lane < 15) {
    const int i = (lane - 6) / 3, j = (lane - 6) % 3;
    float ai[3], bj[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      ai[c] = s.gxmat[g1][3 * c + i];
      bj[c] = s.gxmat[g2][3 * c + j];
    }
    cross(L, ai, bj);
    const float l = sqrtf(dot3(L, L));
    valid = l >= 1e-6f;
    if (valid) { L[0] /= l; L[1] /= l; L[2] /= l; }
  }
  if (valid) {
    float ra = 0.f, rb = 0.f;
#pragma unroll
    for (int k = 0; k < 3; k++) { ra += ha[k] * fabsf(dot3(axA[k], L)); rb += hb[k] * fabsf(dot3(axB[k], L)); }
    sep = fabsf(dot3(t, L)) - ra - rb;
  }
  float best_face = -1e30f, best_edge = -1e30f;
  int face_id = -1, edge_lane = -1;
#pragma unroll
  for (int a = 0; a < 6; a++) {
    const float v = rdlane(sep, a);
    if (v > best_face) { best_face = v; face_id = a; }
  }
#pragma unroll
  for (int a = 6; a < 15; a++) {
    const float v = rdlane(sep, a);
    if (v > -1e30f && v > best_edge) { best_edge = v; edge_lane = a; }
  }
  const float best = fmaxf(best_face, best_edge);
  if (!(best < margin)) return;
  const bool use_edge = edge_lane >= 0 && best_edge > 0.95f * best_face + 1e-5f;
  const int src = use_edge ? edge_lane : face_id;
  float n[3] = {rdlane(L[0], src), rdlane(L[1], src), rdlane(L[2], src)};
  const float sg = dot3(t, n) >= 0.f ? 1.f : -1.f;
  n[0] *= sg; n[1] *= sg; n[2] *= sg;
  const int base = s.ncon;
  sync();
  if (use_edge) {
    const int ei = (edge_lane - 6) / 3, ej = (edge_lane - 6) % 3;
    float pa[3], pb[3], da[3], db[3];
#pragma unroll
    for (int c = 0; c < 3; c++) { pa[c] = x1[c]; pb[c] = x2[c]; }
#pragma unroll
    for (int k = 0; k < 3; k++) {
      if (k != ei) {
        const float s_ = dot3(n, axA[k]) >= 0.f ? 1.f : -1.f;
#pragma unroll
        for (int c = 0; c < 3; c++) pa[c] += s_ * ha[k] * axA[k][c];
      }
      if (k != ej) {
        const float s_ = dot3(n, axB[k]) >= 0.f ? -1.f : 1.f;
#pragma unroll
        for (int c = 0; c < 3; c++) pb[c] += s_ * hb[k] * axB[k][c];
      }
    }
    const float hae = m->geom_size[g1][ei], hbe = m->geom_size[g2][ej];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const float ae = s.gxmat[g1][3 * c + ei], be = s.gxmat[g2][3 * c + ej];
      pa[c] -= hae * ae; da[c] = 2.f * hae * ae;
      pb[c] -= hbe * be; db[c] = 2.f * hbe * be;
    }
    float sc, uc;
    seg_seg(pa, da, pb, db, &sc, &uc);
    if (lane == 0 && base < S::MAXACT) {
      float f[9];
      make_frame(f, n);
#pragma unroll
      for (int c = 0; c < 3; c++) s.con_pos[base][c] = 0.5f * (pa[c] + sc * da[c] + pb[c] + uc * db[c]);
#pragma unroll
      for (int e = 0; e < S::FRAMEW; e++) s.con_frame[base][e] = f[e];
      s.con_dist[base] = best_edge;
      s.con_pair[base] = p;
    }
    sync();
    if (lane == 0) s.ncon = base + 1;
    sync();
    return;
  }
  // ---- face contact: reference box owns the face axis.  The run-time axis
  // indices address the boxes' LDS frames and model sizes directly (no
  // select chains, nothing in scratch); same values as the registers above.
  const bool refA = face_id < 3;
  const int fi = refA ? face_id : face_id - 3;
  const int gr = refA ? g1 : g2, gn = refA ? g2 : g1;
  const float* Rr = s.gxmat[gr];  // axis k of a box: (R[k], R[3 + k], R[6 + k])
  const float* Ri = s.gxmat[gn];
  const float* hr = m->geom_size[gr];
  const float* hi = m->geom_size[gn];
  float cr[3], ci[3], nf[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    cr[c] = s.gxpos[gr][c];
    ci[c] = s.gxpos[gn][c];
    nf[c] = refA ? n[c] : -n[c];
  }
  const float d0 = fabsf(Ri[0] * nf[0] + Ri[3] * nf[1] + Ri[6] * nf[2]);
  const float d1 = fabsf(Ri[1] * nf[0] + Ri[4] * nf[1] + Ri[7] * nf[2]);
  const float d2 = fabsf(Ri[2] * nf[0] + Ri[5] * nf[1] + Ri[8] * nf[2]);
  int ki = 0;
  float bestdot = d0;
  if (d1 > bestdot) { bestdot = d1; ki = 1; }
  if (d2 > bestdot) { bestdot = d2; ki = 2; }
  const int u = ki == 0 ? 1 : (ki == 1 ? 2 : 0), v = ki == 0 ? 2 : (ki == 1 ? 0 : 1);
  float Ik[3], Iu[3], Iv[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    Ik[c] = Ri[3 * c + ki];
    Iu[c] = Ri[3 * c + u];
    Iv[c] = Ri[3 * c + v];
  }
  const float hk = hi[ki], hu = hi[u], hv = hi[v];
  const float si = dot3(Ik, nf) > 0.f ? -1.f : 1.f;
  if (lane < 4) {
    const float su = (lane == 0 || lane == 3) ? 1.f : -1.f, sv = lane < 2 ? 1.f : -1.f;
#pragma unroll
    for (int k = 0; k < 3; k++) s.poly[0][lane][k] = ci[k] + si * hk * Ik[k] + su * hu * Iu[k] + sv * hv * Iv[k];
  }
  int np = 4, cur = 0;
  // fast path: an incident face wholly inside the reference face's 4 side
  // planes (an object resting inside a table top) passes every clip unchanged
  // -- Sutherland-Hodgman keeps each vertex and adds no crossing -- so the 4
  // sequential clips are skipped for exactly the same polygon
  bool inside = true;
  sync();
  if (lane < 4) {
    const float P[3] = {s.poly[0][lane][0], s.poly[0][lane][1], s.poly[0][lane][2]};
#pragma unroll
    for (int pl = 0; pl < 4; pl++) {  // the clip loop's own dp expression
      const int ax = (fi + 1 + (pl >> 1)) % 3;
      const float sgn = (pl & 1) ? -1.f : 1.f;
      const float Ra[3] = {Rr[ax], Rr[3 + ax], Rr[6 + ax]};
      const float cra = dot3(cr, Ra);
      inside = inside && sgn * (dot3(P, Ra) - cra) - hr[ax] <= 0.f;
    }
  }
  if (__ballot(!inside) == 0ull) np = -np;  // marker: skip the clips
  for (int pl = 0; pl < 4 && np > 0; pl++) {
    sync();
    const int ax = (fi + 1 + (pl >> 1)) % 3;
    const float sgn = (pl & 1) ? -1.f : 1.f;
    const float Ra[3] = {Rr[ax], Rr[3 + ax], Rr[6 + ax]};
    const float hax = hr[ax];
    const float cra = dot3(cr, Ra);
    float P[3] = {0.f, 0.f, 0.f}, Q[3] = {0.f, 0.f, 0.f}, dp = 0.f, dq = 0.f;
    int e0 = 0, e1 = 0;
    if (lane < np) {
      const int c2 = lane + 1 == np ? 0 : lane + 1;
#pragma unroll
      for (int k = 0; k < 3; k++) { P[k] = s.poly[cur][lane][k]; Q[k] = s.poly[cur][c2][k]; }
      dp = sgn * (dot3(P, Ra) - cra) - hax;
      dq = sgn * (dot3(Q, Ra) - cra) - hax;
      e0 = dp <= 0.f;
      e1 = (dp < 0.f && dq > 0.f) || (dp > 0.f && dq < 0.f);
    }
    int tot;
    const int o = wscan_excl(e0 + e1, tot);
    if (e0) {
#pragma unroll
      for (int k = 0; k < 3; k++) s.poly[cur ^ 1][o][k] = P[k];
    }
    if (e1) {
      const float wgt = dp / (dp - dq);
#pragma unroll
      for (int k = 0; k < 3; k++) s.poly[cur ^ 1][o + e0][k] = P[k] + wgt * (Q[k] - P[k]);
    }
    np = tot;
    cur ^= 1;
  }
  if (np < 0) np = -np;
  sync();
  if (np == 0) return;
  const float hrf = hr[fi];
  float depth = -3e38f;
  bool keep = false;
  if (lane < np) {
    const float rel[3] = {s.poly[cur][lane][0] - cr[0], s.poly[cur][lane][1] - cr[1], s.poly[cur][lane][2] - cr[2]};
    depth = hrf - dot3(rel, nf);
    keep = -depth < margin;
  }
  const unsigned long long km = __ballot(keep);
  const int nkeep = __popcll(km);
  if (nkeep == 0) return;
  const int rank = lanes_below(km);  // position of this lane among the kept points
  int slot = keep ? rank : -1;
  int npick = nkeep;
  if (nkeep > 4) {
    // deepest kept point (first maximum), then evenly spaced around the polygon
    int d0 = 0;
    float dbest = -3e38f;
#pragma unroll
    for (int c = 0; c < 8; c++) {
      const float dc = rdlane(depth, c);
      const bool kc = (km >> c) & 1ull;
      const int rc = __popcll(km & ((1ull << c) - 1ull));
      if (kc && dc > dbest) { dbest = dc; d0 = rc; }
    }
    slot = -1;
#pragma unroll
    for (int q = 0; q < 4; q++)
      if (keep && rank == (d0 + q * nkeep / 4) % nkeep) slot = q;
    npick = 4;
  }
  if (slot >= 0 && base + slot < S::MAXACT) {
    const int o = base + slot;
    float f[9];
    make_frame(f, n);
#pragma unroll
    for (int k = 0; k < 3; k++) s.con_pos[o][k] = s.poly[cur][lane][k] + nf[k] * 0.5f * depth;
#pragma unroll
    for (int e = 0; e < S::FRAMEW; e++) s.con_frame[o][e] = f[e];
    s.con_dist[o] = -depth;
    s.con_pair[o] = p;
  }
  sync();
  if (lane == 0) s.ncon = base + npick;
  sync();
}

}  // namespace mpcr
