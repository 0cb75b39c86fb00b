// manifold.h -- the plane-mesh and polyhedron contact manifolds of the dual-arm rollout
// kernels, wave-cooperative.
#pragma once
#include "convex_mpr.h"

namespace mpcr {

__device__ __forceinline__ bool beats(float v, float best) { return v > best + 1e-4f * fabsf(best) + 1e-12f; }
__device__ __forceinline__ bool near_max(float v, float mx) { return v >= mx - (1e-4f * fabsf(mx) + 1e-12f); }
__device__ __forceinline__ float wmax(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// Both manifold callees below are inlined: 241 -> 235 VGPRs, no scratch (the
// contact arrays stay in registers), C4 48.6 -> 46.7 ms
// Plane-mesh manifold (MJX plane_convex / _manifold_points, the oracle's
// col_plane_mesh), wave-cooperative: every lane calls it with the same pair
// (mesh g, plane normal n through xp, penetration depth) and lane q receives
// the contacts.  The hull's vertices are scanned 64 at a time -- a first /
// last ballot for the penetrating set, then per pick a wave max and a ballot
// for its first index within the tie band (near_max, as the oracle) -- instead
// of four serial per-lane scans (a 2691-vertex hull touching the table made a
// handful of dual-arm candidates 3x slower than the rest).
template <class S>
__device__ __forceinline__
void plane_mesh_manifold_wave(const DevModel* __restrict__ m_, const S& s, int g,
                                                      const float n_[3], const float* xp_, float depth, int q, int lane,
                                                      float dist[4], float pos[4][3], float nrm[4][3], int& nsl) {
  const MPCR_GMEM DevModel* __restrict__ m = uniform_model(m_);
  ASSUME_LDS(&s); ASSUME_PRIVATE(dist); ASSUME_PRIVATE(pos); ASSUME_PRIVATE(nrm); ASSUME_PRIVATE(&nsl);
  const float n[3] = {n_[0], n_[1], n_[2]}, xp[3] = {xp_[0], xp_[1], xp_[2]};  // in registers (no alias reloads)
  const float* R = s.gxmat[g];
  const float* xg = s.gxpos[g];
  float nl[3], pl[3];
  mtv(nl, R, n);
  const float dx[3] = {xp[0] - xg[0], xp[1] - xg[1], xp[2] - xg[2]};
  mtv(pl, R, dx);
  const float thr = fmaxf(0.f, depth - 1e-3f);
  const int v0 = m->geom_hulladr[g], v1 = v0 + m->geom_hullnum[g];
  const MPCR_GMEM float4* __restrict__ hv = m->hull_vert;
  auto sup = [&](const float4& v) { return (pl[0] - v.x) * nl[0] + (pl[1] - v.y) * nl[1] + (pl[2] - v.z) * nl[2]; };
  int ia = -1, il = -1;
  for (int base = v0; base < v1; base += WAVE) {
    const int i = base + lane;
    const unsigned long long bm = __ballot(i < v1 && sup(hv[i < v1 ? i : v0]) > thr);
    if (bm) {
      if (ia < 0) ia = base + __builtin_ctzll(bm);
      il = base + 63 - __builtin_clzll(bm);
    }
  }
  if (ia < 0) {  // the climb's vertex alone (threshold rounding): lane q keeps it
    if (lane == q) nsl = 1;
    return;
  }
  // max of e over the penetrating set, then its first index within the band
  auto pick = [&](auto&& ef, float& mx) {
    float lm = -1.f;
    for (int base = ia; base <= il; base += WAVE) {
      const int i = base + lane;
      if (i <= il) {
        const float4 v = hv[i];
        if (sup(v) > thr) lm = fmaxf(lm, ef(v));
      }
    }
    mx = wmax(lm);
    for (int base = ia; base <= il; base += WAVE) {
      const int i = base + lane;
      bool hit = false;
      if (i <= il) {
        const float4 v = hv[i];
        hit = sup(v) > thr && near_max(ef(v), mx);
      }
      const unsigned long long bm = __ballot(hit);
      if (bm) return base + __builtin_ctzll(bm);
    }
    return ia;  // unreachable: the maximum itself is within the band
  };
  const float4 a = hv[ia];
  float mx;
  const int ib = pick([&](const float4& v) {
    return (a.x - v.x) * (a.x - v.x) + (a.y - v.y) * (a.y - v.y) + (a.z - v.z) * (a.z - v.z);
  }, mx);
  const float4 b = hv[ib];
  float ab[3];
  {
    const float amb[3] = {a.x - b.x, a.y - b.y, a.z - b.z};
    cross(ab, nl, amb);
  }
  const int ic = pick([&](const float4& v) {
    return fabsf((a.x - v.x) * ab[0] + (a.y - v.y) * ab[1] + (a.z - v.z) * ab[2]);
  }, mx);
  const float4 c = hv[ic];
  float ac[3], bc[3];
  {
    const float amc[3] = {a.x - c.x, a.y - c.y, a.z - c.z}, bmc[3] = {b.x - c.x, b.y - c.y, b.z - c.z};
    cross(ac, nl, amc);
    cross(bc, nl, bmc);
  }
  float bbp, bap;
  const int ibp = pick([&](const float4& v) {
    return fabsf((b.x - v.x) * bc[0] + (b.y - v.y) * bc[1] + (b.z - v.z) * bc[2]);
  }, bbp);
  const int iap = pick([&](const float4& v) {
    return fabsf((a.x - v.x) * ac[0] + (a.y - v.y) * ac[1] + (a.z - v.z) * ac[2]);
  }, bap);
  const int idx[4] = {ia, ib, ic, beats(bap, bbp) ? iap : ibp};
#pragma unroll
  for (int k = 0; k < 4; k++) {
    bool dup = false;
#pragma unroll
    for (int t = 0; t < k; t++) dup |= idx[t] == idx[k];
    const float4 v = hv[idx[k]];
    const float l[3] = {v.x, v.y, v.z};
    float w[3];
    mv(w, R, l);
    const float d = -sup(v);
    if (lane == q) {
      dist[k] = dup ? 1e30f : d;
#pragma unroll
      for (int e = 0; e < 3; e++) { pos[k][e] = w[e] + xg[e] - 0.5f * d * n[e]; nrm[k][e] = n[e]; }
    }
  }
  if (lane == q) nsl = 4;
}

constexpr int kPendingManifold = -4;  // narrow_lane: plane-mesh pair awaiting plane_mesh_manifold_wave
constexpr float kPolyConeCos = 0.94f;  // ~20 degrees: candidate faces' Gauss-map cone about MPR's normal
static_assert(kPolyConeCos == (float)CONE_COS, "the host's cone table is built for this cone");
constexpr int kPendingPoly = -5;      // narrow_lane: polyhedron pair hit by MPR, awaiting poly_manifold_wave

// hull vertex index of geom g's support point along dir (world): the mesh
// climb from hint (the pair's, read only), or the box corner (+ side on an
// exactly zero component) -- the oracle's support_vertex
template <class S>
__device__ __forceinline__ int support_vertex(const DevModel* __restrict__ m, const S& s, int g, const float dir[3],
                                              int hint) {
  if (m->geom_type[g] == 6) {
    // the corner on the side of each axis; an axis within the tie band of
    // zero (a face normal from fp32 rounding) takes the + side, as MPR's box
    // support does (tie_sign)
    float l[3];
    mtv(l, s.gxmat[g], dir);
    const float ln = sqrtf(l[0] * l[0] + l[1] * l[1] + l[2] * l[2]);
    return m->geom_cornadr[g] + (tie_sign(l[0], ln) >= 0.f ? 1 : 0) + (tie_sign(l[1], ln) >= 0.f ? 2 : 0) +
           (tie_sign(l[2], ln) >= 0.f ? 4 : 0);
  }
  float p[3];
  support_geom(m, s, g, dir, p, hint);
  return hint;
}

// world outward normal of face f of geom g and its plane offset relative to
// c (nw . (x - c) = off on the face)
template <class S>
__device__ __forceinline__ void face_rel_fp(const S& s, int g, const float4 fp, const float* c, float nw[3],
                                            float& off) {
  const float nl[3] = {fp.x, fp.y, fp.z};
  mv(nw, s.gxmat[g], nl);
  off = fp.w + nw[0] * (s.gxpos[g][0] - c[0]) + nw[1] * (s.gxpos[g][1] - c[1]) + nw[2] * (s.gxpos[g][2] - c[2]);
}
template <class S>
__device__ __forceinline__ void face_rel(const DevModel* __restrict__ m, const S& s, int g, int f, const float* c,
                                         float nw[3], float& off) {
  const float4 fp = m->face_plane[f];
  const float nl[3] = {fp.x, fp.y, fp.z};
  mv(nw, s.gxmat[g], nl);
  off = fp.w + nw[0] * (s.gxpos[g][0] - c[0]) + nw[1] * (s.gxpos[g][1] - c[1]) + nw[2] * (s.gxpos[g][2] - c[2]);
}

// hull vertex v of geom g relative to c
template <class S>
__device__ __forceinline__ void vert_rel(const DevModel* __restrict__ m, const S& s, int g, int v, const float* c,
                                         float w[3]) {
  const float4 hv = m->hull_vert[v];
  const float l[3] = {hv.x, hv.y, hv.z};
  mv(w, s.gxmat[g], l);
  w[0] += s.gxpos[g][0] - c[0]; w[1] += s.gxpos[g][1] - c[1]; w[2] += s.gxpos[g][2] - c[2];
}

// Polyhedron pairs (mesh-mesh, box-mesh): the face-clipping manifold
// (mujoco-mjx 3.3.1 convex_convex; the oracle's poly_manifold, same rules and
// orders), wave-cooperative: every lane calls it with the same pair and MPR's
// normal n (g1 -> g2) / depth, lane q receives up to 4 contacts (nsl = 4) or
// keeps MPR's single one (nsl = 1: an edge axis carries the contact).  One
// lane per candidate reference face (the faces on both support vertices and
// those within the Gauss-map cone of MPR's normal) with its own support query
// for the SAT separation, one lane per candidate
// incident face, Sutherland-Hodgman against the reference face's side planes
// with one lane per polygon vertex and scan compaction (as box_box_wave), the
// _manifold_points picks as wave maxima.  Coordinates relative to g2's
// centre, as MPR's.
// PS: the clip polygon / SAT-separation scratch (polyw, satsep): the LDS
// image's own, or -- the second wave of a two-wave candidate in the joint
// convex flush -- a PolyScratchT in the dead dynamics region.
template <class S, class PS>
__device__ __forceinline__
void poly_manifold_wave(const DevModel* __restrict__ m_, const S& s, PS& ps, const short* hints, int p,
                                                const float n_[3], float depth, int q, int lane, float dist[4],
                                                float pos[4][3], float nrm[4][3], int& nsl) {
  const MPCR_GMEM DevModel* __restrict__ m = uniform_model(m_);
  ASSUME_GLOBAL(hints); ASSUME_LDS(&s); ASSUME_LDS(&ps); ASSUME_PRIVATE(dist); ASSUME_PRIVATE(pos); ASSUME_PRIVATE(nrm);
  ASSUME_PRIVATE(&nsl);
  const float n[3] = {n_[0], n_[1], n_[2]};  // in registers (no alias reloads)
  PSTAMP_DECL
  const int g1 = m->pair_g1[p], g2 = m->pair_g2[p];
  const float c[3] = {s.gxpos[g2][0], s.gxpos[g2][1], s.gxpos[g2][2]};
  const int hw = reinterpret_cast<const int*>(hints)[p - m->cvx_base];
  const int h0 = (int)(short)(hw & 0xffff), h1 = hw >> 16;
  // support vertices: lane 0 of g1 along n, lane 1 of g2 along -n
  int sv = 0;
  if (lane < 2) {
    const float sg = lane ? -1.f : 1.f;
    const float d[3] = {sg * n[0], sg * n[1], sg * n[2]};
    sv = support_vertex(m, s, lane ? g2 : g1, d, lane ? h1 : h0);
  }
  const int s1 = __shfl(sv, 0), s2 = __shfl(sv, 1);
  PSTAMP(m, 23);
  const int2 i1 = m->vert_finfo[s1], i2 = m->vert_finfo[s2];
  // a deep penetration between small hulls: every face is a candidate (MPR's
  // normal, which seeds the cone below, is that deep the portal face MPR
  // ended on -- fp32 and fp64 ended 70 degrees apart on the Hand-E's
  // interpenetrating finger pads)
  const int nf1 = m->geom_facenum[g1], nf2 = m->geom_facenum[g2];
  const bool allf = POLY_ALLF_ON && depth > POLY_DEEP && nf1 + nf2 <= POLY_ALLF;
  float bsep = 0.f;
  int fr = -1;
  bool rtwo = false, found = false;
  if (allf) {
    // SAT separation of every face (lane = face, rounds of 64) into LDS,
    // the wave max, then the lowest face index within the max's tie band
    // (MPCR_ALLF_U faces per lane per pass: their face-plane loads, then
    // their support queries' first loads, in flight together -- a pass was
    // two dependent load latencies per 64 faces, up to 8 passes in turn)
    const int fa1 = m->geom_faceadr[g1], fa2 = m->geom_faceadr[g2], nf = nf1 + nf2;
    constexpr int U = MPCR_ALLF_U;
    float mxl = -3e38f;  // this lane's maximum (the wave max below: max is exact in any order)
#pragma unroll 1
    for (int b0 = 0; b0 < nf; b0 += U * WAVE) {
      float4 fp[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int k = b0 + u * WAVE + lane;
        fp[u] = make_float4(0.f, 0.f, 1.f, 0.f);
        if (k < nf) fp[u] = m->face_plane[k >= nf1 ? fa2 + k - nf1 : fa1 + k];
      }
      SupQ q[U];
      float nw[U][3], off[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int k = b0 + u * WAVE + lane;
        if (k < nf) {
          const bool two = k >= nf1;
          const int g = two ? g2 : g1, go = two ? g1 : g2;
          face_rel_fp(s, g, fp[u], c, nw[u], off[u]);
          const float mn[3] = {-nw[u][0], -nw[u][1], -nw[u][2]};
          sup_start(m, s, go, mn, two ? h0 : h1, q[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int k = b0 + u * WAVE + lane;
        if (k < nf) {
          const bool two = k >= nf1;
          float pt[3];
          int h = two ? h0 : h1;
          sup_finish(m, s, two ? g1 : g2, q[u], pt, h, c, MPCR_SAT_TIES != 0);
          const float sp = nw[u][0] * pt[0] + nw[u][1] * pt[1] + nw[u][2] * pt[2] - off[u];
          ps.satsep[k] = sp;
          mxl = fmaxf(mxl, sp);
        }
      }
    }
    const float mxa = wmax(mxl);
    sync();
    // the key 2 f + side keeps the side with the face: two geoms of one mesh
    // share their face range, and on equal faces g1's wins, the
    // oracle's first-listed candidate
    float fmin = 3e38f;
#pragma unroll 1
    for (int b0 = 0; b0 < nf; b0 += WAVE) {
      const int k = b0 + lane;
      const bool nb = k < nf && near_max(ps.satsep[k], mxa);
      const int key = k >= nf1 ? 2 * (fa2 + k - nf1) + 1 : 2 * (fa1 + k);
      fmin = fminf(fmin, -wmax(nb ? -(float)key : -3e38f));
    }
    found = fmin < 3e38f;
    if (found) {
      const int key = (int)fmin;
      fr = key >> 1;
      rtwo = (key & 1) != 0;
      bsep = ps.satsep[rtwo ? nf1 + fr - fa2 : fr - fa1];
    }
    sync();  // satsep shares bytes with the clip buffer below
  }
  const int c1 = allf ? 0 : min(i1.y, WAVE), c2 = allf ? 0 : min(i2.y, WAVE - c1), ns = c1 + c2;
  // candidate reference faces, at most 64 (one per lane), in the oracle's
  // order: g1's on s1, g2's on s2, then every face whose outward normal lies
  // within the Gauss-map cone of n (g1) / -n (g2), face index order, those
  // already listed skipped -- a ballot-compacted scan of both face tables into
  // an LDS list (the clip buffer's second half, free until the clip)
  // The faces scanned are the host's cone table entries for the cube-map cell
  // of the local direction (DevModel::cone_cell: a superset of the faces the
  // test below accepts, ascending), not all of the geom's faces (up to 5219
  // on the dual arm's hulls): the same candidates in the same order.  The
  // support-vertex faces of each side sit one per lane (lane k: entry k) and
  // the duplicate test reads them with readlane.
  int* const cl = reinterpret_cast<int*>(&ps.polyw[1][0][0]);
  int nc = ns;
  const int vf1 = lane < c1 ? m->vert_face[i1.x + lane] : -1, vf2 = lane < c2 ? m->vert_face[i2.x + lane] : -1;
#pragma unroll 1
  for (int sd = 0; sd < 2 && !allf; sd++) {
    const int g = sd ? g2 : g1;
    const int cs = sd ? c2 : c1, vfs = sd ? vf2 : vf1;
    const float sg = sd ? -1.f : 1.f;
    float l[3];
    {
      const float dn[3] = {sg * n[0], sg * n[1], sg * n[2]};
      mtv(l, s.gxmat[g], dn);
    }
    const int2 cc = m->cone_cell[m->geom_coneadr[g] + lut_cell<CONE_R>(l)];
#pragma unroll 1
    for (int b0 = 0; b0 < cc.y && nc < WAVE; b0 += WAVE) {
      bool sel = false;
      int f = -1;
      if (b0 + lane < cc.y) {
        f = m->cone_face[cc.x + b0 + lane];
        const float4 fp = m->face_plane[f];
        const float nl[3] = {fp.x, fp.y, fp.z};
        float nw[3];
        mv(nw, s.gxmat[g], nl);
        sel = sg * (nw[0] * n[0] + nw[1] * n[1] + nw[2] * n[2]) >= kPolyConeCos;
      }
#pragma unroll 1
      for (int k = 0; k < cs; k++) sel &= __builtin_amdgcn_readlane(vfs, k) != f;
      int tot;
      const int o = wscan_excl(sel ? 1 : 0, tot);
      if (sel && nc + o < WAVE) cl[nc - ns + o] = f | (sd << 24);
      nc = min(nc + tot, WAVE);
    }
  }
  sync();
  PSTAMP(m, 24);
  // SAT separation along each candidate's outward normal
  float sep = -3e38f;
  int fid = -1, two = 0;
  if (!allf && lane < nc) {
    if (lane < ns) {
      two = lane >= c1;
      fid = m->vert_face[two ? i2.x + lane - c1 : i1.x + lane];
    } else {
      const int e = cl[lane - ns];
      two = e >> 24;
      fid = e & 0xffffff;
    }
    const int g = two ? g2 : g1, go = two ? g1 : g2;
    float nw[3], off, pt[3];
    face_rel(m, s, g, fid, c, nw, off);
    const float mn[3] = {-nw[0], -nw[1], -nw[2]};
    int h = two ? h0 : h1;
    support_geom(m, s, go, mn, pt, h, c, MPCR_SAT_TIES != 0);
    sep = nw[0] * pt[0] + nw[1] * pt[1] + nw[2] * pt[2] - off;
  }
  // the maximum's tie band: the lowest face index (a flush face pair has the
  // same separation from either side)
  if (!allf) {
    const float mx = wmax(sep);
    const bool nb = lane < nc && near_max(sep, mx);
    const float fmn = -wmax(nb ? -(float)fid : -3e38f);
    const unsigned long long bm = __ballot(nb && (float)fid == fmn);
    const int kb = bm ? __builtin_ctzll(bm) : 0;
    found = bm != 0;
    bsep = __shfl(sep, kb);
    fr = __shfl(fid, kb);
    rtwo = __shfl(two, kb) != 0;
  }
  PSTAMP(m, 25);
  if (!found || -bsep > 1.05f * depth + 1e-5f) {  // an edge axis: MPR's single contact
    if (lane == q) nsl = 1;
    return;
  }
  const int gr = rtwo ? g2 : g1, gi = rtwo ? g1 : g2;
  float nr[3], offr;
  face_rel(m, s, gr, fr, c, nr, offr);
  // the reference polygon's vertices (lane k: vertex k), loaded here so their
  // latency hides behind the incident face's support climb
  const int2 fri = m->face_vinfo[fr];
  const int nrv = fri.y;
  float A[3] = {0.f, 0.f, 0.f}, sn[3];
  if (lane < nrv) vert_rel(m, s, gr, m->face_vert[fri.x + lane], c, A);
  // incident face: the most anti-parallel face on gi's support vertex along -nr
  int si = 0;
  if (lane == 0) {
    const float d[3] = {-nr[0], -nr[1], -nr[2]};
    si = support_vertex(m, s, gi, d, rtwo ? h0 : h1);
  }
  si = __shfl(si, 0);
  const int2 ii = m->vert_finfo[si];
  const int ci = min(ii.y, WAVE);
  float al = -3e38f;
  int finc = -1;
  if (lane < ci) {
    finc = m->vert_face[ii.x + lane];
    const float4 fp = m->face_plane[finc];
    const float nl[3] = {fp.x, fp.y, fp.z};
    float nw[3];
    mv(nw, s.gxmat[gi], nl);
    al = -(nw[0] * nr[0] + nw[1] * nr[1] + nw[2] * nr[2]);
  }
  const float mxa = wmax(al);
  const unsigned long long bma = __ballot(lane < ci && near_max(al, mxa));
  if (!bma) {
    if (lane == q) nsl = 1;
    return;
  }
  const int fi = __shfl(finc, __builtin_ctzll(bma));
  // reference polygon (lane k: vertex k and its edge's outward side-plane
  // normal), incident polygon into the clip buffer
  const int2 fii = m->face_vinfo[fi];
  const int ninc = fii.y;
  {
    const int ln = lane + 1 >= nrv ? 0 : lane + 1;
    const float ed[3] = {__shfl(A[0], ln) - A[0], __shfl(A[1], ln) - A[1], __shfl(A[2], ln) - A[2]};
    cross(sn, ed, nr);
  }
  if (lane < ninc) {
    float w[3];
    vert_rel(m, s, gi, m->face_vert[fii.x + lane], c, w);
    ps.polyw[0][lane][0] = w[0]; ps.polyw[0][lane][1] = w[1]; ps.polyw[0][lane][2] = w[2];
  }
  sync();
  PSTAMP(m, 26);
  int np = ninc, cur = 0;
  for (int e = 0; e < nrv && np > 0; e++) {
    const float Ae[3] = {__shfl(A[0], e), __shfl(A[1], e), __shfl(A[2], e)};
    const float se[3] = {__shfl(sn[0], e), __shfl(sn[1], e), __shfl(sn[2], e)};
    float P[3] = {0.f, 0.f, 0.f}, Q[3] = {0.f, 0.f, 0.f}, dp = 0.f, dq = 0.f;
    int e0 = 0, e1 = 0;
    if (lane < np) {
      const int k2 = lane + 1 == np ? 0 : lane + 1;
#pragma unroll
      for (int k = 0; k < 3; k++) { P[k] = ps.polyw[cur][lane][k]; Q[k] = ps.polyw[cur][k2][k]; }
      dp = se[0] * (P[0] - Ae[0]) + se[1] * (P[1] - Ae[1]) + se[2] * (P[2] - Ae[2]);
      dq = se[0] * (Q[0] - Ae[0]) + se[1] * (Q[1] - Ae[1]) + se[2] * (Q[2] - Ae[2]);
      e0 = dp <= 0.f;
      e1 = (dp < 0.f && dq > 0.f) || (dp > 0.f && dq < 0.f);
    }
    int tot;
    const int o = wscan_excl(e0 + e1, tot);
    if (e0 && o < S::PMAXW) {
#pragma unroll
      for (int k = 0; k < 3; k++) ps.polyw[cur ^ 1][o][k] = P[k];
    }
    if (e1 && o + e0 < S::PMAXW) {
      const float wgt = dp / (dp - dq);
#pragma unroll
      for (int k = 0; k < 3; k++) ps.polyw[cur ^ 1][o + e0][k] = P[k] + wgt * (Q[k] - P[k]);
    }
    np = min(tot, S::PMAXW);
    cur ^= 1;
    sync();
  }
  // the clipped points below the reference plane
  float P[3] = {0.f, 0.f, 0.f}, dk = 3e38f;
  bool keep = false;
  if (lane < np) {
#pragma unroll
    for (int k = 0; k < 3; k++) P[k] = ps.polyw[cur][lane][k];
    dk = nr[0] * P[0] + nr[1] * P[1] + nr[2] * P[2] - offr;
    keep = dk < m->pair_margin[p];
  }
  const unsigned long long km = __ballot(keep);
  const int nk = __popcll(km);
  sync();  // the clip buffer is free for the next pair
  PSTAMP(m, 27);
  const float sg = rtwo ? -1.f : 1.f;  // contact normal g1 -> g2
  if (nk == 0) {
    // no clipped point below the reference plane (a small reference face
    // over a deep penetration): the SAT axis still carries the contact, one
    // point at gi's support vertex along -nr (the oracle's rule; MPR's own
    // normal for a penetration this deep is path-dependent)
    float w[3];
    vert_rel(m, s, gi, si, c, w);
    const float dk = nr[0] * w[0] + nr[1] * w[1] + nr[2] * w[2] - offr;
    if (lane == q) {
      if (dk < m->pair_margin[p]) {
        dist[0] = dk;
        dist[1] = dist[2] = dist[3] = 1e30f;
#pragma unroll
        for (int e = 0; e < 3; e++) { pos[0][e] = w[e] - 0.5f * dk * nr[e] + c[e]; nrm[0][e] = sg * nr[e]; }
        nsl = 4;
      } else {
        nsl = 1;
      }
    }
    return;
  }
  int idx[4] = {-1, -1, -1, -1};
  if (nk <= 4) {
    unsigned long long r = km;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (r) { idx[j] = __builtin_ctzll(r); r &= r - 1; }
    }
  } else {
    // _manifold_points: a = the first, b = the farthest from a, c = the
    // farthest from line ab, d = the farthest from edge bc or ac
    auto pick = [&](float e, float& mxv) {
      mxv = wmax(keep ? e : -1.f);
      return __builtin_ctzll(__ballot(keep && near_max(e, mxv)));
    };
    const int ia = __builtin_ctzll(km);
    const float a[3] = {__shfl(P[0], ia), __shfl(P[1], ia), __shfl(P[2], ia)};
    float mxv;
    const int ib = pick((a[0] - P[0]) * (a[0] - P[0]) + (a[1] - P[1]) * (a[1] - P[1]) + (a[2] - P[2]) * (a[2] - P[2]),
                        mxv);
    const float b[3] = {__shfl(P[0], ib), __shfl(P[1], ib), __shfl(P[2], ib)};
    float ab[3];
    {
      const float amb[3] = {a[0] - b[0], a[1] - b[1], a[2] - b[2]};
      cross(ab, nr, amb);
    }
    const int ic = pick(fabsf((a[0] - P[0]) * ab[0] + (a[1] - P[1]) * ab[1] + (a[2] - P[2]) * ab[2]), mxv);
    const float cc[3] = {__shfl(P[0], ic), __shfl(P[1], ic), __shfl(P[2], ic)};
    float ac[3], bc[3];
    {
      const float amc[3] = {a[0] - cc[0], a[1] - cc[1], a[2] - cc[2]}, bmc[3] = {b[0] - cc[0], b[1] - cc[1], b[2] - cc[2]};
      cross(ac, nr, amc);
      cross(bc, nr, bmc);
    }
    float bbp, bap;
    const int ibp = pick(fabsf((b[0] - P[0]) * bc[0] + (b[1] - P[1]) * bc[1] + (b[2] - P[2]) * bc[2]), bbp);
    const int iap = pick(fabsf((a[0] - P[0]) * ac[0] + (a[1] - P[1]) * ac[1] + (a[2] - P[2]) * ac[2]), bap);
    idx[0] = ia; idx[1] = ib; idx[2] = ic; idx[3] = beats(bap, bbp) ? iap : ibp;
  }
#pragma unroll
  for (int j = 0; j < 4; j++) {
    bool dup = idx[j] < 0;
#pragma unroll
    for (int t = 0; t < j; t++) dup |= idx[t] == idx[j];
    const int L = idx[j] < 0 ? 0 : idx[j];
    const float Pj[3] = {__shfl(P[0], L), __shfl(P[1], L), __shfl(P[2], L)};
    const float dj = __shfl(dk, L);
    if (lane == q) {
      dist[j] = dup ? 1e30f : dj;
#pragma unroll
      for (int e = 0; e < 3; e++) { pos[j][e] = Pj[e] - 0.5f * dj * nr[e] + c[e]; nrm[j][e] = sg * nr[e]; }
    }
  }
  if (lane == q) nsl = 4;
  PSTAMP(m, 28);
}

}  // namespace mpcr
