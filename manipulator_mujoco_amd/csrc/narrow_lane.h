// narrow_lane.h -- the per-lane narrow phase of the rollout kernel, contact frame and
// impedance.
#pragma once
#include "rollout_switches.h"
#include "narrow_prims.h"
#include "manifold.h"

namespace mpcr {

// per-lane narrow phase for plane/capsule/box-vs-capsule pairs (box-box is
// wave-cooperative, below).  out: dist[4], pos[4][3], nrm[4][3]
// Single-arm kernels: dist[] on every lane -- cost_c reads the distances --
// and a capsule-box point's pos / nrm on demand: only where the point will be
// emitted as a contact (its distance under the margin, contacts enabled); on
// most steps no lane of the wave has one and the block is skipped.  With
// DEV_NARROW_EAGER in the device model's flags (MPCR_NARROW_EAGER=1, tests)
// every lane computes them.  rq: quads 0-1 of the pair's set-up record as the
// chunk loop fetched them.
template <class S>
__device__ __forceinline__ int narrow_lane(const DevModel* __restrict__ m, const S& s, short* hints, int p, float dist[4],
                            float pos[4][3], float nrm[4][3], float* dbg = nullptr,
                            [[maybe_unused]] const float4* rq = nullptr) {
  // single-arm kernels: function and geoms from the chunk loop's quads, both
  // sizes from the record's other two (the model's arrays: pair -> geoms ->
  // sizes; held from the chunk loop on they cost the one-wave kernel 6 VGPRs)
  [[maybe_unused]] float4 q0 = {0.f, 0.f, 0.f, 0.f};
  [[maybe_unused]] float sz1[3], sz2[3];
  if constexpr (kStepLoad<S>) {
    const StepPairSetup& ps = step_records(m)->pair[p];
    q0 = rq[0];
    const float4 q2 = recq(ps, 2), q3 = recq(ps, 3);
    sz1[0] = q2.x; sz1[1] = q2.y; sz1[2] = q2.z;
    sz2[0] = q3.x; sz2[1] = q3.y; sz2[2] = q3.z;
  }
  const int g1 = kStepLoad<S> ? __float_as_int(q0.z) : m->pair_g1[p], g2 = kStepLoad<S> ? __float_as_int(q0.w) : m->pair_g2[p];
  const int func = kStepLoad<S> ? __float_as_int(q0.x) : m->pair_func[p];
  const float* x1 = s.gxpos[g1];
  const float* x2 = s.gxpos[g2];
  const float* R1 = s.gxmat[g1];
  const float* R2 = s.gxmat[g2];
  const float* s1 = kStepLoad<S> ? sz1 : m->geom_size[g1];
  const float* s2 = kStepLoad<S> ? sz2 : m->geom_size[g2];
#pragma unroll
  for (int k = 0; k < 4; k++) dist[k] = 1e30f;
  if (func == 0) {  // plane - capsule
    float n[3] = {R1[2], R1[5], R1[8]}, ax[3] = {R2[2], R2[5], R2[8]};
    float r = s2[0], hl = s2[1];
#pragma unroll
    for (int k = 0; k < 2; k++) {
      float sg = k == 0 ? 1.f : -1.f, e[3], dif[3];
#pragma unroll
      for (int c = 0; c < 3; c++) { e[c] = x2[c] + sg * hl * ax[c]; dif[c] = e[c] - x1[c]; }
      float d = dot3(n, dif) - r;
      dist[k] = d;
#pragma unroll
      for (int c = 0; c < 3; c++) { pos[k][c] = e[c] - n[c] * (r + 0.5f * d); nrm[k][c] = n[c]; }
    }
    return 2;
  }
  if (func == 1) {  // plane - box: the 4 deepest corners, ascending depth (ties: corner index)
    // depth(c) = n.(x2 - x1) + sum_k +-w_k with w_k = h_k n.R2_k: the deepest
    // corner takes the sign against each w_k, the next ones flip the axis of
    // the smallest |w|, of the second smallest, and then the third axis or
    // both of the first two -- 5 candidates instead of a 4 x 8 scan
    const float n[3] = {R1[2], R1[5], R1[8]};
    float w[3];
#pragma unroll
    for (int k = 0; k < 3; k++) w[k] = s2[k] * (n[0] * R2[k] + n[1] * R2[3 + k] + n[2] * R2[6 + k]);
    const int c0 = (w[0] < 0.f ? 1 : 0) | (w[1] < 0.f ? 2 : 0) | (w[2] < 0.f ? 4 : 0);
    int ax0 = 0, ax1 = 1, ax2 = 2;  // axes by |w| ascending, index order on ties
    if (fabsf(w[ax1]) < fabsf(w[ax0])) { const int t = ax0; ax0 = ax1; ax1 = t; }
    if (fabsf(w[ax2]) < fabsf(w[ax1])) { const int t = ax1; ax1 = ax2; ax2 = t; }
    if (fabsf(w[ax1]) < fabsf(w[ax0])) { const int t = ax0; ax0 = ax1; ax1 = t; }
    auto depth = [&](int c) {  // the same expression as the oracle's corner distance
      const float l[3] = {(c & 1) ? s2[0] : -s2[0], (c & 2) ? s2[1] : -s2[1], (c & 4) ? s2[2] : -s2[2]};
      float v[3];
      mv(v, R2, l);
      return n[0] * (x2[0] + v[0] - x1[0]) + n[1] * (x2[1] + v[1] - x1[1]) + n[2] * (x2[2] + v[2] - x1[2]);
    };
    int cs[4] = {c0, c0 ^ (1 << ax0), c0 ^ (1 << ax1), c0 ^ (1 << ax2)};
    float ds[4] = {depth(cs[0]), depth(cs[1]), depth(cs[2]), depth(cs[3])};
    {
      const int c4 = c0 ^ (1 << ax0) ^ (1 << ax1);
      const float d4 = depth(c4);
      if (d4 < ds[3] || (d4 == ds[3] && c4 < cs[3])) { cs[3] = c4; ds[3] = d4; }
    }
    // order the four by (depth, index): sorting network (0,1) (2,3) (0,2) (1,3) (1,2)
    auto cx = [&](int i, int j) {
      if (ds[j] < ds[i] || (ds[j] == ds[i] && cs[j] < cs[i])) {
        const float td = ds[i]; ds[i] = ds[j]; ds[j] = td;
        const int tc = cs[i]; cs[i] = cs[j]; cs[j] = tc;
      }
    };
    cx(0, 1); cx(2, 3); cx(0, 2); cx(1, 3); cx(1, 2);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int c = cs[k];
      const float l[3] = {(c & 1) ? s2[0] : -s2[0], (c & 2) ? s2[1] : -s2[1], (c & 4) ? s2[2] : -s2[2]};
      float v[3];
      mv(v, R2, l);
      dist[k] = ds[k];
#pragma unroll
      for (int e = 0; e < 3; e++) { pos[k][e] = x2[e] + v[e] - n[e] * 0.5f * ds[k]; nrm[k][e] = n[e]; }
    }
    return 4;
  }
  if (func == 2) {  // capsule - capsule
    float a1[3] = {R1[2], R1[5], R1[8]}, a2[3] = {R2[2], R2[5], R2[8]};
    float p1[3], d1[3], p2[3], d2[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      p1[c] = x1[c] - s1[1] * a1[c]; d1[c] = 2 * s1[1] * a1[c];
      p2[c] = x2[c] - s2[1] * a2[c]; d2[c] = 2 * s2[1] * a2[c];
    }
    float sc, tc, n[3], c1[3];
    seg_seg(p1, d1, p2, d2, &sc, &tc);
#pragma unroll
    for (int c = 0; c < 3; c++) { c1[c] = p1[c] + sc * d1[c]; n[c] = p2[c] + tc * d2[c] - c1[c]; }
    float len = sqrtf(dot3(n, n));
    if (len < 1e-12f) {
      float t[3] = {1, 0, 0};
      if (fabsf(a1[0]) > 0.9f) { t[0] = 0; t[1] = 1; }
      cross(n, a1, t);
      float l = sqrtf(dot3(n, n));
      n[0] /= l; n[1] /= l; n[2] /= l;
    } else {
      n[0] /= len; n[1] /= len; n[2] /= len;
    }
    float d = len - s1[0] - s2[0];
    dist[0] = d;
#pragma unroll
    for (int c = 0; c < 3; c++) { pos[0][c] = c1[c] + n[c] * (s1[0] + 0.5f * d); nrm[0][c] = n[c]; }
    return 1;
  }
  if (func == 3) {  // capsule - box
    float ax[3] = {R1[2], R1[5], R1[8]}, r = s1[0], hl = s1[1];
    const float* h = s2;
    float A[3], B[3], a[3], dd[3];
#pragma unroll
    for (int c = 0; c < 3; c++) { A[c] = x1[c] - hl * ax[c] - x2[c]; B[c] = 2 * hl * ax[c]; }
    mtv(a, R2, A);
    mtv(dd, R2, B);
    float tlo = -1.f, thi = 2.f, flo = 0.f, fhi = 0.f;
    // knots: 0, 1, (+-h_k - a_k)/dd_k inside (0,1), where the squared
    // distance's derivative fp (piecewise linear, non-decreasing: the
    // distance is convex along the segment) is evaluated.  The interior knots
    // only matter when fp changes sign inside (fp(0) < 0 <= fp(1)); when no
    // lane's does, the minimum is an end on every lane (ts 0 or 1 below, as
    // the full scan gives) and the six interior knots are skipped (C3: most
    // steps of the 20 robot capsule / box pairs, MPCR_CB_SKIP)
    auto knot = [&](int i) {
      float t;
      bool ok = true;
      if (i == 0) t = 0.f;
      else if (i == 1) t = 1.f;
      else {
        int k = (i - 2) >> 1;
        float sg = ((i - 2) & 1) ? 1.f : -1.f;
        ok = fabsf(dd[k]) > kMinVal;
        t = ok ? (sg * h[k] - a[k]) / dd[k] : 0.f;
        ok = ok && t > 0.f && t < 1.f;
      }
      if (ok) {
        // x - clamp(x, -h, h) is +-(|x| - h) outside the slab, 0 inside --
        // the same value as the sign-selected excess, one v_med3 instead
        // of the compares and selects
        float fp = 0.f;
#pragma unroll
        for (int k = 0; k < 3; k++) {
          const float x = a[k] + t * dd[k];
          fp += 2.f * dd[k] * (x - __builtin_amdgcn_fmed3f(x, -h[k], h[k]));
        }
        if (fp < 0) { if (t > tlo) { tlo = t; flo = fp; } }
        else { if (t < thi) { thi = t; fhi = fp; } }
      }
    };
    knot(0);
    knot(1);
    if (!MPCR_CB_SKIP || __ballot(tlo == 0.f && thi == 1.f) != 0ull) {
#pragma unroll
      for (int i = 2; i < 8; i++) knot(i);
    }
    float ts;
    if (tlo < 0) ts = 0.f;
    else if (thi > 1) ts = 1.f;
    else ts = fhi - flo > 0 ? tlo - flo * (thi - tlo) / (fhi - flo) : tlo;
    float pp[3], q[3], nl[3];
#pragma unroll
    for (int c = 0; c < 3; c++) pp[c] = a[c] + ts * dd[c];
    float g = point_box(pp, h, nl, q);
    if (g <= 1e-6f) {  // on or in the box (penetrating segments land on the surface): the oracle's band
      // deepest point of g(t) = max_k |x_k(t)| - h_k over its kinks
      float gbest = 1e30f, tbest = 0.f;
#pragma unroll
      for (int i = 0; i < 17; i++) {
        float t;
        bool ok = true;
        if (i == 0) t = 0.f;
        else if (i == 1) t = 1.f;
        else if (i < 5) {
          int k = i - 2;
          ok = fabsf(dd[k]) > kMinVal;
          t = ok ? -a[k] / dd[k] : 0.f;
          ok = ok && t > 0.f && t < 1.f;
        } else {
          int q4 = i - 5;        // 0..11: pair (ii,jj) x signs
          int pr = q4 >> 2;      // 0:(0,1) 1:(0,2) 2:(1,2)
          int ii = pr == 2 ? 1 : 0, jj = pr == 0 ? 1 : 2;
          float si = (q4 & 2) ? 1.f : -1.f, sj = (q4 & 1) ? 1.f : -1.f;
          float den = si * dd[ii] - sj * dd[jj];
          ok = fabsf(den) > kMinVal;
          t = ok ? (h[ii] - h[jj] - si * a[ii] + sj * a[jj]) / den : 0.f;
          ok = ok && t > 0.f && t < 1.f;
        }
        if (ok) {
          float gm = -1e30f;
#pragma unroll
          for (int k = 0; k < 3; k++) gm = fmaxf(gm, fabsf(a[k] + t * dd[k]) - h[k]);
          // a flat minimum (the segment parallel to a face: every kink as
          // deep) keeps the first candidate -- a later one must be deeper by
          // more than 1 um, so fp32 and fp64 pick the same point (the oracle's rule)
          if (gm < gbest - 1e-6f) { gbest = gm; tbest = t; }
        }
      }
      ts = tbest;
#pragma unroll
      for (int c = 0; c < 3; c++) pp[c] = a[c] + ts * dd[c];
      g = point_box(pp, h, nl, q);
    }
    // which points get their pos / nrm (single-arm kernels; uniform parts first)
    [[maybe_unused]] bool want_all = true, want_any = true;
    [[maybe_unused]] float mg = 0.f;
    if constexpr (!S::WIDE) {
      want_all = (m->disableflags & DEV_NARROW_EAGER) != 0;
      want_any = !(m->disableflags & 16);
      mg = kStepLoad<S> ? rq[1].w : m->pair_margin[p];
    }
    // the far end: on or in the box, the first point's face, the segment
    // clipped to the face's extent (the oracle's col_capsule_box, round 4);
    // outside, its own point_box
    int fk = -1;
    float fsg = 0.f;
    if (g <= 0.f) {
#pragma unroll
      for (int c = 0; c < 3; c++)
        if (nl[c] != 0.f) { fk = c; fsg = -nl[c]; }
    }
#pragma unroll
    for (int k = 0; k < 2; k++) {
      if (k == 1) {
        float t = ts < 0.5f ? 1.f : 0.f;
        if (fk >= 0) {
#pragma unroll
          for (int j = 0; j < 3; j++) {
            if (j == fk || !(fabsf(dd[j]) > kMinVal)) continue;
            const float x = a[j] + t * dd[j];
            if (fabsf(x) > h[j]) {
              const float tb = ((x > 0.f ? h[j] : -h[j]) - a[j]) / dd[j];
              t = ts < t ? fminf(t, fmaxf(tb, ts)) : fmaxf(t, fminf(tb, ts));
            }
          }
          float gf = 0.f;
#pragma unroll
          for (int c = 0; c < 3; c++) {
            pp[c] = a[c] + t * dd[c];
            nl[c] = c == fk ? -fsg : 0.f;
            q[c] = c == fk ? fsg * h[c] : pp[c];
            gf = c == fk ? fsg * pp[c] - h[c] : gf;
          }
          g = gf;
        } else {
#pragma unroll
          for (int c = 0; c < 3; c++) pp[c] = a[c] + t * dd[c];
          g = point_box(pp, h, nl, q);
        }
      }
      if constexpr (S::WIDE) {
        float n[3], pl[3], tmp[3];
        mv(n, R2, nl);
#pragma unroll
        for (int c = 0; c < 3; c++) pl[c] = 0.5f * (pp[c] + r * nl[c] + q[c]);
        mv(tmp, R2, pl);
        dist[k] = g - r;
#pragma unroll
        for (int c = 0; c < 3; c++) { pos[k][c] = tmp[c] + x2[c]; nrm[k][c] = n[c]; }
      } else {
        dist[k] = g - r;
        if (want_all || (want_any && dist[k] < mg)) {
          float n[3], pl[3], tmp[3];
          mv(n, R2, nl);
#pragma unroll
          for (int c = 0; c < 3; c++) pl[c] = 0.5f * (pp[c] + r * nl[c] + q[c]);
          mv(tmp, R2, pl);
#pragma unroll
          for (int c = 0; c < 3; c++) { pos[k][c] = tmp[c] + x2[c]; nrm[k][c] = n[c]; }
        }
      }
    }
    return 2;
  }
  if constexpr (S::WIDE) {
    // hull hill climbs start where this pair's previous step ended (the
    // oracle keeps the same per-pair cache)
    int* hp = reinterpret_cast<int*>(hints) + (p - m->cvx_base);  // (side 0, side 1) as two shorts
    const int hv = *hp;
    int hint[2] = {(int)(short)(hv & 0xffff), hv >> 16};
    if (func == 9) {  // general convex (MPR)
      float depth, n[3], pp[3];
      float* tr = (dbg && (int)dbg[DBG_MPR] == p) ? dbg + DBG_MPR : nullptr;
      const bool hit = mpr_lane(m, s, g1, g2, depth, n, pp, hint, tr);
      if (tr) {
        tr[1] = hit ? 1.f : 0.f; tr[2] = depth;
        tr[3] = n[0]; tr[4] = n[1]; tr[5] = n[2]; tr[6] = pp[0]; tr[7] = pp[1]; tr[8] = pp[2];
      }
      *hp = (hint[0] & 0xffff) | (hint[1] << 16);
      if (hit) {
        if (n[0] == 0.f && n[1] == 0.f && n[2] == 0.f) n[2] = 1.f;
        dist[0] = -depth;
#pragma unroll
        for (int c = 0; c < 3; c++) { pos[0][c] = pp[c]; nrm[0][c] = n[c]; }
        // a penetrating polyhedron pair: the caller runs the face-clipping manifold
        if (m->pair_ncon[p] == 4 && depth > 0.f) return kPendingPoly;
      }
      return 1;
    }
    if (func == 10 && m->pair_ncon[p] == 4 && m->geom_type[g2] == 5) {
      // plane - cylinder: MuJoCo's mjc_PlaneCylinder (the oracle's
      // col_plane_cylinder): deepest rim point, the far cap's on that side,
      // two near-cap rim points 120 degrees either side of the first
      const float n[3] = {R1[2], R1[5], R1[8]};
      float ax[3] = {R2[2], R2[5], R2[8]}, vec[3];
      float prjaxis = dot3(n, ax);
      if (prjaxis > 0.f) { ax[0] = -ax[0]; ax[1] = -ax[1]; ax[2] = -ax[2]; prjaxis = -prjaxis; }
      const float dist0 = n[0] * (x2[0] - x1[0]) + n[1] * (x2[1] - x1[1]) + n[2] * (x2[2] - x1[2]);
#pragma unroll
      for (int c = 0; c < 3; c++) vec[c] = ax[c] * prjaxis - n[c];
      const float len = sqrtf(dot3(vec, vec));
      if (len < kMinVal) { vec[0] = R2[0]; vec[1] = R2[3]; vec[2] = R2[6]; }
      else { const float il = 1.f / len; vec[0] *= il; vec[1] *= il; vec[2] *= il; }
#pragma unroll
      for (int c = 0; c < 3; c++) { vec[c] *= s2[0]; ax[c] *= s2[1]; }
      const float prjvec = dot3(vec, n);
      prjaxis *= s2[1];
      const float margin = m->pair_margin[p];
      float d = dist0 + prjaxis + prjvec;
      dist[0] = d;
#pragma unroll
      for (int c = 0; c < 3; c++) { pos[0][c] = x2[c] + vec[c] + ax[c] - 0.5f * d * n[c]; nrm[0][c] = n[c]; }
      if (d <= margin) {
        d = dist0 - prjaxis + prjvec;
        if (d <= margin) {
          dist[1] = d;
#pragma unroll
          for (int c = 0; c < 3; c++) { pos[1][c] = x2[c] + vec[c] - ax[c] - 0.5f * d * n[c]; nrm[1][c] = n[c]; }
        }
        d = dist0 + prjaxis - 0.5f * prjvec;
        if (d <= margin) {
          float v1[3];
          cross(v1, vec, ax);
          const float l1 = sqrtf(dot3(v1, v1));
          const float sc = l1 > 0.f ? s2[0] * 0.8660254037844386f / l1 : 0.f;
#pragma unroll
          for (int k = 0; k < 2; k++) {
            const float sv = k ? -sc : sc;
            dist[2 + k] = d;
#pragma unroll
            for (int c = 0; c < 3; c++) {
              pos[2 + k][c] = x2[c] + sv * v1[c] + ax[c] - 0.5f * vec[c] - 0.5f * d * n[c];
              nrm[2 + k][c] = n[c];
            }
          }
        }
      }
      return 4;
    }
    if (func == 10) {  // plane - convex: deepest support point
      float n[3] = {R1[2], R1[5], R1[8]}, nn[3] = {-R1[2], -R1[5], -R1[8]}, q[3];
      support_geom(m, s, g2, nn, q, hint[1]);
      *hp = (hint[0] & 0xffff) | (hint[1] << 16);
      const float d = n[0] * (q[0] - x1[0]) + n[1] * (q[1] - x1[1]) + n[2] * (q[2] - x1[2]);
      dist[0] = d;
#pragma unroll
      for (int c = 0; c < 3; c++) { pos[0][c] = q[c] - 0.5f * d * n[c]; nrm[0][c] = n[c]; }
      // a penetrating mesh: the caller runs the wave-cooperative manifold
      return (d < 0.f && m->geom_type[g2] == 7) ? kPendingManifold : 1;
    }
  }
  return 0;
}

__device__ __forceinline__ void make_frame(float f[9], const float n[3]) {
  f[0] = n[0]; f[1] = n[1]; f[2] = n[2];
  float y[3] = {0.f, 1.f, 0.f};
  if (fabsf(n[1]) >= 0.5f) { y[1] = 0.f; y[2] = 1.f; }
  float dd = dot3(n, y);
  y[0] -= dd * n[0]; y[1] -= dd * n[1]; y[2] -= dd * n[2];
  float ny = sqrtf(dot3(y, y));
  f[3] = y[0] / ny; f[4] = y[1] / ny; f[5] = y[2] / ny;
  cross(f + 6, f, f + 3);
}

__device__ __forceinline__ float impedance(const float* si, float pos, float margin) {
  float dmin = clampf(si[0], kMinImp, kMaxImp), dmax = clampf(si[1], kMinImp, kMaxImp);
  float width = si[2], mid = si[3], power = si[4];
  if (dmin == dmax || width <= kMinVal) return 0.5f * (dmin + dmax);
  float x = fabsf((pos - margin) / width);
  if (x >= 1.f) return dmax;
  if (x <= 0.f) return dmin;
  float y;
  if (power == 1.f) y = x;
  else if (power == 2.f) y = x <= mid ? x * x / mid : 1.f - (1.f - x) * (1.f - x) / (1.f - mid);  // default solimp
  else if (x <= mid) y = powf(x, power) / powf(mid, power - 1.f);
  else y = 1.f - powf(1.f - x, power) / powf(1.f - mid, power - 1.f);
  return dmin + y * (dmax - dmin);
}

}  // namespace mpcr
