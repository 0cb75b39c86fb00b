// linesearch.h -- Newton's line-search point and the elliptic friction cone of the
// rollout kernel.
#pragma once
#include "rollout.h"
#include "wave.h"
#include "vecmath.h"

namespace mpcr {

// ---------------------------------------------------------------------------
// line search point (MJX-style, see oracle)

// cost: complete, or (narrow kernel, full == false) without its constant
// part q0 (the active rows' 0.5 D jar^2 + the Gauss term), which the bracket
// never reads: the line search adds it once for the final two points.
// T: the precision of a point's step size, cost and derivatives and of the
// bracket arithmetic -- fp64 in the dual-arm class (LsReal): the point's cost
// alpha^2 q2 + alpha q1 + q0 cancels a ~1e4 constant to compare candidates
// that differ in the last fp32 bits, and the bracket's Newton steps
// alpha - d0 / d1 divide two such differences; in fp32 those decisions
// halved the dual arm's parity (78 -> 37 well-conditioned
// misses of the fp32 restatement against fp64).  The row sums stay fp32.
template <class T>
struct LsPtT { T alpha, cost, d0, d1; bool full; };
template <class S>
using LsReal = typename std::conditional<S::WIDE, double, float>::type;

// elliptic rows: efc_src = (5 << 24) | (contact << 14) | (pair << 4) | side
__device__ __forceinline__ bool ell_row(int src) { return (src >> 24) == 5; }
__device__ __forceinline__ bool ell_head(int src) { return (src >> 24) == 5 && (src & 15) == 0; }
__device__ __forceinline__ int ell_pair(int src) { return (src >> 4) & 1023; }


// the row's side of its kink at the step size alpha (in alpha's precision)
template <class T>
__device__ __forceinline__ bool ls_neg(float jar, float jv, T alpha) {
  return (T)jar + alpha * (T)jv < (T)0;
}

template <class S, class T>
__device__ __forceinline__ void ls_rows(const S& s, int lane, T alpha, float& q0, float& q1, float& q2) {
  q0 = q1 = q2 = 0.f;
  for (int r = lane; r < s.nefc; r += WAVE) {
    float jar = s.efc_jar[r], jv = s.efc_jv[r];
    if constexpr (S::WIDE) {
      if (ell_row(s.efc_src[r])) continue;
    }
    if (((s.efc_src[r] >> 24) == 1) || ls_neg(jar, jv, alpha)) {
      float D = s.efc_D[r];
      q0 += 0.5f * D * jar * jar;
      q1 += D * jv * jar;
      q2 += 0.5f * D * jv * jv;
    }
  }
}

template <class T>
__device__ __forceinline__ LsPtT<T> ls_make(T alpha, T q0, T q1, T q2) {
  LsPtT<T> p;
  p.alpha = alpha;
  p.cost = alpha * alpha * q2 + alpha * q1 + q0;
  p.d0 = (T)2 * alpha * q2 + q1;
  p.d1 = (T)2 * q2 + (q2 == (T)0 ? (T)kMinVal : (T)0);
  p.full = true;
  return p;
}

template <class S, bool Q0 = true, class T = LsReal<S>>
__device__ __forceinline__ LsPtT<T> ls_eval(const S& s, int lane, const float qg[3], T alpha) {
  float q0, q1, q2;
  ls_rows(s, lane, alpha, q0, q1, q2);
  if constexpr (Q0) wsum3(q0, q1, q2); else wsum2(q1, q2);
  q0 = Q0 ? q0 + qg[0] : 0.f;
  q1 = q1 + qg[1];
  q2 = q2 + qg[2];
  LsPtT<T> p = ls_make<T>(alpha, q0, q1, q2);
  p.full = Q0;
  return p;
}
// the deferred constant parts of two line-search points in one row pass
template <class S, class T>
__device__ __forceinline__ void ls_finish(const S& s, int lane, const float qg[3], LsPtT<T>& a, LsPtT<T>& b) {
  float qa = 0.f, qb = 0.f;
  for (int r = lane; r < s.nefc; r += WAVE) {
    const float jar = s.efc_jar[r], jv = s.efc_jv[r];
    const bool eq = (s.efc_src[r] >> 24) == 1;
    const float c0 = 0.5f * s.efc_D[r] * jar * jar;
    if (eq || ls_neg(jar, jv, a.alpha)) qa += c0;
    if (eq || ls_neg(jar, jv, b.alpha)) qb += c0;
  }
  wsum2(qa, qb);
  qa = qa + qg[0];
  qb = qb + qg[0];
  if (!a.full) { a.cost = a.cost + qa; a.full = true; }
  if (!b.full) { b.cost = b.cost + qb; b.full = true; }
}

// three line-search points in one pass over the rows; the 9 reductions are
// independent so their DPP chains interleave
template <class S, bool Q0 = true, class T = LsReal<S>>
__device__ __forceinline__ void ls_eval3(const S& s, int lane, const float qg[3], T a0, T a1, T a2,
                                         LsPtT<T>& p0, LsPtT<T>& p1, LsPtT<T>& p2) {
  float q[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const T al[3] = {a0, a1, a2};
  for (int r = lane; r < s.nefc; r += WAVE) {
    const float jar = s.efc_jar[r], jv = s.efc_jv[r], D = s.efc_D[r];
    const bool eq = (s.efc_src[r] >> 24) == 1;
    if constexpr (S::WIDE) {
      if (ell_row(s.efc_src[r])) continue;
    }
    const float c0 = 0.5f * D * jar * jar, c1 = D * jv * jar, c2 = 0.5f * D * jv * jv;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      if (eq || ls_neg(jar, jv, al[k])) { q[3 * k] += c0; q[3 * k + 1] += c1; q[3 * k + 2] += c2; }
    }
  }
  if constexpr (Q0) {
    wsum3(q[0], q[1], q[2]);
    wsum3(q[3], q[4], q[5]);
    wsum3(q[6], q[7], q[8]);
  } else {
    wsum3(q[1], q[2], q[4]);
    wsum3(q[5], q[7], q[8]);
  }
#pragma unroll
  for (int k = 0; k < 9; k++) q[k] = (Q0 || k % 3) ? q[k] + qg[k % 3] : 0.f;
  p0 = ls_make<T>(a0, q[0], q[1], q[2]);
  p1 = ls_make<T>(a1, q[3], q[4], q[5]);
  p2 = ls_make<T>(a2, q[6], q[7], q[8]);
  p0.full = p1.full = p2.full = Q0;
}

// ---------------------------------------------------------------------------
// elliptic friction cone of one condim-3 contact (rows n, t1, t2; equal
// sliding frictions), MuJoCo's primal three-zone cost (oracle: ell_update /
// ell_line).  N = mu x_n, U = fri x_t, T = |U|:
//   top    N >= mu T        no cost
//   bottom mu N + T <= 0    0.5 sum D_k x_k^2
//   middle                  0.5 Dm (N - mu T)^2, Dm = D_n / (mu^2 (1 + mu^2))

// cost; f = -dcost/dx; h = Hessian (h00 h01 h02 h11 h12 h22)
__device__ __forceinline__ float cone_update(const float x[3], float mu, float fri, const float D[3], float f[3],
                                             float h[6]) {
  const float N = mu * x[0], U0 = fri * x[1], U1 = fri * x[2], T = sqrtf(U0 * U0 + U1 * U1);
  if (N >= mu * T || (T <= 0.f && N >= 0.f)) {
    f[0] = f[1] = f[2] = 0.f;
#pragma unroll
    for (int k = 0; k < 6; k++) h[k] = 0.f;
    return 0.f;
  }
  if (mu * N + T <= 0.f || (T <= 0.f && N < 0.f)) {
    f[0] = -D[0] * x[0]; f[1] = -D[1] * x[1]; f[2] = -D[2] * x[2];
    h[0] = D[0]; h[1] = 0.f; h[2] = 0.f; h[3] = D[1]; h[4] = 0.f; h[5] = D[2];
    return 0.5f * (D[0] * x[0] * x[0] + D[1] * x[1] * x[1] + D[2] * x[2] * x[2]);
  }
  const float Dm = D[0] / (mu * mu * (1.f + mu * mu)), phi = N - mu * T, iT = 1.f / T;
  const float g[3] = {mu, -mu * fri * U0 * iT, -mu * fri * U1 * iT};
  f[0] = -Dm * phi * g[0]; f[1] = -Dm * phi * g[1]; f[2] = -Dm * phi * g[2];
  const float c = -Dm * phi * mu * fri * fri * iT, u0 = U0 * iT, u1 = U1 * iT;
  h[0] = Dm * g[0] * g[0];
  h[1] = Dm * g[0] * g[1];
  h[2] = Dm * g[0] * g[2];
  h[3] = Dm * g[1] * g[1] + c * (1.f - u0 * u0);
  h[4] = Dm * g[1] * g[2] - c * u0 * u1;
  h[5] = Dm * g[2] * g[2] + c * (1.f - u1 * u1);
  return 0.5f * Dm * phi * phi;
}

// cost and its first two derivatives along x + alpha v (zones at alpha)
template <class A>
__device__ __forceinline__ void cone_line(const float x0[3], const float v[3], A alpha, float mu, float fri,
                                          const float D[3], float& c0, float& c1, float& c2) {
  const float x[3] = {(float)((A)x0[0] + alpha * (A)v[0]), (float)((A)x0[1] + alpha * (A)v[1]),
                      (float)((A)x0[2] + alpha * (A)v[2])};
  const float N = mu * x[0], U0 = fri * x[1], U1 = fri * x[2], W0 = fri * v[1], W1 = fri * v[2];
  const float T = sqrtf(U0 * U0 + U1 * U1);
  if (N >= mu * T || (T <= 0.f && N >= 0.f)) { c0 = c1 = c2 = 0.f; return; }
  if (mu * N + T <= 0.f || (T <= 0.f && N < 0.f)) {
    c0 = 0.5f * (D[0] * x[0] * x[0] + D[1] * x[1] * x[1] + D[2] * x[2] * x[2]);
    c1 = D[0] * x[0] * v[0] + D[1] * x[1] * v[1] + D[2] * x[2] * v[2];
    c2 = D[0] * v[0] * v[0] + D[1] * v[1] * v[1] + D[2] * v[2] * v[2];
    return;
  }
  const float Dm = D[0] / (mu * mu * (1.f + mu * mu));
  const float T1 = (U0 * W0 + U1 * W1) / T, T2 = (W0 * W0 + W1 * W1 - T1 * T1) / T;
  const float phi = N - mu * T, phi1 = mu * v[0] - mu * T1, phi2 = -mu * T2;
  c0 = 0.5f * Dm * phi * phi;
  c1 = Dm * phi * phi1;
  c2 = Dm * (phi1 * phi1 + phi * phi2);
}

template <class S>
__device__ __forceinline__ const float* jrow_ptr(const S& s, const float* gx, int r) {
  return (S::JL == S::MAXEFC || r < S::JL) ? &s.J[r][0] : gx + (r - S::JL) * S::LDJ;
}

// line-search extra terms of the elliptic contacts at three step sizes
template <class S, class T>
__device__ __forceinline__ void ls_cones3(const S& s, const DevModel* __restrict__ m, int lane, const T al[3],
                                          float e[9]) {
#pragma unroll
  for (int k = 0; k < 9; k++) e[k] = 0.f;
  for (int r = lane; r < s.nefc; r += WAVE) {
    const int src = s.efc_src[r];
    if (!ell_head(src)) continue;
    const int p = ell_pair(src);
    const float x[3] = {s.efc_jar[r], s.efc_jar[r + 1], s.efc_jar[r + 2]};
    const float v[3] = {s.efc_jv[r], s.efc_jv[r + 1], s.efc_jv[r + 2]};
    const float D[3] = {s.efc_D[r], s.efc_D[r + 1], s.efc_D[r + 2]};
#pragma unroll
    for (int k = 0; k < 3; k++) {
      float c0, c1, c2;
      cone_line(x, v, al[k], m->pair_cmu[p], m->pair_friction[p], D, c0, c1, c2);
      e[3 * k] += c0; e[3 * k + 1] += c1; e[3 * k + 2] += c2;
    }
  }
  wsum3(e[0], e[1], e[2]);
  wsum3(e[3], e[4], e[5]);
  wsum3(e[6], e[7], e[8]);
}

template <class T>
__device__ __forceinline__ void ls_add(LsPtT<T>& p, float c0, float c1, float c2) {
  p.cost += (T)c0;
  p.d0 += (T)c1;
  p.d1 = p.d1 - (p.d1 == (T)kMinVal ? (T)kMinVal : (T)0) + (T)c2;
  if (p.d1 == (T)0) p.d1 = (T)kMinVal;
}

}  // namespace mpcr
