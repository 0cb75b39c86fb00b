// spd_solve.h -- the dense SPD solves of the rollout kernel, rows in registers.
#pragma once
#include "rollout.h"
#include "wave.h"
#include "vecmath.h"

namespace mpcr {

// ---------------------------------------------------------------------------
// dense SPD solve, row-per-lane in registers.  Lane i (< DX_NV) holds row i
// of A in a[]; rows >= n must be identity rows.  On return a[] holds row i of
// the lower Cholesky factor.  x = A^-1 b for b held one value per lane.

// All DX_NV pivots run even when nv is smaller: a run-time exit inside the
// unrolled chain breaks it into blocks the scheduler cannot overlap
// (measured 4.07 -> 4.94 ms), while the padded pivots cost 2/16 of it.
template <int N>
__device__ __forceinline__ void chol_rows(float (&a)[N], int lane) {
#pragma unroll
  for (int k = 0; k < N; k++) {
    float dkk = sqrtf(fmaxf(rdlane(a[k], k), kMinVal));
    float lik = lane == k ? dkk : (lane > k ? a[k] / dkk : 0.f);
    a[k] = lik;
#pragma unroll
    for (int j = k + 1; j < N; j++) {
      float ljk = rdlane(lik, j);
      a[j] = fmaf(-lik, ljk, a[j]);
    }
  }
}

// x = L^-T L^-1 b with lane i holding row i of L in l[].  Forward pass: lane
// k finalises y_k, one v_readlane broadcasts it, every lane updates its own
// accumulator with its own register l[k].  For the backward pass each lane
// needs its COLUMN of L: the rows are scattered transposed to the LDS scratch
// Lt[DX_NV][LDL] once, each lane reads its column back with 4 ds_read_b128,
// and the same broadcast chain runs backwards.  32 readlanes per solve.
// Returns x[lane].  Must be called by all lanes (one barrier).
template <int N, int LDL>
__device__ __forceinline__ float chol_solve(const float (&l)[N], float b, int lane, float* Lt) {
  if (lane < N) {
#pragma unroll
    for (int j = 0; j < N; j++) Lt[j * LDL + lane] = l[j];
  }
  float acc = b, y = 0.f;
#pragma unroll
  for (int k = 0; k < N; k++) {
    const float yk = rdlane(acc, k) / rdlane(l[k], k);
    if (lane > k) acc = fmaf(-l[k], yk, acc);
    if (lane == k) y = yk;
  }
  sync();
  float lt[N];
  {
    const float4* col = reinterpret_cast<const float4*>(Lt + (lane < N ? lane : 0) * LDL);
#pragma unroll
    for (int q = 0; q < N / 4; q++) {
      const float4 v = col[q];
      lt[4 * q] = v.x; lt[4 * q + 1] = v.y; lt[4 * q + 2] = v.z; lt[4 * q + 3] = v.w;
    }
  }
  float x = 0.f;
  acc = y;
#pragma unroll
  for (int k = N - 1; k >= 0; k--) {
    const float xk = rdlane(acc, k) / rdlane(l[k], k);
    if (lane < k) acc = fmaf(-lt[k], xk, acc);
    if (lane == k) x = xk;
  }
  sync();
  return x;
}

// The same factorisation and solve for N = 16 (narrow variant) with DPP row
// broadcasts instead of v_readlane: row_newbcast:j hands lane j's value to
// every lane of its 16-lane row, and as the src0 modifier of v_fmac_f32 it
// makes each (k, j) update of the right-looking factorisation ONE VALU
// instruction (readlane + fma before, plus the SGPR hazards).  Lanes 16..63
// run the same code on their own rows and their results are ignored.
template <int J>
__device__ __forceinline__ float rbc(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x150 + J, 0xF, 0xF, true));
}
// acc -= bcast_J(src) * own.  NOP: src was just written by a VALU op (DPP
// reads need 2 wait states; the compiler does not track them in inline asm)
template <int J, bool NOP>
__device__ __forceinline__ void fnmac_bc(float& acc, float src, float own) {
  if constexpr (NOP)
    asm("s_nop 1\n\tv_fmac_f32_dpp %0, -%1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
        : "+v"(acc) : "v"(src), "v"(own), "n"(J));
  else
    asm("v_fmac_f32_dpp %0, -%1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
        : "+v"(acc) : "v"(src), "v"(own), "n"(J));
}
template <int K, int J>
struct Chol16Upd {  // a[j] -= l[j][k] * l[i][k] for j = J..15
  static __device__ __forceinline__ void run(float (&a)[16], float lik) {
    fnmac_bc<J, J == K + 1>(a[J], lik, lik);
    Chol16Upd<K, J + 1>::run(a, lik);
  }
};
template <int K>
struct Chol16Upd<K, 16> {
  static __device__ __forceinline__ void run(float (&)[16], float) {}
};
// The factor is kept with a ZERO diagonal: l[i][i] lives only as its inverse
// in dinv (lane i).  The sweeps then leave lane K's accumulator alone when
// they broadcast its value, and read every result off at the end (acc * dinv)
// instead of capturing it with a per-step select.
template <int K>
struct Chol16 {  // column K; dinv collects 1 / l[i][i] at lane i
  static __device__ __forceinline__ void run(float (&a)[16], float& dinv, int lane) {
    const float dkk = sqrtf(fmaxf(rbc<K>(a[K]), kMinVal));
    const float inv = 1.f / dkk;
    const float lik = lane > K ? a[K] * inv : 0.f;
    a[K] = lik;
    dinv = lane == K ? inv : dinv;
    Chol16Upd<K, K + 1>::run(a, lik);
    Chol16<K + 1>::run(a, dinv, lane);
  }
};
template <>
struct Chol16<16> {
  static __device__ __forceinline__ void run(float (&)[16], float&, int) {}
};
// forward (L y = b) / backward (L^T x = y) sweeps: lane K's value is final
// at step K, t = acc / l_KK, and one fused DPP FMA hands it to the other
// lanes' updates (lanes already final and lane K see zero coefficients: l is
// triangular with a zero diagonal); the results are acc * dinv afterwards
template <int K, int STEP>
struct Sweep16 {
  static __device__ __forceinline__ void run(const float (&c)[16], float& acc, float dinv) {
    const float t = acc * dinv;
    fnmac_bc<K, true>(acc, t, c[K]);
    Sweep16<K + STEP, STEP>::run(c, acc, dinv);
  }
};
template <int STEP>
struct Sweep16<16, STEP> {
  static __device__ __forceinline__ void run(const float (&)[16], float&, float) {}
};
template <int STEP>
struct Sweep16<-1, STEP> {
  static __device__ __forceinline__ void run(const float (&)[16], float&, float) {}
};
// The solves launder their lane argument: the lane compares inside are
// re-derived (one v_cmp each) instead of being hoisted into spilled SGPR pairs
__device__ __forceinline__ void chol16(float (&a)[16], float& dinv, int lane) {
  asm volatile("" : "+v"(lane));
  dinv = 0.f;
  Chol16<0>::run(a, dinv, lane);
}
// Blocked variant for block-diagonal systems (the mass matrix is block
// diagonal by kinematic tree): tree t's <= 8 dofs are rows of lanes 16 t ..
// 16 t + 7, and row_newbcast:K broadcasts each tree's K-th row to its own
// lanes, so all trees factor in ONE 8-column chain (36 fused updates instead
// of 120) -- the same operations per block as the dense factorisation
// (off-block entries are exact zeros there), in the same order.
template <int N, int K, int J>
struct CholNUpd {
  static __device__ __forceinline__ void run(float (&a)[N], float lik) {
    fnmac_bc<J, J == K + 1>(a[J], lik, lik);
    CholNUpd<N, K, J + 1>::run(a, lik);
  }
};
template <int N, int K>
struct CholNUpd<N, K, N> {
  static __device__ __forceinline__ void run(float (&)[N], float) {}
};
template <int N, int K>
struct CholN {  // lr: the lane's row within its 16-lane DPP row
  static __device__ __forceinline__ void run(float (&a)[N], float& dinv, int lr) {
    const float dkk = sqrtf(fmaxf(rbc<K>(a[K]), kMinVal));
    const float inv = 1.f / dkk;
    const float lik = lr > K ? a[K] * inv : 0.f;
    a[K] = lik;
    dinv = lr == K ? inv : dinv;
    CholNUpd<N, K, K + 1>::run(a, lik);
    CholN<N, K + 1>::run(a, dinv, lr);
  }
};
template <int N>
struct CholN<N, N> {
  static __device__ __forceinline__ void run(float (&)[N], float&, int) {}
};
template <int N, int K, int STEP>
struct SweepN {
  static __device__ __forceinline__ void run(const float (&c)[N], float& acc, float dinv) {
    const float t = acc * dinv;
    fnmac_bc<K, true>(acc, t, c[K]);
    SweepN<N, K + STEP, STEP>::run(c, acc, dinv);
  }
};
template <int N, int STEP>
struct SweepN<N, N, STEP> {
  static __device__ __forceinline__ void run(const float (&)[N], float&, float) {}
};
template <int N, int STEP>
struct SweepN<N, -1, STEP> {
  static __device__ __forceinline__ void run(const float (&)[N], float&, float) {}
};
// x = A^-1 b for a symmetric A that is block diagonal by kinematic tree (tree
// t's <= N dofs on lanes 16 t ..), elem(d, dj) = A[d][dj]; b and x are
// dof-indexed LDS vectors (x may alias b).  Lt: 4 N^2-float LDS scratch (it
// may alias A's storage: every element is read before the first write).  Must
// be called by all lanes (two barriers).
// (split in two for a factor computed ahead of its solve, possibly on
// another wave: blocked_factor, then blocked_sweep -- the same operations)
template <int N, class F>
__device__ __forceinline__ void blocked_factor(const DevModel* __restrict__ m, F&& elem, int lane, float (&a)[N],
                                               float& dinv) {
  static_assert(N == 8 || N == 16, "blocked Cholesky width");
  asm volatile("" : "+v"(lane));
  const int lr = lane & 15, lb = lane & ~15;
  const int d = m->blane_dof[lane];
#pragma unroll
  for (int j = 0; j < N; j++) {
    const int dj = m->blane_dof[lb + j];
    a[j] = (d >= 0 && dj >= 0) ? elem(d, dj) : (j == lr ? 1.f : 0.f);
  }
  dinv = 0.f;
  CholN<N, 0>::run(a, dinv, lr);
}
template <int N>
__device__ __forceinline__ void blocked_sweep(const DevModel* __restrict__ m, const float (&a)[N], float dinv,
                                              const float* bv, float* xv, int lane, float* Lt) {
  asm volatile("" : "+v"(lane));
  const int lr = lane & 15, t = lane >> 4;
  const int d = m->blane_dof[lane];
  float acc = d >= 0 ? bv[d] : 0.f;
  SweepN<N, 0, 1>::run(a, acc, dinv);
  const float y = acc * dinv;
  if (lr < N) {
#pragma unroll
    for (int j = 0; j < N; j++) Lt[t * N * N + j * N + lr] = a[j];
  }
  sync();
  float lt[N];
  {
    const float4* col = reinterpret_cast<const float4*>(Lt + t * N * N + (lr & (N - 1)) * N);
#pragma unroll
    for (int q = 0; q < N / 4; q++) {
      const float4 v = col[q];
      lt[4 * q] = v.x; lt[4 * q + 1] = v.y; lt[4 * q + 2] = v.z; lt[4 * q + 3] = v.w;
    }
  }
  acc = y;
  SweepN<N, N - 1, -1>::run(lt, acc, dinv);
  const float x = acc * dinv;
  sync();
  if (d >= 0) xv[d] = x;
}
template <int N, class F>
__device__ __forceinline__ void blocked_solve(const DevModel* __restrict__ m, F&& elem, const float* bv, float* xv,
                                              int lane, float* Lt) {
  float a[N], dinv;
  blocked_factor<N>(m, elem, lane, a, dinv);
  blocked_sweep<N>(m, a, dinv, bv, xv, lane, Lt);
}
// the blocked (per-tree) Cholesky for M and uncoupled Newton Hessians, for a
// kernel variant of NVW dofs: 8-wide chains in the
// narrow kernel (trees <= 8 dofs), 16-wide in the dual-arm one (trees <= 16)
template <int NVW>
__device__ __forceinline__ bool blk_usable(const DevModel* __restrict__ m) {
  return NVW == 16 ? m->blk_n == 8 : m->blk_n != 0;
}
template <int NVW, class F>
__device__ __forceinline__ void blk_solve(const DevModel* __restrict__ m, F&& elem, const float* bv, float* xv,
                                          int lane, float* Lt) {
  blocked_solve<NVW == 16 ? 8 : 16>(m, elem, bv, xv, lane, Lt);
}

// x = L^-T L^-1 b (lane i: row i of L in l[]); Lt: LDS transpose scratch
template <int LDL>
__device__ __forceinline__ float chol16_solve(const float (&l)[16], float dinv, float b, int lane, float* Lt) {
  asm volatile("" : "+v"(lane));
  if (lane < 16) {
#pragma unroll
    for (int j = 0; j < 16; j++) Lt[j * LDL + lane] = l[j];
  }
  float acc = b;
  Sweep16<0, 1>::run(l, acc, dinv);
  const float y = acc * dinv;
  sync();
  float lt[16];
  {
    const float4* col = reinterpret_cast<const float4*>(Lt + (lane & 15) * LDL);
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const float4 v = col[q];
      lt[4 * q] = v.x; lt[4 * q + 1] = v.y; lt[4 * q + 2] = v.z; lt[4 * q + 3] = v.w;
    }
  }
  acc = y;
  Sweep16<15, -1>::run(lt, acc, dinv);
  const float x = acc * dinv;
  sync();
  return x;
}

}  // namespace mpcr
