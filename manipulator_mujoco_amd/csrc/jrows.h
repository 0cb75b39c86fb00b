// jrows.h -- constraint-row (J) access of the rollout kernel, LDS or HBM slab, and its
// row products on the matrix core.
#pragma once
#include "rollout.h"
#include "vecmath.h"

namespace mpcr {

// ---------------------------------------------------------------------------
// J row access: rows < JL in LDS, the rest in the block's HBM slab gx.  The
// branches are per lane, and the HBM side is skipped (execz) unless a lane
// has a row past JL.

template <class S>
__device__ __forceinline__ void jstore(S& s, float* gx, int r, int i, float v) {
  if (S::JL == S::MAXEFC || r < S::JL) s.J[r][i] = v;
  else gx[(r - S::JL) * S::LDJ + i] = v;
}
template <class S>
__device__ __forceinline__ float jdot(const S& s, const float* gx, int r, const float* vec) {
  if (S::JL == S::MAXEFC || r < S::JL) return dotN<S::NVW>(s.J[r], vec);
  return dotN<S::NVW>(gx + (r - S::JL) * S::LDJ, vec);
}
// body(row pointer, r) over rows r = r0, r0 + step, ... < nefc: the LDS rows,
// then the slab rows (two loops, no per-row address-space select)
template <class S, class F>
__device__ __forceinline__ void jrows(const S& s, const float* gx, int r0, int step, int nefc, F&& body) {
  const int n1 = nefc < S::JL ? nefc : S::JL;
  for (int r = r0; r < n1; r += step) body(&s.J[r][0], r);
  if constexpr (S::JL < S::MAXEFC) {
    for (int r = S::JL + r0; r < nefc; r += step) body(gx + (r - S::JL) * S::LDJ, r);
  }
}

// narrow variant: the Newton gradient J^T f and Hessian J^T D J on the matrix
// core (v_mfma_f32_16x16x4_f32) instead of per-row VALU loops
typedef float mfx4 __attribute__((ext_vector_type(4)));
typedef float mfx16 __attribute__((ext_vector_type(16)));
// narrow variant: the chain / subtree sums of the dynamics (CRB, body
// velocities, cdof_dot, RNE accelerations, bias forces) and the mass matrix as
// 16 x 16 (x 16) products on the matrix core: a 0/1 (or qvel-weighted) chain
// mask times per-dof / per-body rows.  v_mfma_f32_16x16x4_f32 is a k-ordered
// fmaf chain, and the products are the loops' own (qvel x cdof, fvec x cdof),
// so the results are bitwise the per-lane loops'
// acc + A B over k < 16 (4 instructions): lane l supplies A[l & 15][k] =
// af(l & 15, k) and B[k][l & 15] = bf(k, l & 15) for its k = 4 s + (l >> 4);
// register v of lane l then holds row 4 (l >> 4) + v, column l & 15
template <int KB, class AF, class BF>
__device__ __forceinline__ mfx4 mm16(AF&& af, BF&& bf, mfx4 acc, int lane) {
  const int i = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int s4 = 0; s4 < KB; s4++) {
    const int k = 4 * s4 + kq;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af(i, k), bf(k, i), acc, 0, 0, 0);
  }
  return acc;
}
// the same for the 32-wide (dual-arm) Newton on v_mfma_f32_32x32x2_f32
// (neutral while the 32-wide readlane Cholesky dominated; with the blocked
// per-tree solve C4 66.2 -> 65.2 ms)

// 32-wide: acc += sum over constraint rows, two per v_mfma_f32_32x32x2_f32
// (lane (gi, gq) supplies A = J[r0 + gq][gi] and B = bf(r, A)).  Rows < JL
// come from LDS; the HBM-slab rows (heavily constrained candidates: 100+
// rows) are read four row pairs at a time with the loads issued together,
// instead of one dependent flat load per instruction.  Same MFMAs in the same
// row order (pairs wholly past nefc skipped): bitwise the single loop.
template <class S, class BF>
__device__ __forceinline__ mfx16 mfma_rows32(const S& s, const float* gx, int nefc, int gi, int gq, BF&& bf,
                                             mfx16 acc) {
  static_assert(S::JL % 2 == 0, "a row group never straddles the LDS / slab boundary");
  const int n1 = nefc < S::JL ? nefc : S::JL;
  for (int r0 = 0; r0 < n1; r0 += 2) {
    const int r = r0 + gq;
    const bool ok = r < nefc;
    const float a = ok ? s.J[r][gi] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, ok ? bf(r, a) : 0.f, acc, 0, 0, 0);
  }
  if constexpr (S::JL < S::MAXEFC) {
    for (int r0 = S::JL; r0 < nefc; r0 += 8) {
      float a[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int r = r0 + 2 * u + gq;
        a[u] = r < nefc ? gx[(r - S::JL) * S::LDJ + gi] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int r = r0 + 2 * u + gq;
        if (r0 + 2 * u < nefc)
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], r < nefc ? bf(r, a[u]) : 0.f, acc, 0, 0, 0);
      }
    }
  }
  return acc;
}

}  // namespace mpcr
