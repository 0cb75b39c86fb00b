// narrow_prims.h -- primitive narrow phase of the rollout kernel: segment and box distances.
#pragma once
#include "rollout.h"
#include "vecmath.h"

namespace mpcr {

// ---------------------------------------------------------------------------
// narrow phase (contact definitions identical to the oracle's)

__device__ __forceinline__ void seg_seg(const float p1[3], const float d1[3], const float p2[3], const float d2[3],
                                        float* sc, float* tc) {
  float r[3] = {p1[0] - p2[0], p1[1] - p2[1], p1[2] - p2[2]};
  float a = dot3(d1, d1), e = dot3(d2, d2), f = dot3(d2, r);
  float s, t;
  if (a <= kMinVal && e <= kMinVal) { *sc = 0; *tc = 0; return; }
  if (a <= kMinVal) {
    s = 0; t = clampf(f / e, 0, 1);
  } else {
    float c = dot3(d1, r);
    if (e <= kMinVal) {
      t = 0; s = clampf(-c / a, 0, 1);
    } else {
      float b = dot3(d1, d2), den = a * e - b * b;
      s = den > 1e-12f * a * e ? clampf((b * f - c * e) / den, 0, 1) : 0.f;
      t = (b * s + f) / e;
      if (t < 0) { t = 0; s = clampf(-c / a, 0, 1); }
      else if (t > 1) { t = 1; s = clampf((b - c) / a, 0, 1); }
    }
  }
  *sc = s; *tc = t;
}

__device__ __forceinline__ float point_box(const float p[3], const float h[3], float nl[3], float q[3]) {
  float out2 = 0, o[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    q[k] = clampf(p[k], -h[k], h[k]);
    o[k] = q[k] - p[k];
    out2 += o[k] * o[k];
  }
  if (out2 > 0) {
    const float l = sqrtf(out2);
#pragma unroll
    for (int k = 0; k < 3; k++) nl[k] = o[k] / l;
    return l;
  }
  // inside: the deepest face is argmax_k |p_k| - h_k; ties within 1 um go to
  // the lower axis and a point on the box's mid-plane to the + face (the
  // oracle's point_box rule)
  const float g0 = fabsf(p[0]) - h[0], g1 = fabsf(p[1]) - h[1], g2 = fabsf(p[2]) - h[2];
  int best = 0;
  float g = g0;
  if (g1 > g + 1e-6f) { g = g1; best = 1; }
  if (g2 > g + 1e-6f) { g = g2; best = 2; }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float sg = p[k] >= -1e-6f ? 1.f : -1.f;
    nl[k] = k == best ? -sg : 0.f;
    q[k] = k == best ? sg * h[k] : p[k];
  }
  return g;
}

}  // namespace mpcr
