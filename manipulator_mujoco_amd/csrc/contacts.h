// contacts.h -- contact bookkeeping of the rollout kernel: the slot history, the
// active-contact list.
#pragma once
#include "rollout_switches.h"
#include "kernarg.h"
#include "wave.h"
#include "narrow_lane.h"

namespace mpcr {

// Per-lane contact bookkeeping after a narrow-phase pass: cost_c on the
// robot-masked slots (SBP/mjx_planner.py:284-296) and ballot-compacted append
// of the active contacts.  Must be called by all lanes (two barriers).
// Previous-step masked slot distances (cost_c's history term) of the lane's
// own pairs, held in registers across the horizon (narrow variant): the lane
// that owns pair p in 64-pair chunk k owns its <= 4 slots every step, so
// chunk k < NC keeps them in v[k][0..3] (no per-step HBM slab round trip: the
// slab's L2 evictions were ~8.6 MB of a C3 launch's 29.7 MB HBM traffic);
// pairs of later chunks use the slab.  The dual-arm class keeps the slab.
template <class S>
struct SlotHist {
  static constexpr int NC = S::WIDE ? 0 : 128 / WAVE;
  float v[NC > 0 ? NC : 1][4];
};

// the active contacts (dist < margin) of pair p into the contact list from
// position o on (those past MAXACT are dropped; the caller counts them)
template <class S>
__device__ __forceinline__ void put_contacts(const DevModel* __restrict__ m, S& s, int o, int p, int nsl,
                                             const float dist[4], const float pos[4][3], const float nrm[4][3]) {
  const float mg = m->pair_margin[p];
#pragma unroll
  for (int c = 0; c < 4; c++) {
    if (c < nsl && dist[c] < mg) {
      if (o < S::MAXACT) {
        float f[9];
        make_frame(f, nrm[c]);
        s.con_pos[o][0] = pos[c][0]; s.con_pos[o][1] = pos[c][1]; s.con_pos[o][2] = pos[c][2];
#pragma unroll
        for (int e = 0; e < S::FRAMEW; e++) s.con_frame[o][e] = f[e];
        s.con_dist[o] = dist[c];
        s.con_pair[o] = p;
      }
      o++;
    }
  }
}

// SW (the STATE / SCEN kernels): the call's slot weights (rollout.h SlotWArgs)
// price the lane's slots -- cost_c += w[slot] * term where it was cost_c +=
// term -- read here, at the use, from the problem's L2-resident block: the
// pointer and the stride from the kernarg segment, the problem from the
// candidate, so no register holds anything of them across the step (a resumed
// horizon segment looks the same block up again).  A null block is w = 1, which
// leaves every sum bitwise what it was.  Without SW the terms fold away.
template <class S, bool SW = false>
__device__ __forceinline__ void emit_contacts(const DevModel* __restrict__ m, S& s, const RolloutArgs& args,
                                              [[maybe_unused]] unsigned aflags, int b,
                                              int t, int H, bool valid, int p, int nsl, const float dist[4],
                                              const float pos[4][3], const float nrm[4][3], float& cost_c,
                                              SlotHist<S>& sh, int k,
                                              [[maybe_unused]] const float4* rq = nullptr,
                                              [[maybe_unused]] float a_col = 1.f) {
  int act = 0;
  if (valid) {
    // single-arm kernels: slot address, slot count and margin from the pair's
    // set-up record, the two quads the chunk loop fetched (rq)
    float4 q0 = {0.f, 0.f, 0.f, 0.f}, q1 = q0;
    if constexpr (kStepLoad<S>) {
      q0 = rq[0];
      q1 = rq[1];
    }
    const int sa = kStepLoad<S> ? __float_as_int(q0.y) : m->pair_slotadr[p];
    if (sa >= 0) {
      const int ns = kStepLoad<S> ? __float_as_int(q1.x) >> 16 : m->pair_ncon[p];
      float w[4] = {1.f, 1.f, 1.f, 1.f};
      if constexpr (SW) {
        const float* wp = KSW->slot_w;
        if (wp) {
          // (the problem fields from the segment too, in both units: no by-value copy of them held across
          //  the horizon loop for this one use)
          const int pn = *kernarg_at<int>(offsetof(RolloutArgs, prob_n));
          const int po = *kernarg_at<int>(offsetof(RolloutArgs, prob_off));
          wp += (size_t)(pn ? (po + b) / pn : 0) * (unsigned)KSW->stride + sa;
#pragma unroll
          for (int c = 0; c < 4; c++)
            if (c < ns) w[c] = wp[c];
        }
        // the call's step weights (StepWArgs): this step's a_col -- the
        // caller's, read once ahead of the phase (single-arm kernels), or read
        // here like the slot weights (dual-arm kernels) -- folds into the slot
        // weights: cost_c += (a_col[t] w[slot]) * term, the approach term of
        // step t included.  1 (no schedule, or ones) leaves w what it was.
        if constexpr (S::WIDE) {
          if (const float* row = step_w_row(b, t)) a_col = row[2];
        }
#pragma unroll
        for (int c = 0; c < 4; c++) w[c] *= a_col;
      }
      if constexpr (SlotHist<S>::NC == 2) {
        // single-arm kernels: the chunk index is the wave's, so a scalar branch
        // names the chunk's history registers (hv; null: the slab) where
        // per-slot selects over k read and wrote them
        auto slots = [&](float* hv) {
#pragma unroll
          for (int c = 0; c < 4; c++) {
            if (c < ns) {
              const float d = dist[c];
              if (d < 0.f) cost_c += w[c] * 1.f;
              if (hv) {
                if (t > 0) cost_c += w[c] * fmaxf(hv[c] * (1.f - 0.005f) - d, 0.f);
                hv[c] = d;
              } else {
                float* cp = KA->slot_prev + (size_t)b * m->nslot;
                if (t > 0) cost_c += w[c] * fmaxf(cp[sa + c] * (1.f - 0.005f) - d, 0.f);
                cp[sa + c] = d;
              }
              if (ARGS_HAS(AF_TRACE_SLOTS, KA->trace_slots && b < KA->n)) KA->trace_slots[((size_t)b * H + t) * m->nslot + sa + c] = d;
            }
          }
        };
        const int ku = __builtin_amdgcn_readfirstlane(k);
        if (ku == 0) slots(sh.v[0]);
        else if (ku == 1) slots(sh.v[1]);
        else slots(nullptr);
      } else {
#pragma unroll
      for (int c = 0; c < 4; c++) {
        if (c < ns) {
          const float d = dist[c];
          if (d < 0.f) cost_c += w[c] * 1.f;
          if (SlotHist<S>::NC > 0 && k < SlotHist<S>::NC) {  // this lane's registers (chunk k, slot c)
            float prev = 0.f;
#pragma unroll
            for (int j = 0; j < SlotHist<S>::NC; j++) prev = j == k ? sh.v[j][c] : prev;
            if (t > 0) cost_c += w[c] * fmaxf(prev * (1.f - 0.005f) - d, 0.f);
#pragma unroll
            for (int j = 0; j < SlotHist<S>::NC; j++) sh.v[j][c] = j == k ? d : sh.v[j][c];
          } else {
            float* cp = KA->slot_prev + (size_t)b * m->nslot;
            if (t > 0) cost_c += w[c] * fmaxf(cp[sa + c] * (1.f - 0.005f) - d, 0.f);
            cp[sa + c] = d;
          }
          if (ARGS_HAS(AF_TRACE_SLOTS, KA->trace_slots && b < KA->n)) KA->trace_slots[((size_t)b * H + t) * m->nslot + sa + c] = d;
        }
      }
      }
    }
    if (!(m->disableflags & 16)) {
      const float mg = kStepLoad<S> ? q1.w : m->pair_margin[p];
#pragma unroll
      for (int c = 0; c < 4; c++) act += (c < nsl && dist[c] < mg) ? 1 : 0;
    }
  }
  int tot;
  const int pre = wscan_excl(act, tot);
  const int base = s.ncon;
  if (act) put_contacts(m, s, base + pre, p, nsl, dist, pos, nrm);
  sync();
  if ((threadIdx.x & (WAVE - 1)) == 0) s.ncon = base + tot;
  sync();
}

}  // namespace mpcr
