// The last line of the five chip prologues (cn_prepare_chips_kernel, cn_window_chips_kernel in cn_edges.hip;
// cn_augment_x_kernel, cn_augment_series_kernel, cn_augment_target_kernel in cn_augment.hip): final clip, the optional
// log transform of EdgeDataset.get (data/datasets.py:481-484, torch.log(x * 50.0 + 1.0).clamp_min(1e-9), between the
// augmentation and the z-score), then the NormValues z-score. One definition, so the five agree bit for bit.
#pragma once
#include "cn_common.h"

// LOG = false is the plain store: its CnChipLog is empty, so a plain kernel takes no argument for the transform and
// compiles to the clip and the z-score alone. LOG = true, in fp32 step by step as torch does it:
//   t = v * gain    u = t + 1    (two roundings: never contracted into an fma, which would move the low bins by
//                                 hundreds of ulp of log u)
//   w = max(log u, floor)        (log in double, rounded once: within half an ulp next to u = 1, where w ~ 0.005;
//                                 v_log_f32 is not)
// A stored 0, a negative value and a zero-filled window border arrive as v = lo = 1e-9: u = 1, log u = 0, w = floor.
template <bool LOG>
struct CnChipLog {
  float gain, floor;
};
template <>
struct CnChipLog<false> {};

template <bool LOG>
struct CnChipStore {
  float* p;
  float lo, hi, m, inv;
  CnChipLog<LOG> lg;
  // v already lies in [lo, hi]
  __device__ __forceinline__ void put(long i, float v) const {
    if constexpr (LOG) {
      // contraction is switched off for this block: __fmul_rn / __fadd_rn are plain operators in HIP's headers and
      // fuse under the default -ffp-contract=fast like any other product and sum
#pragma clang fp contract(off)
      const float t = v * lg.gain;
      const float u = t + 1.0f;
      v = fmaxf((float)log((double)u), lg.floor);
    }
    p[i] = (v - m) * inv;
  }
  // final clip (x: then log, z-score; bdist: m = 0, inv = 1, LOG = false)
  __device__ __forceinline__ void operator()(long i, float v) const { put(i, fminf(fmaxf(v, lo), hi)); }

  // For a loop that does fp32 arithmetic of its own in front of the store (the blur, the bilinear resize, the noise):
  // the compiler contracts such an expression into fmas as it sees fit for each loop it generates, and a loop that also
  // holds the logarithm is not the loop of the plain kernel, so the two would differ in the last bit of v here and there
  // -- a handful of ulp of w at the low bins. Such a loop stores through values(), which for LOG writes the clipped v
  // alone, exactly the loop of the plain kernel, and the same thread then transforms its elements in place with
  // finish(). For LOG = false values() is the store itself and finish() is empty.
  __device__ __forceinline__ CnChipStore<false> values() const {
    if constexpr (LOG) return CnChipStore<false>{p, lo, hi, 0.f, 1.f, {}};
    else return *this;
  }
  __device__ __forceinline__ void finish(long i) const {
    if constexpr (LOG) put(i, p[i]);
  }
};
