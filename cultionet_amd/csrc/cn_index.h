// Index, window and mask rules that the fp32 NCHW and the bf16 NHWC kernels must decide identically: each is defined
// here once and force-inlined into both families.
#pragma once
#include "cn_common.h"

// ---- bilinear resize, align_corners=True ---------------------------------------------------------------------------
static inline float cn_bl_scale(int in_size, int out_size) {
  return out_size > 1 ? (float)(in_size - 1) / (float)(out_size - 1) : 0.f;
}

// Source pixels i0, i1 and the weight l1 of i1 for output index o: ATen's area_pixel_compute_source_index in fp32.
__device__ __forceinline__ void cn_bl_src(int o, float scale, int in_size, int& i0, int& i1, float& l1) {
#pragma clang fp contract(off)  // ATen rounds scale*o before subtracting floor(): an fma here shifts lambda by ~1e-6
  const float src = scale * (float)o;
  i0 = (int)src;
  if (i0 > in_size - 1) i0 = in_size - 1;
  i1 = i0 + ((i0 < in_size - 1) ? 1 : 0);
  l1 = src - i0;
}

// Adjoint: the output indices reading input index i and their weights (<= 4 for resizes that shrink by less than 2x);
// returns their number, idx / wgt hold the first four. Candidates: src in (i-1, i+1) -> o in ((i-1)/s, (i+1)/s),
// widened by one for rounding.
__device__ __forceinline__ int cn_bl_candidates(int i, int in_size, int out_size, float scale, float inv_scale,
                                                int* idx, float* wgt) {
  int lo = (int)floorf((i - 1) * inv_scale) - 1, hi = (int)ceilf((i + 1) * inv_scale) + 1;
  if (scale == 0.f) { lo = 0; hi = out_size - 1; }
  lo = max(lo, 0);
  hi = min(hi, out_size - 1);
  // The outputs reading input index i are CONSECUTIVE (the source coordinate is monotonic; a zero weight can only be
  // the first output of the run, whose source falls exactly on i - 1): the search only counts them and notes the first,
  // the <= 4 weights are then recomputed with static register indices. (Storing idx[n] / wgt[n] from inside the search
  // loop through an if-chain on n lost candidate 1 whenever a fourth one was found -- resizes growing by 1.5x..2x.)
  int n = 0, first = 0;
#pragma unroll 1
  for (int o = lo; o <= hi; ++o) {
    int i0, i1; float l1;
    cn_bl_src(o, scale, in_size, i0, i1, l1);
    float w = 0.f;
    if (i0 == i) w += 1.f - l1;
    if (i1 == i) w += l1;
    if (w != 0.f) {
      if (n == 0) first = o;
      ++n;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool live = k < n;
    const int o = live ? first + k : first;
    int i0, i1; float l1;
    cn_bl_src(o, scale, in_size, i0, i1, l1);
    float w = 0.f;
    if (i0 == i) w += 1.f - l1;
    if (i1 == i) w += l1;
    idx[k] = o;
    wgt[k] = live ? w : 0.f;
  }
  return n;
}

// ---- neighborhood attention, kernel size 3 -------------------------------------------------------------------------
#define CN_NA_K 3
#define CN_NA_KK 9

// natten get_window_start (K = 3, n = 1)
__device__ __forceinline__ int cn_na_window_start(int i, int len, int dil) {
  if (dil <= 1) return max(i - 1, 0) + ((i + 1 >= len) ? (len - i - 2) : 0);
  const int ni = i - dil;
  if (ni < 0) return i % dil;
  if (i + dil >= len) {
    const int imodd = i % dil;
    const int a = (len / dil) * dil;
    const int b = len - a;
    if (imodd < b) return len - b + imodd - 2 * dil;
    return a + imodd - CN_NA_K * dil;
  }
  return ni;
}

// ---- dropout masks ---------------------------------------------------------------------------------------------------
// keep(i) = cn_splitmix64(seed + i) >= thresh with thresh = p * 2^64, saturated; 0 (keep everything) for p <= 0.
static inline unsigned long long cn_dropout_thresh(float p) {
  if (!(p > 0.f)) return 0ull;
  const double t = (double)p * 18446744073709551616.0;  // p * 2^64
  return t >= 18446744073709551615.0 ? ~0ull : (unsigned long long)t;
}

// attn_drop (nn.Dropout on the soft-maxed logits [B*heads][9][H*W]): keep/(1-p) factor of tap t of query pixel p,
// recomputed from the counter hash in forward and backward; 1.0 when dropout is off.
__device__ __forceinline__ float cn_na_keep(unsigned long long thresh, float scale, unsigned long long seed, long bh,
                                            int t, int HW, int p) {
  if (thresh == 0ull) return 1.0f;
  const unsigned long long i = ((unsigned long long)bh * CN_NA_KK + t) * (unsigned long long)HW + p;
  return cn_splitmix64(seed + i) >= thresh ? scale : 0.f;
}

// ---- maxima ----------------------------------------------------------------------------------------------------------
// F.adaptive_max_pool2d: window of output o along one axis is [floor(o*In/Out), ceil((o+1)*In/Out)).
__device__ __forceinline__ int cn_amp_start(int o, int in, int out) { return (int)(((long)o * in) / out); }
__device__ __forceinline__ int cn_amp_end(int o, int in, int out) { return (int)((((long)(o + 1)) * in + out - 1) / out); }

// A NaN wins the maximum (ATen: val > max || isnan(val), so the last NaN stays; torch.amax propagates it).
__device__ __forceinline__ bool cn_max_takes(float m, float v) { return v > m || v != v; }
__device__ __forceinline__ float cn_max_nan(float m, float v) { return cn_max_takes(m, v) ? v : m; }
