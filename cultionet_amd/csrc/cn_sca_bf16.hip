// Mixed-precision (bf16 NHWC) kernels of the two constructor variants that have their own reductions:
//   attention_weights="spatial_channel" -- SpatialChannelAttention (reference nn/modules/attention.py:12-126, applied
//     at nn/modules/convolution.py:388-393): the pools of the skip tensor and the gating of the block output;
//   pool_by_max=True -- F.adaptive_max_pool2d (nn/modules/convolution.py:499-503).
// Activations / activation gradients are bf16 [rows][ld] (row = b*H*W + pixel, channels innermost, ld >= C, 16-byte
// channel groups); pools, statistics and attention vectors stay fp32 and feed the fp32 twins unchanged
// (cn_sca_mlp_*_f32, the fp32 3x3 conv on [B][2][H][W]). Every sum runs in a fixed order: per block in LDS, then over
// the blocks by index in a second launch -- no float atomics, bit-reproducible run to run.
//
// Tie rules are those of the reference's ops on bf16 tensors:
//   H*W max (nn.AdaptiveMaxPool2d(1)) and the max-pool windows: ONE position gets the gradient -- the first maximum in
//     scan order; a NaN wins (ATen: val > max || isnan(val), so the last NaN);
//   channel max (einops.reduce 'max' = torch.amax): the gradient is split evenly across the tied channels.
#include "cn_bf16.h"
#include "cn_index.h"

// ---------------------------------------------------------------------------
// block tiling of the SCA passes: 256 threads = R pixel rows x G channel groups (G = C/8, R = 256/G, threads past R*G
// idle); a block walks SB_ITER such rows of pixels of ONE image, so it owns whole pixels (channel sums finish in LDS)
// and a slice of every channel's pixels (one partial row of C per block, summed over the blocks by the finisher).
// ---------------------------------------------------------------------------
#define SB_ITER 8
#define SB_MAXC 1024  // the channel MLPs (cn_sca_mlp_*_f32) take C <= 1024

static inline int sb_rows(int C) { return 256 / (C >> 3); }
static inline int sb_chunks(int C, int L) {
  const int pb = sb_rows(C) * SB_ITER;
  return (L + pb - 1) / pb;
}

// "a is a better H*W-max candidate than b": a NaN beats a number (the later NaN beats an earlier one), a larger value
// beats a smaller one, equal values go to the smaller index. idx < 0: no candidate.
__device__ __forceinline__ bool sb_better(float av, int ai, float bv, int bi) {
  if (bi < 0) return ai >= 0;
  if (ai < 0) return false;
  const bool an = av != av, bn = bv != bv;
  if (an || bn) return an && (!bn || ai > bi);
  if (av != bv) return av > bv;
  return ai < bi;
}

// ---- pool forward ---------------------------------------------------------------------------------------------------
// pooled[b][0][l] = mean_c x, pooled[b][1][l] = max_c x (fp32 NCHW, the 3x3 conv's input);
// per block: psum / pmax / pidx [b][chunk][C] = sum / max / argmax over the block's pixels of every channel.
__global__ __launch_bounds__(256) void cn_sca_pool_fwd_bf16_kernel(const bf16_t* __restrict__ x, long ldx, int C, int L,
                                                                  int nchunk, float* __restrict__ pooled,
                                                                  float* __restrict__ psum, float* __restrict__ pmax,
                                                                  int* __restrict__ pidx) {
  __shared__ float s_ps[SB_ITER * 256], s_pm[SB_ITER * 256];  // per (iteration, thread): 8-channel sum / max of a pixel
  __shared__ float s_cs[2048], s_cm[2048];                    // per (row r, channel): column partials, R * C <= 2048
  __shared__ int s_ci[2048];
  const int G = C >> 3, R = 256 / G;
  const int t = threadIdx.x, r = t / G, g = t - r * G;
  const bool act = r < R;
  const int chunk = blockIdx.x, b = blockIdx.y;
  const int l0 = chunk * R * SB_ITER;
  float cs[8], cm[8];
  int ci[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { cs[j] = 0.f; cm[j] = -INFINITY; ci[j] = -1; }
#pragma unroll 2
  for (int it = 0; it < SB_ITER; ++it) {
    const int l = l0 + it * R + r;
    float ps = 0.f, pm = -INFINITY;
    if (act && l < L) {
      float v[8];
      cn_unpack8(*reinterpret_cast<const u32x4*>(x + ((long)b * L + l) * ldx + g * 8), v);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        cs[j] += v[j];
        if (ci[j] < 0 || v[j] > cm[j] || v[j] != v[j]) { cm[j] = v[j]; ci[j] = l; }
        ps += v[j];
        pm = cn_max_nan(pm, v[j]);
      }
    }
    s_ps[it * 256 + t] = ps;
    s_pm[it * 256 + t] = pm;
  }
  if (act) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      s_cs[r * C + g * 8 + j] = cs[j];
      s_cm[r * C + g * 8 + j] = cm[j];
      s_ci[r * C + g * 8 + j] = ci[j];
    }
  }
  __syncthreads();
  for (int q = t; q < R * SB_ITER; q += 256) {  // pixel l0 + q = iteration q / R, row q % R
    const int l = l0 + q;
    if (l >= L) break;
    const float* ps = s_ps + (q / R) * 256 + (q % R) * G;
    const float* pm = s_pm + (q / R) * 256 + (q % R) * G;
    float s = 0.f, m = -INFINITY;
    for (int k = 0; k < G; ++k) {
      s += ps[k];
      m = cn_max_nan(m, pm[k]);
    }
    pooled[(long)b * 2 * L + l] = s / C;
    pooled[(long)b * 2 * L + L + l] = m;
  }
  for (int c = t; c < C; c += 256) {
    float s = 0.f, m = -INFINITY;
    int mi = -1;
    for (int k = 0; k < R; ++k) {
      s += s_cs[k * C + c];
      const float v = s_cm[k * C + c];
      const int vi = s_ci[k * C + c];
      if (sb_better(v, vi, m, mi)) { m = v; mi = vi; }
    }
    const long o = ((long)b * nchunk + chunk) * C + c;
    psum[o] = s;
    pmax[o] = m;
    pidx[o] = mi;
  }
}

// avg / mx / idx [b][c] from the per-block partials, blocks in index order
__global__ __launch_bounds__(256) void cn_sca_pool_finish_bf16_kernel(const float* __restrict__ psum,
                                                                     const float* __restrict__ pmax,
                                                                     const int* __restrict__ pidx, int C, int L,
                                                                     int nchunk, float* __restrict__ avg,
                                                                     float* __restrict__ mx, int* __restrict__ idx) {
  const int c = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (c >= C) return;
  float s = 0.f, m = -INFINITY;
  int mi = -1;
  for (int k = 0; k < nchunk; ++k) {
    const long o = ((long)b * nchunk + k) * C + c;
    s += psum[o];
    if (sb_better(pmax[o], pidx[o], m, mi)) { m = pmax[o]; mi = pidx[o]; }
  }
  avg[b * C + c] = s / L;
  mx[b * C + c] = m;
  idx[b * C + c] = mi;
}

// fp32 scratch of cn_sca_pool_fwd_bf16 / cn_sca_apply_bwd_bf16 (one buffer serves both)
extern "C" long cn_sca_workspace_floats_bf16(int B, int C, int L) {
  if (B <= 0 || C <= 0 || L <= 0 || (C & 7) || C > SB_MAXC) return 0;
  const long n = (long)B * sb_chunks(C, L);
  return 3 * n * C + n + B;
}

extern "C" int cn_sca_pool_fwd_bf16(const void* x, long ldx, int B, int C, int L, float* avg, float* mx, int* idx,
                                    float* pooled, float* ws, long ws_floats, void* stream) {
  if (B <= 0 || C <= 0 || L <= 0) return CN_OK;
  if ((C & 7) || C > SB_MAXC || ldx < C || B > 65535) return CN_ERR_ARG;
  const int nchunk = sb_chunks(C, L);
  const long n = (long)B * nchunk * C;
  if (ws_floats < cn_sca_workspace_floats_bf16(B, C, L)) return CN_ERR_ARG;
  float* psum = ws;
  float* pmax = ws + n;
  int* pidx = reinterpret_cast<int*>(ws + 2 * n);
  CN_LAUNCH(cn_sca_pool_fwd_bf16_kernel, dim3(nchunk, B), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx, C,
            L, nchunk, pooled, psum, pmax, pidx);
  CN_LAUNCH(cn_sca_pool_finish_bf16_kernel, dim3((C + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, psum, pmax,
            pidx, C, L, nchunk, avg, mx, idx);
  return cn_check_launch();
}

// ---- pool backward --------------------------------------------------------------------------------------------------
// dx[b,l,c] (+)= davg[b,c]/L + [l == idx[b,c]] dmx[b,c] + dpooled[b,0,l]/C + [x[b,l,c] == max_c x[b,l,:]] dpooled[b,1,l]/n
// (n = number of tied channels, recounted from x)
__global__ __launch_bounds__(256) void cn_sca_pool_bwd_bf16_kernel(const bf16_t* __restrict__ x, long ldx,
                                                                  const float* __restrict__ davg,
                                                                  const float* __restrict__ dmx,
                                                                  const int* __restrict__ idx,
                                                                  const float* __restrict__ dpooled,
                                                                  bf16_t* __restrict__ dx, long lddx, int C, int L,
                                                                  int accumulate) {
  __shared__ float s_pm[SB_ITER * 256], s_pn[SB_ITER * 256];  // per (iteration, thread): 8-channel max / tie count
  __shared__ float s_max[2048], s_dmax[2048], s_dmean[2048];   // per pixel of the block (R * SB_ITER <= 2048)
  const int G = C >> 3, R = 256 / G;
  const int t = threadIdx.x, r = t / G, g = t - r * G;
  const bool act = r < R;
  const int chunk = blockIdx.x, b = blockIdx.y;
  const int l0 = chunk * R * SB_ITER;
#pragma unroll 2
  for (int it = 0; it < SB_ITER; ++it) {
    const int l = l0 + it * R + r;
    float pm = -INFINITY, pn = 0.f;
    if (act && l < L) {
      float v[8];
      cn_unpack8(*reinterpret_cast<const u32x4*>(x + ((long)b * L + l) * ldx + g * 8), v);
#pragma unroll
      for (int j = 0; j < 8; ++j) pm = cn_max_nan(pm, v[j]);
#pragma unroll
      for (int j = 0; j < 8; ++j) pn += v[j] == pm ? 1.f : 0.f;
    }
    s_pm[it * 256 + t] = pm;
    s_pn[it * 256 + t] = pn;
  }
  __syncthreads();
  for (int q = t; q < R * SB_ITER; q += 256) {
    const int l = l0 + q;
    if (l >= L) break;
    const float* pm = s_pm + (q / R) * 256 + (q % R) * G;
    const float* pn = s_pn + (q / R) * 256 + (q % R) * G;
    float m = -INFINITY, n = 0.f;
    for (int k = 0; k < G; ++k) {
      if (pm[k] > m || pm[k] != pm[k]) { m = pm[k]; n = pn[k]; }
      else if (pm[k] == m) n += pn[k];
    }
    s_max[q] = m;
    s_dmax[q] = n > 0.f ? dpooled[(long)b * 2 * L + L + l] / n : 0.f;
    s_dmean[q] = dpooled[(long)b * 2 * L + l] / C;
  }
  __syncthreads();
  if (!act) return;
  float da[8], dm[8];
  int mi[8];
  const float invL = 1.f / L;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    da[j] = davg[b * C + g * 8 + j] * invL;
    dm[j] = dmx[b * C + g * 8 + j];
    mi[j] = idx[b * C + g * 8 + j];
  }
#pragma unroll 2
  for (int it = 0; it < SB_ITER; ++it) {  // x again: the block's pixels were read a moment ago (L2)
    const int q = it * R + r, l = l0 + q;
    if (l >= L) break;
    float v[8], o[8];
    cn_unpack8(*reinterpret_cast<const u32x4*>(x + ((long)b * L + l) * ldx + g * 8), v);
    const float m = s_max[q], dmax = s_dmax[q], dmean = s_dmean[q];
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = da[j] + (l == mi[j] ? dm[j] : 0.f) + dmean + (v[j] == m ? dmax : 0.f);
    bf16_t* dp = dx + ((long)b * L + l) * lddx + g * 8;
    if (accumulate) {
      float a[8];
      cn_unpack8(*reinterpret_cast<const u32x4*>(dp), a);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] += a[j];
    }
    *reinterpret_cast<u32x4*>(dp) = cn_pack8(o);
  }
}

extern "C" int cn_sca_pool_bwd_bf16(const void* x, long ldx, const float* davg, const float* dmx, const int* idx,
                                    const float* dpooled, void* dx, long lddx, int B, int C, int L, int accumulate,
                                    void* stream) {
  if (B <= 0 || C <= 0 || L <= 0) return CN_OK;
  if ((C & 7) || C > SB_MAXC || ldx < C || lddx < C || B > 65535) return CN_ERR_ARG;
  CN_LAUNCH(cn_sca_pool_bwd_bf16_kernel, dim3(sb_chunks(C, L), B), dim3(256), 0, (hipStream_t)stream,
            (const bf16_t*)x, ldx, davg, dmx, idx, dpooled, (bf16_t*)dx, lddx, C, L, accumulate);
  return cn_check_launch();
}

// ---- apply forward: y = out * (1 + gamma * 0.5 * (ca[b,c] + sigmoid(sconv[b,l]))) -----------------------------------
__global__ __launch_bounds__(256) void cn_sca_apply_fwd_bf16_kernel(const bf16_t* __restrict__ out, long ldo,
                                                                   const float* __restrict__ ca,
                                                                   const float* __restrict__ sconv,
                                                                   const float* __restrict__ gamma,
                                                                   bf16_t* __restrict__ y, long ldy, long P, int C,
                                                                   int L) {
  const int G = C >> 3;
  const float gg = 0.5f * gamma[0];
  const long n = P * G;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) {
    const long p = i / G;
    const int c0 = (int)(i - p * G) * 8;
    const long b = p / L;
    const float sa = cn_sigmoid(sconv[p]);
    const float4 a0 = *reinterpret_cast<const float4*>(ca + b * C + c0);
    const float4 a1 = *reinterpret_cast<const float4*>(ca + b * C + c0 + 4);
    const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
    float v[8];
    cn_unpack8(*reinterpret_cast<const u32x4*>(out + p * ldo + c0), v);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] *= 1.f + gg * (a[j] + sa);
    *reinterpret_cast<u32x4*>(y + p * ldy + c0) = cn_pack8(v);
  }
}

extern "C" int cn_sca_apply_fwd_bf16(const void* out, long ldo, const float* ca, const float* sconv,
                                     const float* gamma, void* y, long ldy, int B, int C, int L, void* stream) {
  if (B <= 0 || C <= 0 || L <= 0) return CN_OK;
  if ((C & 7) || ldo < C || ldy < C) return CN_ERR_ARG;
  const long P = (long)B * L;
  long blocks = (P * (C >> 3) + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  CN_LAUNCH(cn_sca_apply_fwd_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
            (const bf16_t*)out, ldo, ca, sconv, gamma, (bf16_t*)y, ldy, P, C, L);
  return cn_check_launch();
}

// ---- apply backward -------------------------------------------------------------------------------------------------
// With gg = gamma/2, sa = sigmoid(sconv), S[b,c] = sum_l dy out, T[b,l] = sum_c dy out:
//   dout (+)= dy (1 + gg (ca + sa));  dca = gg S;  dsconv = gg sa (1 - sa) T;
//   dgamma += 0.5 sum dy out (ca + sa) = 0.5 (sum_{b,c} ca S + sum_{b,l} sa T)
// Main pass (block per (chunk, b)): dout, dsconv, per-block rows pS[b][chunk][C] and pT[b][chunk] = sum_l sa T.
__global__ __launch_bounds__(256) void cn_sca_apply_bwd_bf16_kernel(const bf16_t* __restrict__ dy, long ldd,
                                                                   const bf16_t* __restrict__ out, long ldo,
                                                                   const float* __restrict__ ca,
                                                                   const float* __restrict__ sconv,
                                                                   const float* __restrict__ gamma,
                                                                   bf16_t* __restrict__ dout, long lddo, int accumulate,
                                                                   float* __restrict__ dsconv, float* __restrict__ pS,
                                                                   float* __restrict__ pT, int C, int L, int nchunk) {
  __shared__ float s_ps[SB_ITER * 256];  // per (iteration, thread): 8-channel sum of dy out of a pixel
  __shared__ float s_cs[2048];           // per (row r, channel): column partials of dy out
  __shared__ float s_red[4];
  const int G = C >> 3, R = 256 / G;
  const int t = threadIdx.x, r = t / G, g = t - r * G;
  const bool act = r < R;
  const int chunk = blockIdx.x, b = blockIdx.y;
  const int l0 = chunk * R * SB_ITER;
  const float gg = 0.5f * gamma[0];
  float a[8], cs[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    a[j] = act ? ca[b * C + g * 8 + j] : 0.f;
    cs[j] = 0.f;
  }
#pragma unroll 2
  for (int it = 0; it < SB_ITER; ++it) {
    const int l = l0 + it * R + r;
    float ps = 0.f;
    if (act && l < L) {
      const long p = (long)b * L + l;
      const float sa = cn_sigmoid(sconv[p]);
      float d[8], o[8];
      cn_unpack8(*reinterpret_cast<const u32x4*>(dy + p * ldd + g * 8), d);
      cn_unpack8(*reinterpret_cast<const u32x4*>(out + p * ldo + g * 8), o);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float pr = d[j] * o[j];
        cs[j] += pr;
        ps += pr;
        o[j] = d[j] * (1.f + gg * (a[j] + sa));
      }
      if (dout) {
        bf16_t* dp = dout + p * lddo + g * 8;
        if (accumulate) {
          float e[8];
          cn_unpack8(*reinterpret_cast<const u32x4*>(dp), e);
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] += e[j];
        }
        *reinterpret_cast<u32x4*>(dp) = cn_pack8(o);
      }
    }
    s_ps[it * 256 + t] = ps;
  }
  if (act) {
#pragma unroll
    for (int j = 0; j < 8; ++j) s_cs[r * C + g * 8 + j] = cs[j];
  }
  __syncthreads();
  float st = 0.f;
  for (int q = t; q < R * SB_ITER; q += 256) {
    const int l = l0 + q;
    if (l >= L) break;
    const float* ps = s_ps + (q / R) * 256 + (q % R) * G;
    float s = 0.f;
    for (int k = 0; k < G; ++k) s += ps[k];
    const long p = (long)b * L + l;
    const float sa = cn_sigmoid(sconv[p]);
    dsconv[p] = gg * sa * (1.f - sa) * s;
    st += sa * s;
  }
  for (int c = t; c < C; c += 256) {
    float s = 0.f;
    for (int k = 0; k < R; ++k) s += s_cs[k * C + c];
    pS[((long)b * nchunk + chunk) * C + c] = s;
  }
  st = cn_block_sum<float, 256>(st, s_red);
  if (t == 0) pT[(long)b * nchunk + chunk] = st;
}

// block per b: dca[b,c] = gg sum_chunk pS;  dgpart[b] = 0.5 (sum_c ca S + sum_chunk pT)
__global__ __launch_bounds__(256) void cn_sca_apply_bwd_finish_bf16_kernel(const float* __restrict__ pS,
                                                                          const float* __restrict__ pT,
                                                                          const float* __restrict__ ca,
                                                                          const float* __restrict__ gamma,
                                                                          float* __restrict__ dca,
                                                                          float* __restrict__ dgpart, int C,
                                                                          int nchunk) {
  __shared__ float s_red[4];
  const int b = blockIdx.x, t = threadIdx.x;
  const float gg = 0.5f * gamma[0];
  float acc = 0.f;
  for (int c = t; c < C; c += 256) {
    float s = 0.f;
    for (int k = 0; k < nchunk; ++k) s += pS[((long)b * nchunk + k) * C + c];
    dca[b * C + c] = gg * s;
    acc += ca[b * C + c] * s;
  }
  for (int k = t; k < nchunk; k += 256) acc += pT[(long)b * nchunk + k];
  acc = cn_block_sum<float, 256>(acc, s_red);
  if (t == 0) dgpart[b] = 0.5f * acc;
}

// dgamma[0] += sum_b dgpart[b] (one block, fixed order)
__global__ __launch_bounds__(256) void cn_sca_dgamma_bf16_kernel(const float* __restrict__ dgpart, int B,
                                                                float* __restrict__ dgamma) {
  __shared__ float s_red[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < B; i += 256) s += dgpart[i];
  s = cn_block_sum<float, 256>(s, s_red);
  if (threadIdx.x == 0) dgamma[0] += s;
}

// dout nullable (then only the attention gradients). dgamma is ACCUMULATED; dca / dsconv are overwritten.
// ws: cn_sca_workspace_floats_bf16(B, C, L) floats.
extern "C" int cn_sca_apply_bwd_bf16(const void* dy, long ldd, const void* out, long ldo, const float* ca,
                                     const float* sconv, const float* gamma, void* dout, long lddo,
                                     int accumulate_dout, float* dca, float* dsconv, float* dgamma, float* ws,
                                     long ws_floats, int B, int C, int L, void* stream) {
  if (B <= 0 || C <= 0 || L <= 0) return CN_OK;
  if ((C & 7) || C > SB_MAXC || ldd < C || ldo < C || (dout && lddo < C) || B > 65535) return CN_ERR_ARG;
  if (ws_floats < cn_sca_workspace_floats_bf16(B, C, L)) return CN_ERR_ARG;
  const int nchunk = sb_chunks(C, L);
  const long n = (long)B * nchunk;
  float* pS = ws;
  float* pT = ws + n * C;
  float* dgpart = pT + n;
  CN_LAUNCH(cn_sca_apply_bwd_bf16_kernel, dim3(nchunk, B), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dy, ldd,
            (const bf16_t*)out, ldo, ca, sconv, gamma, (bf16_t*)dout, lddo, accumulate_dout, dsconv, pS, pT, C, L,
            nchunk);
  CN_LAUNCH(cn_sca_apply_bwd_finish_bf16_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, pS, pT, ca, gamma, dca,
            dgpart, C, nchunk);
  CN_LAUNCH(cn_sca_dgamma_bf16_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, dgpart, B, dgamma);
  return cn_check_launch();
}

// ---------------------------------------------------------------------------
// F.adaptive_max_pool2d on bf16 NHWC. Window of output o along an axis: [cn_amp_start, cn_amp_end) (windows overlap
// when In % Out != 0). idx (nullable without backward): int32
// [B*Ho*Wo][C], the flat input pixel iy*Wi + ix of the first maximum in row-major window order (a NaN wins, as in
// ATen). Backward is a gather over the outputs whose windows can hold the input pixel: deterministic, no atomics.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cn_adaptive_maxpool_fwd_bf16_kernel(const bf16_t* __restrict__ x, long ldx,
                                                                          bf16_t* __restrict__ y, long ldy,
                                                                          int* __restrict__ idx, int B, int C, int Hi,
                                                                          int Wi, int Ho, int Wo) {
  const int G = C >> 3;
  const long n = (long)B * Ho * Wo * G;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) {
    const long po = i / G;
    const int c0 = (int)(i - po * G) * 8;
    const int b = (int)(po / ((long)Ho * Wo));
    const int op = (int)(po - (long)b * Ho * Wo);
    const int oy = op / Wo, ox = op - oy * Wo;
    const int y0 = cn_amp_start(oy, Hi, Ho), y1 = cn_amp_end(oy, Hi, Ho);
    const int x0 = cn_amp_start(ox, Wi, Wo), x1 = cn_amp_end(ox, Wi, Wo);
    const bf16_t* xb = x + (long)b * Hi * Wi * ldx + c0;
    float best[8];
    int bi[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { best[j] = -INFINITY; bi[j] = y0 * Wi + x0; }
    for (int iy = y0; iy < y1; ++iy)
      for (int ix = x0; ix < x1; ++ix) {
        const int p = iy * Wi + ix;
        float v[8];
        cn_unpack8(*reinterpret_cast<const u32x4*>(xb + (long)p * ldx), v);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (cn_max_takes(best[j], v[j])) { best[j] = v[j]; bi[j] = p; }
      }
    *reinterpret_cast<u32x4*>(y + po * ldy + c0) = cn_pack8(best);
    if (idx) {
      int4* ip = reinterpret_cast<int4*>(idx + po * C + c0);
      ip[0] = int4{bi[0], bi[1], bi[2], bi[3]};
      ip[1] = int4{bi[4], bi[5], bi[6], bi[7]};
    }
  }
}

__global__ __launch_bounds__(256) void cn_adaptive_maxpool_bwd_bf16_kernel(const bf16_t* __restrict__ dy, long ldd,
                                                                          const int* __restrict__ idx,
                                                                          bf16_t* __restrict__ dx, long lddx, int B,
                                                                          int C, int Hi, int Wi, int Ho, int Wo,
                                                                          int accumulate) {
  const int G = C >> 3;
  const long n = (long)B * Hi * Wi * G;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256L) {
    const long pi = i / G;
    const int c0 = (int)(i - pi * G) * 8;
    const int b = (int)(pi / ((long)Hi * Wi));
    const int p = (int)(pi - (long)b * Hi * Wi);
    const int iy = p / Wi, ix = p - iy * Wi;
    // outputs whose window can contain (iy, ix): start(o) <= i < end(o)
    const int oy_lo = max((int)(((long)iy * Ho) / Hi) - 1, 0);
    const int oy_hi = min((int)((((long)(iy + 1)) * Ho + Hi - 1) / Hi), Ho - 1);
    const int ox_lo = max((int)(((long)ix * Wo) / Wi) - 1, 0);
    const int ox_hi = min((int)((((long)(ix + 1)) * Wo + Wi - 1) / Wi), Wo - 1);
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int oy = oy_lo; oy <= oy_hi; ++oy)
      for (int ox = ox_lo; ox <= ox_hi; ++ox) {
        const long po = (long)b * Ho * Wo + oy * Wo + ox;
        const int4* ip = reinterpret_cast<const int4*>(idx + po * C + c0);
        const int4 i0 = ip[0], i1 = ip[1];
        const int m[8] = {i0.x, i0.y, i0.z, i0.w, i1.x, i1.y, i1.z, i1.w};
        float d[8];
        cn_unpack8(*reinterpret_cast<const u32x4*>(dy + po * ldd + c0), d);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += m[j] == p ? d[j] : 0.f;
      }
    bf16_t* o = dx + pi * lddx + c0;
    if (accumulate) {
      float e[8];
      cn_unpack8(*reinterpret_cast<const u32x4*>(o), e);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += e[j];
    }
    *reinterpret_cast<u32x4*>(o) = cn_pack8(acc);
  }
}

extern "C" int cn_adaptive_maxpool_fwd_bf16(const void* x, long ldx, void* y, long ldy, int* idx, int B, int C, int Hi,
                                            int Wi, int Ho, int Wo, void* stream) {
  if (B <= 0 || C <= 0 || Ho <= 0 || Wo <= 0) return CN_OK;
  if ((C & 7) || ldx < C || ldy < C || Hi <= 0 || Wi <= 0) return CN_ERR_ARG;
  const long n = (long)B * Ho * Wo * (C >> 3);
  long blocks = (n + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  CN_LAUNCH(cn_adaptive_maxpool_fwd_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
            (const bf16_t*)x, ldx, (bf16_t*)y, ldy, idx, B, C, Hi, Wi, Ho, Wo);
  return cn_check_launch();
}

extern "C" int cn_adaptive_maxpool_bwd_bf16(const void* dy, long ldd, const int* idx, void* dx, long lddx, int B, int C,
                                            int Hi, int Wi, int Ho, int Wo, int accumulate, void* stream) {
  if (B <= 0 || C <= 0 || Hi <= 0 || Wi <= 0) return CN_OK;
  if ((C & 7) || ldd < C || lddx < C || Ho <= 0 || Wo <= 0) return CN_ERR_ARG;
  const long n = (long)B * Hi * Wi * (C >> 3);
  long blocks = (n + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  CN_LAUNCH(cn_adaptive_maxpool_bwd_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
            (const bf16_t*)dy, ldd, idx, (bf16_t*)dx, lddx, B, C, Hi, Wi, Ho, Wo, accumulate);
  return cn_check_launch();
}
