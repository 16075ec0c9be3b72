// Neighborhood attention core (q.k over a clamped/dilated KxK window -> softmax -> .v) on NCHW
// planes, forward and backward. HBM/L2-bound; one lane per (pixel, head).
//
// Restates natten 0.17.1's unfused NA2D (na2d_qk -> softmax -> na2d_av, no rel-pos bias,
// non-causal) used at /root/reference/src/cultionet/nn/modules/convolution.py:341-350.
// The surrounding qkv / proj Linear layers run as 1x1 convolutions on the MFMA kernel
// (cn_conv.hip), so q,k,v arrive as channel blocks of one [B, 3C, H, W] tensor:
// channel of (which, head, d) = which*C + head*D + d  (== natten's reshape(B,H,W,3,heads,D)).
#include "cn_index.h"

#define NA_K CN_NA_K
#define NA_KK CN_NA_KK

// qkv [B][3C][H][W] (batch stride qbs); out [B][C][H][W]; attn [B][heads][9][H][W] (saved probs).
template <int D>
__global__ __launch_bounds__(256) void cn_na2d_fwd_kernel(const float* __restrict__ qkv, long qbs,
                                                         float* __restrict__ out, long obs,
                                                         float* __restrict__ attn, int B, int C, int heads, int H,
                                                         int W, int dil, float scale, unsigned long long dthresh,
                                                         float dscale, unsigned long long dseed_, const unsigned long long* __restrict__ dstep, int Dr) {
  const int DD = D > 0 ? D : Dr;  // D == 0: head dimension known at run time only (any width)
  const unsigned long long dseed = cn_step_seed(dseed_, dstep);
  const int HW = H * W;
  int bx, h, b;
  if (!cn_xcd_block((HW + 255) / 256, heads, ((HW + 255) / 256) * heads * B, bx, h, b)) return;
  const int p = bx * 256 + threadIdx.x;
  if (p >= HW) return;
  const int y = p / W, x = p - y * W;
  const int sy = cn_na_window_start(y, H, dil), sx = cn_na_window_start(x, W, dil);
  const float* qp = qkv + b * qbs + (long)(h * DD) * HW;
  const float* kp = qp + (long)C * HW;
  const float* vp = kp + (long)C * HW;
  // Loop order: channel plane outermost, the 9 taps inside. A tap-outer order revisits each of the D planes once
  // per tap with the other D-1 planes in between (reuse distance D * ~1.3 KB > the 32 KB L1): every tap then
  // misses to L2 and the kernel moves 9x the k / v bytes. Plane-outer touches a plane's few lines 9 times in a row.
  int kpix[NA_KK];
#pragma unroll
  for (int i = 0; i < NA_K; ++i)
#pragma unroll
    for (int j = 0; j < NA_K; ++j) kpix[i * NA_K + j] = (sy + i * dil) * W + sx + j * dil;
  float lg[NA_KK];
#pragma unroll
  for (int t = 0; t < NA_KK; ++t) lg[t] = 0.f;
#pragma unroll 4
  for (int d = 0; d < DD; ++d) {
    const float qd = qp[(long)d * HW + p] * scale;
    const float* kd = kp + (long)d * HW;
#pragma unroll
    for (int t = 0; t < NA_KK; ++t) lg[t] += qd * kd[kpix[t]];
  }
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < NA_KK; ++t) mx = fmaxf(mx, lg[t]);
  float den = 0.f;
#pragma unroll
  for (int t = 0; t < NA_KK; ++t) {
    lg[t] = expf(lg[t] - mx);
    den += lg[t];
  }
  const float inv = 1.0f / den;
  float* ap = attn + ((long)(b * heads + h) * NA_KK) * HW + p;
#pragma unroll
  for (int t = 0; t < NA_KK; ++t) {
    lg[t] *= inv;
    if (attn) ap[(long)t * HW] = lg[t];
    lg[t] *= cn_na_keep(dthresh, dscale, dseed, (long)b * heads + h, t, HW, p);
  }
  float* op = out + b * obs + (long)(h * DD) * HW + p;
#pragma unroll 4
  for (int d = 0; d < DD; ++d) {
    const float* vd = vp + (long)d * HW;
    float o = 0.f;
#pragma unroll
    for (int t = 0; t < NA_KK; ++t) o += lg[t] * vd[kpix[t]];
    op[(long)d * HW] = o;
  }
}

// Backward, query side: dP = dOut.v ; dS = P*(dP - sum P dP) ; dq = scale * sum dS*k ; saves dS.
template <int D>
__global__ __launch_bounds__(256) void cn_na2d_bwd_q_kernel(const float* __restrict__ qkv, long qbs,
                                                           const float* __restrict__ dout, long dobs,
                                                           const float* __restrict__ attn,
                                                           float* __restrict__ dattn, float* __restrict__ dqkv,
                                                           long dqbs, int B, int C, int heads, int H, int W, int dil,
                                                           float scale, unsigned long long dthresh, float dscale,
                                                           unsigned long long dseed_, const unsigned long long* __restrict__ dstep, int Dr) {
  const int DD = D > 0 ? D : Dr;  // D == 0: head dimension known at run time only (any width)
  const unsigned long long dseed = cn_step_seed(dseed_, dstep);
  const int HW = H * W;
  int bx, h, b;
  if (!cn_xcd_block((HW + 255) / 256, heads, ((HW + 255) / 256) * heads * B, bx, h, b)) return;
  const int p = bx * 256 + threadIdx.x;
  if (p >= HW) return;
  const int y = p / W, x = p - y * W;
  const int sy = cn_na_window_start(y, H, dil), sx = cn_na_window_start(x, W, dil);
  const float* kp = qkv + b * qbs + (long)(C + h * DD) * HW;
  const float* vp = kp + (long)C * HW;
  const float* dop = dout + b * dobs + (long)(h * DD) * HW + p;
  int kpix[NA_KK];
#pragma unroll
  for (int i = 0; i < NA_K; ++i)
#pragma unroll
    for (int j = 0; j < NA_K; ++j) kpix[i * NA_K + j] = (sy + i * dil) * W + sx + j * dil;
  const float* ap = attn + ((long)(b * heads + h) * NA_KK) * HW + p;
  float pr[NA_KK], dp[NA_KK];
#pragma unroll
  for (int t = 0; t < NA_KK; ++t) dp[t] = 0.f;
  // plane-outer (see the forward kernel): dP[t] = sum_d dOut[d] * v[d][tap t]
#pragma unroll 4
  for (int d = 0; d < DD; ++d) {
    const float gd = dop[(long)d * HW];
    const float* vd = vp + (long)d * HW;
#pragma unroll
    for (int t = 0; t < NA_KK; ++t) dp[t] += gd * vd[kpix[t]];
  }
  float dot = 0.f;
#pragma unroll
  for (int t = 0; t < NA_KK; ++t) {
    pr[t] = ap[(long)t * HW];
    dp[t] *= cn_na_keep(dthresh, dscale, dseed, (long)b * heads + h, t, HW, p);
    dot += pr[t] * dp[t];
  }
  float* dap = dattn + ((long)(b * heads + h) * NA_KK) * HW + p;
#pragma unroll
  for (int t = 0; t < NA_KK; ++t) {
    dp[t] = pr[t] * (dp[t] - dot);  // dS
    dap[(long)t * HW] = dp[t];
  }
  float* dqp = dqkv + b * dqbs + (long)(h * DD) * HW + p;
#pragma unroll 4
  for (int d = 0; d < DD; ++d) {
    const float* kd = kp + (long)d * HW;
    float dq = 0.f;
#pragma unroll
    for (int t = 0; t < NA_KK; ++t) dq += dp[t] * kd[kpix[t]];
    dqp[(long)d * HW] = dq * scale;
  }
}

// Backward, key side (gather form, deterministic): for key pixel (y,x) visit every query whose
// window contains it: dk = scale * sum dS[q,t]*q[q] ; dv = sum P[q,t]*dOut[q].
template <int D>
__global__ __launch_bounds__(256) void cn_na2d_bwd_kv_kernel(const float* __restrict__ qkv, long qbs,
                                                            const float* __restrict__ dout, long dobs,
                                                            const float* __restrict__ attn,
                                                            const float* __restrict__ dattn,
                                                            float* __restrict__ dqkv, long dqbs, int B, int C,
                                                            int heads, int H, int W, int dil, float scale,
                                                            unsigned long long dthresh, float dscale,
                                                            unsigned long long dseed_, const unsigned long long* __restrict__ dstep, int Dr) {
  const int DD = D > 0 ? D : Dr;  // D == 0: head dimension known at run time only (any width)
  const unsigned long long dseed = cn_step_seed(dseed_, dstep);
  const int HW = H * W;
  int bx, h, b;
  if (!cn_xcd_block((HW + 255) / 256, heads, ((HW + 255) / 256) * heads * B, bx, h, b)) return;
  const int p = bx * 256 + threadIdx.x;
  if (p >= HW) return;
  const int y = p / W, x = p - y * W;
  const float* qp = qkv + b * qbs + (long)(h * DD) * HW;
  const float* dop = dout + b * dobs + (long)(h * DD) * HW;
  const float* ap = attn + ((long)(b * heads + h) * NA_KK) * HW;
  const float* dap = dattn + ((long)(b * heads + h) * NA_KK) * HW;
  // CH channels of the head at a time: all D of them when D is a compile-time constant, eight per sweep of the window
  // for a run-time head dimension (D == 0)
  constexpr int CH = D > 0 ? D : 8;
  float* dkp = dqkv + b * dqbs + (long)(C + h * DD) * HW + p;
  float* dvp = dkp + (long)C * HW;
  for (int d0 = 0; d0 < DD; d0 += CH) {
    float dk[CH], dv[CH];
#pragma unroll
    for (int d = 0; d < CH; ++d) {
      dk[d] = 0.f;
      dv[d] = 0.f;
    }
    for (int my = -2; my <= 2; ++my) {
      const int qy = y + my * dil;
      if (qy < 0 || qy >= H) continue;
      const int offy = y - cn_na_window_start(qy, H, dil);
      if (offy < 0 || offy > 2 * dil) continue;  // same residue class => divisible by dil
      const int i = offy / dil;
      for (int mx = -2; mx <= 2; ++mx) {
        const int qx = x + mx * dil;
        if (qx < 0 || qx >= W) continue;
        const int offx = x - cn_na_window_start(qx, W, dil);
        if (offx < 0 || offx > 2 * dil) continue;
        const int t = i * NA_K + offx / dil;
        const int qpix = qy * W + qx;
        const float ds = dap[(long)t * HW + qpix];
        const float pr = ap[(long)t * HW + qpix] * cn_na_keep(dthresh, dscale, dseed, (long)b * heads + h, t, HW, qpix);
#pragma unroll
        for (int d = 0; d < CH; ++d) {
          if (D > 0 || d0 + d < DD) {
            dk[d] += ds * qp[(long)(d0 + d) * HW + qpix];
            dv[d] += pr * dop[(long)(d0 + d) * HW + qpix];
          }
        }
      }
    }
#pragma unroll
    for (int d = 0; d < CH; ++d) {
      if (D > 0 || d0 + d < DD) {
        dkp[(long)(d0 + d) * HW] = dk[d] * scale;
        dvp[(long)(d0 + d) * HW] = dv[d];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Tiled kernels for the head dimensions of training (D = 16, 32). The kernels above give a lane one (pixel, head) and
// gather every tap from global memory: 19 * D dword loads per lane forward, each k and v element fetched nine times
// through L1, 1.0 - 1.7 TB/s of algorithmic bytes. Here a block of 256 lanes owns a strip of whole rows of one
// (batch, head): NAT_PPT pixels per lane, R rows with R * W <= 256 * NAT_PPT. By cn_na_window_start every tap of a
// row lies within 2 * dilation rows of it, so the taps of a strip live in a run of whole rows [lo, hi] of the plane:
// one CONTIGUOUS range of each channel plane. nat_stage copies that range for NAT_CH channels at a time into LDS
// (16-byte loads where the planes allow them, dword loads for a 25 x 25 plane or an odd batch stride), and the nine
// taps come out of LDS at consecutive addresses in consecutive lanes. q,
// dOut, out, dq, the probabilities and dS move once, coalesced. Consecutive blocks are neighbouring strips of one
// plane on one XCD (cn_xcd_block): the halo rows a strip shares with the next come from that L2.
// Every sum runs over the same terms in the same order as in the kernels above: the saved probabilities and dS come
// out bit for bit the same, out and dq agree with them to the last bit or two (at most 7e-7 on unit-variance inputs;
// the compiler contracts the nine-term sums differently). attn == nullptr changes no arithmetic.
#define NAT_THREADS 256
#define NAT_PPT 2  // pixels per lane
#define NAT_CH 8   // channels of a head staged at a time

extern __shared__ float nat_lds[];

// lds[c * n + e] = plane(c0 + c)[e0 + e] for c < NAT_CH, e < n; src points at element e0 of channel c0's plane.
// 16-byte loads when every channel's run starts on a 16-byte boundary and is whole float4s long (HW and n multiples
// of 4: the 100 x 100 and 50 x 50 planes with dense or 16-byte-padded batch strides), dword loads otherwise.
__device__ __forceinline__ void nat_stage(float* __restrict__ lds, const float* __restrict__ src, int HW, int n) {
  if (((reinterpret_cast<uintptr_t>(src) & 15) | ((HW | n) & 3)) == 0) {
    const int n4 = n >> 2, HW4 = HW >> 2;
    const float4* sp = reinterpret_cast<const float4*>(src);
    for (int v = threadIdx.x; v < n4; v += NAT_THREADS) {
      float4 x[NAT_CH];
#pragma unroll
      for (int c = 0; c < NAT_CH; ++c) x[c] = sp[(long)c * HW4 + v];
#pragma unroll
      for (int c = 0; c < NAT_CH; ++c) *reinterpret_cast<float4*>(lds + c * n + 4 * v) = x[c];
    }
    return;
  }
  for (int e = threadIdx.x; e < n; e += NAT_THREADS) {
    float x[NAT_CH];
#pragma unroll
    for (int c = 0; c < NAT_CH; ++c) x[c] = src[(long)c * HW + e];
#pragma unroll
    for (int c = 0; c < NAT_CH; ++c) lds[c * n + e] = x[c];
  }
}

// A block's strip of query rows [y0, y1) and the rows [lo, hi] that hold all their taps.
struct NatStrip {
  int h, b, y0, y1, lo, hi;
};

__device__ __forceinline__ bool nat_strip(int R, int heads, int B, int H, int dil, NatStrip& s) {
  const int nstrips = (H + R - 1) / R;
  int sx;
  if (!cn_xcd_block(nstrips, heads, nstrips * heads * B, sx, s.h, s.b)) return false;
  s.y0 = sx * R;
  s.y1 = min(H, s.y0 + R);
  s.lo = H;
  s.hi = 0;
  for (int y = s.y0; y < s.y1; ++y) {
    const int w0 = cn_na_window_start(y, H, dil);
    s.lo = min(s.lo, w0);
    s.hi = max(s.hi, w0 + 2 * dil);
  }
  return true;
}

// Pixel j of this lane: e = lane + j * 256 within the strip (dead lanes compute pixel 0 of the strip and store nothing);
// p its index in the plane, base the LDS offset of its tap (0, 0).
__device__ __forceinline__ void nat_pixel(const NatStrip& s, int j, int H, int W, int dil, bool& live, int& p, int& base) {
  const int e = threadIdx.x + j * NAT_THREADS;
  live = e < (s.y1 - s.y0) * W;
  p = s.y0 * W + (live ? e : 0);
  const int y = p / W, x = p - y * W;
  base = (cn_na_window_start(y, H, dil) - s.lo) * W + cn_na_window_start(x, W, dil);
}

template <int D>
__global__ __launch_bounds__(NAT_THREADS) void cn_na2d_fwd_tiled_kernel(
    const float* __restrict__ qkv, long qbs, float* __restrict__ out, long obs, float* __restrict__ attn, int B, int C,
    int heads, int H, int W, int dil, float scale, unsigned long long dthresh, float dscale, unsigned long long dseed_,
    const unsigned long long* __restrict__ dstep, int R) {
  static_assert(D % NAT_CH == 0, "whole chunks");
  const unsigned long long dseed = cn_step_seed(dseed_, dstep);
  const int HW = H * W;
  NatStrip s;
  if (!nat_strip(R, heads, B, H, dil, s)) return;
  const int h = s.h, b = s.b;
  const int n = (s.hi - s.lo + 1) * W;
  const int npx = (s.y1 - s.y0) * W;
  const float* qp = qkv + b * qbs + (long)(h * D) * HW;
  const float* kp = qp + (long)C * HW + s.lo * W;
  const float* vp = kp + (long)C * HW;
  bool live[NAT_PPT];
  int p[NAT_PPT], base[NAT_PPT];
  float lg[NAT_PPT][NA_KK];
#pragma unroll
  for (int j = 0; j < NAT_PPT; ++j) {
    nat_pixel(s, j, H, W, dil, live[j], p[j], base[j]);
#pragma unroll
    for (int t = 0; t < NA_KK; ++t) lg[j][t] = 0.f;
  }
#pragma unroll 1
  for (int c0 = 0; c0 < D; c0 += NAT_CH) {
    if (c0) __syncthreads();
    nat_stage(nat_lds, kp + (long)c0 * HW, HW, n);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NAT_PPT; ++j) {
      if (npx <= j * NAT_THREADS) break;  // a short strip: no lane has a pixel j
#pragma unroll 2
      for (int c = 0; c < NAT_CH; ++c) {
        const float qd = qp[(long)(c0 + c) * HW + p[j]] * scale;
        const float* kd = nat_lds + c * n + base[j];
#pragma unroll
        for (int t = 0; t < NA_KK; ++t) lg[j][t] += qd * kd[(t / NA_K) * dil * W + (t % NA_K) * dil];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NAT_PPT; ++j) {
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < NA_KK; ++t) mx = fmaxf(mx, lg[j][t]);
    float den = 0.f;
#pragma unroll
    for (int t = 0; t < NA_KK; ++t) {
      lg[j][t] = expf(lg[j][t] - mx);
      den += lg[j][t];
    }
    const float inv = 1.0f / den;
    float* ap = attn + ((long)(b * heads + h) * NA_KK) * HW + p[j];
#pragma unroll
    for (int t = 0; t < NA_KK; ++t) {
      lg[j][t] *= inv;
      if (attn && live[j]) ap[(long)t * HW] = lg[j][t];
      lg[j][t] *= cn_na_keep(dthresh, dscale, dseed, (long)b * heads + h, t, HW, p[j]);
    }
  }
  float* op = out + b * obs + (long)(h * D) * HW;
#pragma unroll 1
  for (int c0 = 0; c0 < D; c0 += NAT_CH) {
    __syncthreads();
    nat_stage(nat_lds, vp + (long)c0 * HW, HW, n);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NAT_PPT; ++j) {
      if (npx <= j * NAT_THREADS) break;  // a short strip: no lane has a pixel j
#pragma unroll 2
      for (int c = 0; c < NAT_CH; ++c) {
        const float* vd = nat_lds + c * n + base[j];
        float o = 0.f;
#pragma unroll
        for (int t = 0; t < NA_KK; ++t) o += lg[j][t] * vd[(t / NA_K) * dil * W + (t % NA_K) * dil];
        if (live[j]) op[(long)(c0 + c) * HW + p[j]] = o;
      }
    }
  }
}

// Query side of the backward: the strip's rows of v, then of k, as in the forward.
template <int D>
__global__ __launch_bounds__(NAT_THREADS) void cn_na2d_bwd_q_tiled_kernel(
    const float* __restrict__ qkv, long qbs, const float* __restrict__ dout, long dobs, const float* __restrict__ attn,
    float* __restrict__ dattn, float* __restrict__ dqkv, long dqbs, int B, int C, int heads, int H, int W, int dil,
    float scale, unsigned long long dthresh, float dscale, unsigned long long dseed_,
    const unsigned long long* __restrict__ dstep, int R) {
  static_assert(D % NAT_CH == 0, "whole chunks");
  const unsigned long long dseed = cn_step_seed(dseed_, dstep);
  const int HW = H * W;
  NatStrip s;
  if (!nat_strip(R, heads, B, H, dil, s)) return;
  const int h = s.h, b = s.b;
  const int n = (s.hi - s.lo + 1) * W;
  const int npx = (s.y1 - s.y0) * W;
  const float* kp = qkv + b * qbs + (long)(C + h * D) * HW + s.lo * W;
  const float* vp = kp + (long)C * HW;
  const float* dop = dout + b * dobs + (long)(h * D) * HW;
  bool live[NAT_PPT];
  int p[NAT_PPT], base[NAT_PPT];
  float dp[NAT_PPT][NA_KK];
#pragma unroll
  for (int j = 0; j < NAT_PPT; ++j) {
    nat_pixel(s, j, H, W, dil, live[j], p[j], base[j]);
#pragma unroll
    for (int t = 0; t < NA_KK; ++t) dp[j][t] = 0.f;
  }
#pragma unroll 1
  for (int c0 = 0; c0 < D; c0 += NAT_CH) {
    if (c0) __syncthreads();
    nat_stage(nat_lds, vp + (long)c0 * HW, HW, n);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NAT_PPT; ++j) {
      if (npx <= j * NAT_THREADS) break;  // a short strip: no lane has a pixel j
#pragma unroll 2
      for (int c = 0; c < NAT_CH; ++c) {
        const float gd = dop[(long)(c0 + c) * HW + p[j]];
        const float* vd = nat_lds + c * n + base[j];
#pragma unroll
        for (int t = 0; t < NA_KK; ++t) dp[j][t] += gd * vd[(t / NA_K) * dil * W + (t % NA_K) * dil];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NAT_PPT; ++j) {
    const float* ap = attn + ((long)(b * heads + h) * NA_KK) * HW + p[j];
    float pr[NA_KK];
    float dot = 0.f;
#pragma unroll
    for (int t = 0; t < NA_KK; ++t) {
      pr[t] = ap[(long)t * HW];
      dp[j][t] *= cn_na_keep(dthresh, dscale, dseed, (long)b * heads + h, t, HW, p[j]);
      dot += pr[t] * dp[j][t];
    }
    float* dap = dattn + ((long)(b * heads + h) * NA_KK) * HW + p[j];
#pragma unroll
    for (int t = 0; t < NA_KK; ++t) {
      dp[j][t] = pr[t] * (dp[j][t] - dot);  // dS
      if (live[j]) dap[(long)t * HW] = dp[j][t];
    }
  }
  float* dqp = dqkv + b * dqbs + (long)(h * D) * HW;
#pragma unroll 1
  for (int c0 = 0; c0 < D; c0 += NAT_CH) {
    __syncthreads();
    nat_stage(nat_lds, kp + (long)c0 * HW, HW, n);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NAT_PPT; ++j) {
      if (npx <= j * NAT_THREADS) break;  // a short strip: no lane has a pixel j
#pragma unroll 2
      for (int c = 0; c < NAT_CH; ++c) {
        const float* kd = nat_lds + c * n + base[j];
        float dq = 0.f;
#pragma unroll
        for (int t = 0; t < NA_KK; ++t) dq += dp[j][t] * kd[(t / NA_K) * dil * W + (t % NA_K) * dil];
        if (live[j]) dqp[(long)(c0 + c) * HW + p[j]] = dq * scale;
      }
    }
  }
}

// The key side of the backward stays on cn_na2d_bwd_kv_kernel. A tiled form of it (a strip of key rows per block, q and
// dOut staged NAT_CH channels at a time, the dS / P coefficient of each of the 25 candidate queries read from global
// memory inside the candidate loop) was slower alone at every site, 114 / 48 / 26 us against 108 / 29 / 15 us at
// 100 x 100 / 50 x 50 / 25 x 25: each coefficient load waits for the one before it. Fetching a pass's coefficients
// at once needs them in registers across the chunk loop; with two pixels per lane that form did not fit the register
// file (430 registers, 1.2 KB of scratch when capped at 128).
//
// Rows per block of the tiled kernels, or 0 for the one-lane-per-(pixel, head) kernels. Tiled: D = 16 or 32 (the heads
// of the reference's training widths at hidden 32), rows that fit a block (W <= 256), a plane of at least NAT_MIN_PIXELS
// pixels, and NAT_CH channels of R + 4 * dilation rows within 64 KiB of LDS. R: as many whole rows as a block's
// 256 * NAT_PPT pixels hold, halved while that leaves fewer than two blocks for each of the 256 CUs and still a pixel
// for three lanes in four.
#define NAT_MIN_PIXELS 512
static int na_tile_rows(int B, int heads, int D, int H, int W, int dil) {
  if ((D != 16 && D != 32) || W > 256 || (long)H * W < NAT_MIN_PIXELS) return 0;
  int R = min(H, NAT_THREADS * NAT_PPT / W);
  while (R > 1 && (long)((H + R - 1) / R) * heads * B < 512 && ((R + 1) / 2) * W >= NAT_THREADS * 3 / 4) R = (R + 1) / 2;
  if ((long)NAT_CH * min(H, R + 4 * dil) * W * sizeof(float) > 65536) return 0;
  return R;
}
static size_t na_tile_lds(int H, int W, int dil, int R) { return (size_t)NAT_CH * min(H, R + 4 * dil) * W * sizeof(float); }

#define NAT_DISPATCH(D_, KERNEL, ...)                                                                      \
  if (D_ == 32) CN_LAUNCH((KERNEL<32>), tgrid, dim3(NAT_THREADS), tlds, stream, __VA_ARGS__, R);           \
  else CN_LAUNCH((KERNEL<16>), tgrid, dim3(NAT_THREADS), tlds, stream, __VA_ARGS__, R)

// Head dimensions of the reference's widths (hidden 8 .. 128: h/4, h/2, h for powers of two) are compiled in; any other
// width (hidden 24, 40, 48, 96 ...) runs the same kernels with the head dimension as a run-time loop bound (D = 0).
#define NA_DISPATCH(D_, KERNEL, ...)                                                                          \
  switch (D_) {                                                                                               \
    case 2: CN_LAUNCH((KERNEL<2>), grid, dim3(256), 0, stream, __VA_ARGS__, D_); break;             \
    case 4: CN_LAUNCH((KERNEL<4>), grid, dim3(256), 0, stream, __VA_ARGS__, D_); break;             \
    case 8: CN_LAUNCH((KERNEL<8>), grid, dim3(256), 0, stream, __VA_ARGS__, D_); break;             \
    case 16: CN_LAUNCH((KERNEL<16>), grid, dim3(256), 0, stream, __VA_ARGS__, D_); break;           \
    case 32: CN_LAUNCH((KERNEL<32>), grid, dim3(256), 0, stream, __VA_ARGS__, D_); break;           \
    case 64: CN_LAUNCH((KERNEL<64>), grid, dim3(256), 0, stream, __VA_ARGS__, D_); break;           \
    default: CN_LAUNCH((KERNEL<0>), grid, dim3(256), 0, stream, __VA_ARGS__, D_); break;            \
  }

// kernel_size must be 3 (every NATTEN_PARAMS entry used by TowerUNet: unet_parts.py:19-40).
extern "C" int cn_na2d_fwd_f32(const float* qkv, long qbs, float* out, long obs, float* attn, int B, int C,
                               int heads, int H, int W, int kernel_size, int dilation, float attn_drop,
                               unsigned long long seed, const unsigned long long* step, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (kernel_size != NA_K || heads <= 0 || C % heads != 0) return CN_ERR_ARG;
  if (kernel_size * dilation > H || kernel_size * dilation > W) return CN_ERR_ARG;
  const int D = C / heads;
  const float scale = 1.0f / sqrtf((float)D);
  dim3 grid(cn_xcd_grid((long)((H * W + 255) / 256) * heads * B));  // XCD-aware order, decoded in the kernels
  if (!(attn_drop >= 0.f && attn_drop < 1.f)) return CN_ERR_ARG;
  const int R = na_tile_rows(B, heads, D, H, W, dilation);
  if (R > 0) {
    const dim3 tgrid(cn_xcd_grid((long)((H + R - 1) / R) * heads * B));
    const size_t tlds = na_tile_lds(H, W, dilation, R);
    NAT_DISPATCH(D, cn_na2d_fwd_tiled_kernel, qkv, qbs, out, obs, attn, B, C, heads, H, W, dilation, scale,
                 cn_dropout_thresh(attn_drop), 1.0f / (1.0f - attn_drop), seed, step);
    return cn_check_launch();
  }
  NA_DISPATCH(D, cn_na2d_fwd_kernel, qkv, qbs, out, obs, attn, B, C, heads, H, W, dilation, scale,
              cn_dropout_thresh(attn_drop), 1.0f / (1.0f - attn_drop), seed, step);
  return cn_check_launch();
}

// dqkv [B][3C][H][W] is fully overwritten (dq, dk, dv); dattn is scratch of attn's size.
extern "C" int cn_na2d_bwd_f32(const float* qkv, long qbs, const float* dout, long dobs, const float* attn,
                               float* dattn, float* dqkv, long dqbs, int B, int C, int heads, int H, int W,
                               int kernel_size, int dilation, float attn_drop, unsigned long long seed,
                               const unsigned long long* step, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (kernel_size != NA_K || heads <= 0 || C % heads != 0) return CN_ERR_ARG;
  const int D = C / heads;
  const float scale = 1.0f / sqrtf((float)D);
  dim3 grid(cn_xcd_grid((long)((H * W + 255) / 256) * heads * B));  // XCD-aware order, decoded in the kernels
  if (!(attn_drop >= 0.f && attn_drop < 1.f)) return CN_ERR_ARG;
  const unsigned long long th = cn_dropout_thresh(attn_drop);
  const float ds = 1.0f / (1.0f - attn_drop);
  const int R = na_tile_rows(B, heads, D, H, W, dilation);
  if (R > 0) {
    const dim3 tgrid(cn_xcd_grid((long)((H + R - 1) / R) * heads * B));
    const size_t tlds = na_tile_lds(H, W, dilation, R);
    NAT_DISPATCH(D, cn_na2d_bwd_q_tiled_kernel, qkv, qbs, dout, dobs, attn, dattn, dqkv, dqbs, B, C, heads, H, W,
                 dilation, scale, th, ds, seed, step);
  } else {
    NA_DISPATCH(D, cn_na2d_bwd_q_kernel, qkv, qbs, dout, dobs, attn, dattn, dqkv, dqbs, B, C, heads, H, W, dilation,
                scale, th, ds, seed, step);
  }
  // the key side has no tiled kernel (see the note above na_tile_rows)
  NA_DISPATCH(D, cn_na2d_bwd_kv_kernel, qkv, qbs, dout, dobs, attn, dattn, dqkv, dqbs, B, C, heads, H, W, dilation,
              scale, th, ds, seed, step);
  return cn_check_launch();
}
