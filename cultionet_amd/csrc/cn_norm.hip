// BatchNorm (train / eval) with fused SiLU + residual add, LayerNorm over the channel axis
// of NCHW tensors, and per-channel sums. HBM-bound streaming kernels (gfx950).
//
// Reference ops: nn.BatchNorm2d / BatchNorm3d + SiLU inside ConvBlock2d
// (cultionet/nn/modules/convolution.py:71-120, models/nunet.py:18-57),
// nn.LayerNorm over channels in NHWC (nunet.py:93-97, convolution.py:338-353).
// Here tensors stay NCHW: a LayerNorm "row" is the C values of one pixel (stride L),
// lanes walk consecutive pixels so every access is coalesced.
//
// fp32 BatchNorm: the single-tensor and the grouped entry points fill one argument block (CnBnGroupArgs, G = 1 for a
// single call) and share every kernel: the resident ones (one launch per pass, a channel in the registers of a block)
// and, for the channels that fit no block, the two-pass family cn_bn_group_* (partial sums in fp64 through the
// workspace, then an apply launch whose blocks reduce their channel's rows themselves). The entry points differ in the
// number of partial rows only: bn_splits_wide for a single call, bn_splits for a grouped one.
#include "cn_common.h"

#include <initializer_list>

#define BN_SPLIT_MAX 256  // workspace rows per channel
#define BN_SPLIT_GROUP 64 // cap of the grouped calls and the channel sums

#define BN_SERIAL_ROWS 8  // up to here every thread adds the partial rows itself

// Sum of a channel's `splits` partial pairs (rows: [splits][2]); every thread returns the totals, the same bits in
// every thread of every block of the channel. Few rows (the wide launches: 2 x 128 channels at 100 x 100 have 4): each
// thread walks them, block-uniform loads and no cross-lane traffic in a block that then touches ~1000 elements. More
// (up to BN_SPLIT_MAX): every wave sums them itself, lane t taking rows t, t + 64, ... -- no barrier and no LDS.
__device__ __forceinline__ void cn_bn_sum_parts(const double* __restrict__ rows, int splits, double& s, double& ss) {
  double a = 0.0, b = 0.0;
  if (splits <= BN_SERIAL_ROWS) {
    for (int i = 0; i < splits; ++i) {
      a += rows[2 * i];
      b += rows[2 * i + 1];
    }
    s = a;
    ss = b;
    return;
  }
  for (int i = threadIdx.x & 63; i < splits; i += 64) {
    a += rows[2 * i];
    b += rows[2 * i + 1];
  }
  s = cn_wave_sum(a);
  ss = cn_wave_sum(b);
}

// Single BatchNorm with few channels (BatchNorm3d of the time reduction: C = 3 channels of 3.2M elements at batch 32
// were 192 blocks on 256 CUs, ~2 TB/s): up to 256 splits per channel, summed by every wave of the apply kernels (cn_bn_sum_parts).
static int bn_splits_wide(int C, long L) {
  int s = (2048 + C - 1) / C;
  const long maxs = (L + 511) / 512;
  if (s > maxs) s = (int)maxs;
  if (s > BN_SPLIT_MAX) s = BN_SPLIT_MAX;
  if (s < 1) s = 1;
  return s;
}

static int bn_splits(int C, long L) {
  int s = (1024 + C - 1) / C;
  const long maxs = (L + 511) / 512;
  if (s > maxs) s = (int)maxs;
  if (s > BN_SPLIT_GROUP) s = BN_SPLIT_GROUP;
  if (s < 1) s = 1;
  return s;
}

static dim3 plane_grid(int B, int C, int L) {
  int bx = (L + 1023) / 1024;  // ~4 elements per thread
  if (bx < 1) bx = 1;
  return dim3(bx, C, B);
}

extern "C" int cn_bn_workspace_doubles(int C) { return C * BN_SPLIT_MAX * 2; }

// ---------------------------------------------------------------------------
// Grouped BatchNorm (+ SiLU): G (<= 4) BatchNorm layers over G same-shaped tensors in one launch (pair) -- the
// dilation branches of ResidualAConv (convolution.py:376-395). sum_outputs != 0 fuses the ResUNet-a sum
//   y = res + sum_g act(bn_g(x_g))
// into the one normalisation pass (the sequential form re-reads and re-writes the running sum once per branch).
// The single-tensor entry points fill the same argument block with G = 1 (bn_single_args), the residual as the sum.
// ---------------------------------------------------------------------------
#define BN_MAX_GROUPS 4
struct CnBnGroupArgs {
  const float* x[BN_MAX_GROUPS];
  const float* gamma[BN_MAX_GROUPS];
  const float* beta[BN_MAX_GROUPS];
  float* mean[BN_MAX_GROUPS];
  float* rstd[BN_MAX_GROUPS];
  float* running_mean[BN_MAX_GROUPS];
  float* running_var[BN_MAX_GROUPS];
  float* y[BN_MAX_GROUPS];         // forward outputs (sum mode: y[0] only)
  const float* dy[BN_MAX_GROUPS];  // backward: output gradients (sum mode: all the same pointer)
  float* dx[BN_MAX_GROUPS];
  float* dgamma[BN_MAX_GROUPS];
  float* dbeta[BN_MAX_GROUPS];
  int accumulate_dx[BN_MAX_GROUPS];
  long xbs, ybs, dybs, dxbs, rbs;
  const float* res;
  int G, B, C, L, act, splits, training, sum_outputs, accumulate_params;
  int vec4;  // L % 4 == 0 and every plane the pass touches 16-byte aligned => float4 accesses
  float eps, momentum;
  double* part;  // [G][C][splits][2]
};

// ---------------------------------------------------------------------------
// Resident BatchNorm: ONE launch per pass. A block owns channel c of one group (GS == 1, grid = (C, G)) or, in the
// summed forward, of all GS = G groups (grid = (C)). It issues all its loads up front, keeps the channel's B*L values in registers (NV units of 16 bytes, or of one dword
// where a plane is not 16-byte aligned, per thread and tensor), sums in fp64 like the two-pass kernels, reduces across
// the block and applies from the registers: x (and dy) are read once, no partial sums go through memory and the second,
// dependent launch is gone. No block waits for another one: a channel that does not fit one block stays two-pass.
// ---------------------------------------------------------------------------
#define BN_RES_CHUNK 4  // units of the residual / the old dx fetched ahead of their stores
template <bool V4> struct CnBnUnit { typedef float type; };
template <> struct CnBnUnit<true> { typedef float4 type; };

__device__ __forceinline__ void cn_bn_clear(float& v) { v = 0.f; }
__device__ __forceinline__ void cn_bn_clear(float4& v) { v.x = v.y = v.z = v.w = 0.f; }
__device__ __forceinline__ void cn_bn_stat(float v, double& s, double& ss) {
  s += v;
  ss += (double)v * v;
}
__device__ __forceinline__ void cn_bn_stat(const float4& v, double& s, double& ss) {
  s += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
  ss += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
}
template <class F> __device__ __forceinline__ float cn_bn_map(float a, float b, F f) { return f(a, b); }
template <class F> __device__ __forceinline__ float4 cn_bn_map(const float4& a, const float4& b, F f) {
  float4 r;
  r.x = f(a.x, b.x); r.y = f(a.y, b.y); r.z = f(a.z, b.z); r.w = f(a.w, b.w);
  return r;
}

// Both sums of a thread through one pair of barriers; every thread returns the block's totals. The empty asm pins the
// two sums in front of the barrier: without it the compiler finished the second sum behind the first reduction and
// held every value's double in registers until then (that spilled).
template <int NT>
__device__ __forceinline__ void cn_bn_block_sum2(double& a, double& b, double* scratch) {
  asm volatile("" : "+v"(a), "+v"(b));
  a = cn_wave_sum(a);
  b = cn_wave_sum(b);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) {
    scratch[2 * wid] = a;
    scratch[2 * wid + 1] = b;
  }
  __syncthreads();
  a = b = 0.0;
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) {
    a += scratch[2 * i];
    b += scratch[2 * i + 1];
  }
}

// Unit i = t + k * T of a channel of B planes of n units each, k = 0, 1, ...: (b, l) advances by (T / n, T % n) with
// one carry, so the only divisions are the two of the constructor. Unit i exists iff b < B.
struct CnBnWalk {
  int b, l, n, qt, rt;
  // The thread index goes through an empty asm: the compiler then cannot merge the walks of one kernel and keep every
  // unit's offsets in registers from the loads to the stores (that spilled; recomputing them is a few integer ops).
  __device__ __forceinline__ CnBnWalk(int t, int T, int n_) : n(n_) {
    asm volatile("" : "+v"(t));
    b = t / n_;
    l = t - b * n_;
    qt = T / n_;
    rt = T - qt * n_;
  }
  __device__ __forceinline__ void next() {
    b += qt;
    l += rt;
    if (l >= n) {
      l -= n;
      ++b;
    }
  }
};

template <int T, int NV, int GS, bool V4>
__global__ __launch_bounds__(T) void cn_bn_res_fwd_kernel(const CnBnGroupArgs a) {
  typedef typename CnBnUnit<V4>::type V;
  constexpr int U = V4 ? 4 : 1;
  __shared__ double scratch[2 * (T / 64)];
  const int c = blockIdx.x, g0 = GS == 1 ? blockIdx.y : 0;
  const int n = a.L / U;
  const long r0 = (long)c * a.L;
  V v[GS][NV];
  {
    CnBnWalk w(threadIdx.x, T, n);
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      if (w.b < a.B) {
        const long o = w.b * a.xbs + r0 + w.l * U;
#pragma unroll
        for (int g = 0; g < GS; ++g) v[g][k] = *reinterpret_cast<const V*>(a.x[g0 + g] + o);
      } else {
#pragma unroll
        for (int g = 0; g < GS; ++g) cn_bn_clear(v[g][k]);
      }
      w.next();
    }
  }
  const double count = (double)a.B * a.L;
  float m[GS], sc[GS], be[GS];
#pragma unroll
  for (int g = 0; g < GS; ++g) {
    double s = 0.0, ss = 0.0;
#pragma unroll
    for (int k = 0; k < NV; ++k) cn_bn_stat(v[g][k], s, ss);  // a unit past the end holds zeros
    cn_bn_block_sum2<T>(s, ss, scratch);
    const double md = s / count;
    double var = ss / count - md * md;
    if (var < 0.0) var = 0.0;
    m[g] = (float)md;
    const float rs = (float)(1.0 / sqrt(var + (double)a.eps));
    if (threadIdx.x == 0) {
      a.mean[g0 + g][c] = m[g];
      a.rstd[g0 + g][c] = rs;
      if (a.running_mean[g0 + g] != nullptr) {
        const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
        float* rm = a.running_mean[g0 + g];
        float* rv = a.running_var[g0 + g];
        rm[c] = (1.f - a.momentum) * rm[c] + a.momentum * m[g];
        rv[c] = (1.f - a.momentum) * rv[c] + a.momentum * (float)unbiased;
      }
    }
    sc[g] = a.gamma[g0 + g][c] * rs;
    be[g] = a.beta[g0 + g][c];
  }
  // The residual is fetched BN_RES_CHUNK units at a time, each batch ahead of its stores (next to every store, each
  // load waited for the store before it: see cn_ln_fwd_reg_kernel), so it costs a fixed few registers.
  const bool has_res = a.res != nullptr;
  const int act = a.act;
  float* yp = a.y[g0];
  CnBnWalk w(threadIdx.x, T, n);
#pragma unroll
  for (int k0 = 0; k0 < NV; k0 += BN_RES_CHUNK) {
    V rr[BN_RES_CHUNK];
    if (has_res) {
      CnBnWalk wr = w;
#pragma unroll
      for (int j = 0; j < BN_RES_CHUNK; ++j) {
        if (k0 + j < NV && wr.b < a.B) rr[j] = *reinterpret_cast<const V*>(a.res + wr.b * a.rbs + r0 + wr.l * U);
        wr.next();
      }
    }
#pragma unroll
    for (int j = 0; j < BN_RES_CHUNK; ++j) {
      const int k = k0 + j;
      if (k < NV) {
        if (w.b < a.B) {
          V acc;
#pragma unroll
          for (int g = 0; g < GS; ++g) {
            const float mg = m[g], sg = sc[g], bg = be[g];
            const V z = cn_bn_map(v[g][k], v[g][k], [&](float xv, float) {
              const float t = (xv - mg) * sg + bg;
              return act == 1 ? cn_silu(t) : t;
            });
            if (g == 0) {
              if (has_res) acc = cn_bn_map(rr[j], z, [](float r, float f) { return r + f; });
              else if (a.sum_outputs) acc = cn_bn_map(z, z, [](float f, float) { return 0.f + f; });
              else acc = z;
            } else {
              acc = cn_bn_map(acc, z, [](float p, float f) { return p + f; });  // res + f_0 + f_1 + ...
            }
          }
          *reinterpret_cast<V*>(yp + w.b * a.ybs + r0 + w.l * U) = acc;
        }
        w.next();
      }
    }
  }
}

// Backward: the block holds xhat and dz = dy * SiLU'(gamma * xhat + beta) of its channel (SiLU' evaluated once), forms
// sum dz and sum dz * xhat in fp64, writes dgamma / dbeta and stores dx. Always one group per block, grid = (C, G),
// also behind one dy for all groups: a block that owned its channel in all groups and loaded dy once was measured
// SLOWER (C = 128 at 50 x 50: 24.2 us against 17.9; 25 x 25: 12.1 against 8.6 -- half the blocks, twice the registers,
// and the second read of dy comes from the caches).
template <int T, int NV, bool V4>
__global__ __launch_bounds__(T) void cn_bn_res_bwd_kernel(const CnBnGroupArgs a) {
  typedef typename CnBnUnit<V4>::type V;
  constexpr int U = V4 ? 4 : 1;
  __shared__ double scratch[2 * (T / 64)];
  const int c = blockIdx.x, g = blockIdx.y;
  const int n = a.L / U;
  const long r0 = (long)c * a.L;
  V xh[NV], dz[NV];
  {
    CnBnWalk w(threadIdx.x, T, n);
    const float* xp = a.x[g];
    const float* dyp = a.dy[g];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      if (w.b < a.B) {
        xh[k] = *reinterpret_cast<const V*>(xp + w.b * a.xbs + r0 + w.l * U);
        dz[k] = *reinterpret_cast<const V*>(dyp + w.b * a.dybs + r0 + w.l * U);
      } else {
        cn_bn_clear(xh[k]);
        cn_bn_clear(dz[k]);
      }
      w.next();
    }
  }
  const double count = (double)a.B * a.L;
  const int act = a.act;
  const float m = a.mean[g][c], rs = a.rstd[g][c], ga = a.gamma[g][c], be = a.beta[g][c];
  double s1 = 0.0, s2 = 0.0;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    // a unit past the end holds x = dy = 0: dz = 0 there, and both sums are left as they are
    xh[k] = cn_bn_map(xh[k], xh[k], [&](float xv, float) { return (xv - m) * rs; });
    dz[k] = cn_bn_map(dz[k], xh[k], [&](float dv, float h) {
      if (act == 1) dv *= cn_silu_grad(ga * h + be);
      s1 += dv;
      s2 += (double)dv * h;
      return dv;
    });
  }
  cn_bn_block_sum2<T>(s1, s2, scratch);
  if (threadIdx.x == 0) {
    if (a.accumulate_params) {
      a.dgamma[g][c] += (float)s2;
      a.dbeta[g][c] += (float)s1;
    } else {
      a.dgamma[g][c] = (float)s2;
      a.dbeta[g][c] = (float)s1;
    }
  }
  float* dxp = a.dx[g];
  if (dxp == nullptr) return;
  const bool acc = a.accumulate_dx[g] != 0;
  const float k1 = a.training ? (float)(s1 / count) : 0.f, k2 = a.training ? (float)(s2 / count) : 0.f, kg = ga * rs;
  CnBnWalk w(threadIdx.x, T, n);
#pragma unroll
  for (int k0 = 0; k0 < NV; k0 += BN_RES_CHUNK) {
    V pv[BN_RES_CHUNK];
    if (acc) {  // the old dx, a batch ahead of its stores
      CnBnWalk wr = w;
#pragma unroll
      for (int j = 0; j < BN_RES_CHUNK; ++j) {
        if (k0 + j < NV && wr.b < a.B) pv[j] = *reinterpret_cast<const V*>(dxp + wr.b * a.dxbs + r0 + wr.l * U);
        wr.next();
      }
    }
#pragma unroll
    for (int j = 0; j < BN_RES_CHUNK; ++j) {
      const int k = k0 + j;
      if (k < NV) {
        if (w.b < a.B) {
          V o = cn_bn_map(dz[k], xh[k], [&](float d, float h) { return (d - k1 - h * k2) * kg; });
          if (acc) o = cn_bn_map(o, pv[j], [](float gr, float prev) { return gr + prev; });
          *reinterpret_cast<V*>(dxp + w.b * a.dxbs + r0 + w.l * U) = o;
        }
        w.next();
      }
    }
  }
}

// The rule that chooses the path: a pure function of the launch's shape (pass, groups, summed or not, B, C, L, unit).
// BN_RES_SHAPES lists the block shapes (threads T, units NV per thread and tensor) with the most summed groups a block
// of that shape takes in the forward and whether the backward (two tensors per value: xhat and dz) has it: those whose
// data registers, 4 * NV * tensors with 16-byte units, the compiler fits without scratch beside ~45 registers of
// addressing and fp64 sums under the cap of 128 of a 1024-thread block. The first shape that holds the channel is
// taken. At batch 8 that is: forward 100 x 100 (20 000 units) resident unless summed, two summed groups up to
// 50 x 50; backward up to 50 x 50.
struct CnBnPlan {
  int T, NV, GS;  // NV == 0: two-pass
};
static const struct { int T, NV, gs_fwd, bwd; } BN_RES_SHAPES[] = {{512, 4, 3, 1}, {1024, 5, 3, 1}, {1024, 10, 2, 1},
                                                                    {1024, 20, 1, 0}};
// A block streams its channel at the rate of ONE CU, so a launch of few blocks with much to stream is slower resident
// than as two wide launches. Isolated, in us, resident against two-pass (tools/bn_bench.py, profiles/
// r09_batchnorm_f32.txt; values = B * L * groups of the block):
//   blocks  values   forward         backward
//     9     80 000   26.8 / 15.4
//    64     80 000   29.9 / 23.7
//    64     40 000   17.8 / 16.0
//    64     20 000   11.0 / 12.3      9.3 / 13.1
//   128     20 000   12.1 / 16.1     14.2 / 19.2
//   128     40 000   19.8 / 21.2
//   256     80 000   47.9 / 61.5
// so with fewer than BN_RES_FULL_BLOCKS blocks only blocks of at most BN_RES_SMALL values go resident (below that a
// launch is fixed cost, not bytes: every 25 x 25 and 13 x 13 launch is 3 to 5 us faster resident).
#define BN_RES_FULL_BLOCKS 128
#define BN_RES_SMALL 20480

static CnBnPlan bn_resident_plan(bool backward, int G, bool summed, int B, int C, int L, bool v4) {
  const CnBnPlan none = {0, 0, 0};
  const long units = (long)B * (L / (v4 ? 4 : 1));
  const int GS = (!backward && summed) ? G : 1;  // the summed forward: a block owns its channel in all G groups
  for (const auto& s : BN_RES_SHAPES) {
    if ((backward ? !s.bwd : GS > s.gs_fwd) || (long)s.T * s.NV < units) continue;
#ifndef CN_BN_RESIDENT_ALL  // diagnostic build: every shape that fits goes resident (tools/bn_bench.py prices the rule)
    if ((long)C * (GS == 1 ? G : 1) < BN_RES_FULL_BLOCKS && (long)B * L * GS > BN_RES_SMALL) break;
#endif
    const CnBnPlan p = {s.T, s.NV, GS};
    return p;
  }
  return none;
}

template <bool BWD, int T, int NV, int GS>
static void bn_resident_launch_one(const CnBnGroupArgs& a, hipStream_t stream) {
  const dim3 grid(a.C, GS == 1 ? a.G : 1);
  if constexpr (BWD) {
    if (a.vec4) CN_LAUNCH((cn_bn_res_bwd_kernel<T, NV, true>), grid, dim3(T), 0, stream, a);
    else CN_LAUNCH((cn_bn_res_bwd_kernel<T, NV, false>), grid, dim3(T), 0, stream, a);
  } else {
    if (a.vec4) CN_LAUNCH((cn_bn_res_fwd_kernel<T, NV, GS, true>), grid, dim3(T), 0, stream, a);
    else CN_LAUNCH((cn_bn_res_fwd_kernel<T, NV, GS, false>), grid, dim3(T), 0, stream, a);
  }
}

// One case per (shape, groups per block) of BN_RES_SHAPES.
template <bool BWD>
static bool bn_resident_launch(const CnBnPlan& p, const CnBnGroupArgs& a, hipStream_t stream) {
#define CN_BN_RES(T_, NV_, GS_)                           \
  if (p.T == T_ && p.NV == NV_ && p.GS == GS_) {          \
    bn_resident_launch_one<BWD, T_, NV_, GS_>(a, stream); \
    return true;                                          \
  }
  CN_BN_RES(512, 4, 1) CN_BN_RES(1024, 5, 1) CN_BN_RES(1024, 10, 1)
  if constexpr (!BWD) {
    CN_BN_RES(512, 4, 2) CN_BN_RES(512, 4, 3) CN_BN_RES(1024, 5, 2) CN_BN_RES(1024, 5, 3) CN_BN_RES(1024, 10, 2)
    CN_BN_RES(1024, 20, 1)
  }
#undef CN_BN_RES
  return false;
}

// ---------------------------------------------------------------------------
// Two-pass BatchNorm, single (G = 1) and grouped calls alike: the channels that do not fit one block, the launches of
// few blocks on large planes, and every eval forward (the apply kernel alone).
// One body each, instantiated for MAXG = BN_MAX_GROUPS and for MAXG = 1: in a single call the group index is the
// constant 0, so the operands are kernel arguments and not entries of a table indexed at run time -- one dependent
// scalar load less per kernel, 0.6-0.8 us of a 9-21 us launch pair on 3 channels.
// Pass 1: part[g][c][split][2] = {sum, sumsq} of x over this block's share, in fp64. grid = (C, splits, G)
// ---------------------------------------------------------------------------
template <int MAXG>
__global__ __launch_bounds__(256) void cn_bn_group_partial_kernel(const CnBnGroupArgs a) {
  __shared__ double scratch[4];
  const int c = blockIdx.x, sp = blockIdx.y, g = MAXG == 1 ? 0 : blockIdx.z;
  double s = 0.0, ss = 0.0;
  if (a.vec4) {
    const int L4 = a.L >> 2;
    const int per = (L4 + a.splits - 1) / a.splits;
    const int beg = sp * per;
    const int end = (beg + per < L4) ? beg + per : L4;
    for (int b = 0; b < a.B; ++b) {
      const float4* xp = reinterpret_cast<const float4*>(a.x[g] + b * a.xbs + (long)c * a.L);
      for (int l = beg + threadIdx.x; l < end; l += 256) {
        const float4 v = xp[l];
        s += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);  // fp64: a channel far from zero
        ss += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
      }
    }
  } else {
    const int per = (a.L + a.splits - 1) / a.splits;
    const int beg = sp * per;
    const int end = (beg + per < a.L) ? beg + per : a.L;
    for (int b = 0; b < a.B; ++b) {
      const float* xp = a.x[g] + b * a.xbs + (long)c * a.L;
      for (int l = beg + threadIdx.x; l < end; l += 256) {
        const float v = xp[l];
        s += v;
        ss += (double)v * v;
      }
    }
  }
  s = cn_block_sum<double, 256>(s, scratch);
  ss = cn_block_sum<double, 256>(ss, scratch);
  if (threadIdx.x == 0) {
    double* p = a.part + (((long)g * a.C + c) * a.splits + sp) * 2;
    p[0] = s;
    p[1] = ss;
  }
}

// Pass 2: y_g = act(gamma * (x_g - mean) * rstd + beta), or y_0 = res + sum_g of that. act: 0 none, 1 SiLU.
// Training: every block reduces its channel's `splits` partial rows itself instead of waiting for a separate finalize
// launch. Eval: mean / rstd from the running statistics. Block (0, c, 0) publishes mean / rstd for the backward pass
// and, in training, updates the running statistics. grid = (blocks over L, C, B)
template <int MAXG>
__global__ __launch_bounds__(256) void cn_bn_group_apply_kernel(const CnBnGroupArgs a) {
  const int c = blockIdx.y, b = blockIdx.z;
  float m[MAXG], sc[MAXG], be[MAXG];
  const double count = (double)a.B * a.L;
#pragma unroll
  for (int g = 0; g < MAXG; ++g) {
    m[g] = sc[g] = be[g] = 0.f;
    if (g < a.G) {
      float rs;
      if (a.training) {
        double s, ss;
        cn_bn_sum_parts(a.part + ((long)g * a.C + c) * a.splits * 2, a.splits, s, ss);
        const double md = s / count;
        double var = ss / count - md * md;
        if (var < 0.0) var = 0.0;
        m[g] = (float)md;
        rs = (float)(1.0 / sqrt(var + (double)a.eps));
        if (blockIdx.x == 0 && b == 0 && threadIdx.x == 0) {
          a.mean[g][c] = m[g];
          a.rstd[g][c] = rs;
          if (a.running_mean[g] != nullptr) {
            const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
            a.running_mean[g][c] = (1.f - a.momentum) * a.running_mean[g][c] + a.momentum * m[g];
            a.running_var[g][c] = (1.f - a.momentum) * a.running_var[g][c] + a.momentum * (float)unbiased;
          }
        }
      } else {
        m[g] = a.running_mean[g][c];
        rs = 1.0f / sqrtf(a.running_var[g][c] + a.eps);
        if (blockIdx.x == 0 && b == 0 && threadIdx.x == 0) {
          a.mean[g][c] = m[g];
          a.rstd[g][c] = rs;
        }
      }
      sc[g] = a.gamma[g][c] * rs;
      be[g] = a.beta[g][c];
    }
  }
  const long r0 = (long)c * a.L;
  const float* rp = a.res ? a.res + b * a.rbs + r0 : nullptr;
  if (a.vec4) {  // 16-byte accesses: L % 4 == 0 and every plane 16-byte aligned
    const float4 z4 = {0.f, 0.f, 0.f, 0.f};
    for (int l = blockIdx.x * 256 + threadIdx.x; l < (a.L >> 2); l += gridDim.x * 256) {
      float4 acc = rp ? reinterpret_cast<const float4*>(rp)[l] : z4;
#pragma unroll
      for (int g = 0; g < MAXG; ++g) {
        if (g < a.G) {
          const float4 xv = reinterpret_cast<const float4*>(a.x[g] + b * a.xbs + r0)[l];
          float4 z;
          z.x = (xv.x - m[g]) * sc[g] + be[g];
          z.y = (xv.y - m[g]) * sc[g] + be[g];
          z.z = (xv.z - m[g]) * sc[g] + be[g];
          z.w = (xv.w - m[g]) * sc[g] + be[g];
          if (a.act == 1) { z.x = cn_silu(z.x); z.y = cn_silu(z.y); z.z = cn_silu(z.z); z.w = cn_silu(z.w); }
          if (a.sum_outputs) { acc.x += z.x; acc.y += z.y; acc.z += z.z; acc.w += z.w; }
          else reinterpret_cast<float4*>(a.y[g] + b * a.ybs + r0)[l] = z;
        }
      }
      if (a.sum_outputs) reinterpret_cast<float4*>(a.y[0] + b * a.ybs + r0)[l] = acc;
    }
    return;
  }
  for (int l = blockIdx.x * 256 + threadIdx.x; l < a.L; l += gridDim.x * 256) {
    float acc = rp ? rp[l] : 0.f;
#pragma unroll
    for (int g = 0; g < MAXG; ++g) {
      if (g < a.G) {
        float z = (a.x[g][b * a.xbs + r0 + l] - m[g]) * sc[g] + be[g];
        if (a.act == 1) z = cn_silu(z);
        if (a.sum_outputs) acc += z;  // res + f_0 + f_1 + ...: the order of the sequential form
        else a.y[g][b * a.ybs + r0 + l] = z;
      }
    }
    if (a.sum_outputs) a.y[0][b * a.ybs + r0 + l] = acc;
  }
}

// Backward pass 1: per-channel partial sums of dz and dz * xhat, dz = dy * act'(z). grid = (C, splits, G)
template <int MAXG>
__global__ __launch_bounds__(256) void cn_bn_group_bwd_partial_kernel(const CnBnGroupArgs a) {
  __shared__ double scratch[4];
  const int c = blockIdx.x, sp = blockIdx.y, g = MAXG == 1 ? 0 : blockIdx.z;
  const float m = a.mean[g][c], rs = a.rstd[g][c], ga = a.gamma[g][c], be = a.beta[g][c];
  double s1 = 0.0, s2 = 0.0;
  auto term = [&](float xv, float dv) {
    const float xh = (xv - m) * rs;
    float dz = dv;
    if (a.act == 1) dz *= cn_silu_grad(ga * xh + be);
    s1 += dz;
    s2 += (double)dz * xh;
  };
  if (a.vec4) {  // 16-byte lane loads (scalar loads ran this pass at 1.9 TB/s)
    const int L4 = a.L >> 2;
    const int per = (L4 + a.splits - 1) / a.splits;
    const int beg = sp * per;
    const int end = (beg + per < L4) ? beg + per : L4;
    for (int b = 0; b < a.B; ++b) {
      const float4* xp = reinterpret_cast<const float4*>(a.x[g] + b * a.xbs + (long)c * a.L);
      const float4* dp = reinterpret_cast<const float4*>(a.dy[g] + b * a.dybs + (long)c * a.L);
      for (int l = beg + threadIdx.x; l < end; l += 256) {
        const float4 xv = xp[l], dv = dp[l];
        term(xv.x, dv.x); term(xv.y, dv.y); term(xv.z, dv.z); term(xv.w, dv.w);
      }
    }
  } else {
    const int per = (a.L + a.splits - 1) / a.splits;
    const int beg = sp * per;
    const int end = (beg + per < a.L) ? beg + per : a.L;
    for (int b = 0; b < a.B; ++b) {
      const float* xp = a.x[g] + b * a.xbs + (long)c * a.L;
      const float* dp = a.dy[g] + b * a.dybs + (long)c * a.L;
      for (int l = beg + threadIdx.x; l < end; l += 256) term(xp[l], dp[l]);
    }
  }
  s1 = cn_block_sum<double, 256>(s1, scratch);
  s2 = cn_block_sum<double, 256>(s2, scratch);
  if (threadIdx.x == 0) {
    double* p = a.part + (((long)g * a.C + c) * a.splits + sp) * 2;
    p[0] = s1;
    p[1] = s2;
  }
}

// Backward pass 2: dx (+)= gamma*rstd*(dz - mean(dz) - xhat*mean(dz*xhat))   [train]
//                  dx (+)= gamma*rstd*dz                                        [eval]
// Every block reduces its channel's partial rows itself; block (0, c, 0) of a group writes or accumulates dgamma /
// dbeta. grid = (blocks over L x G, C, B), or (G, C, 1) when no group wants dx.
template <int MAXG>
__global__ __launch_bounds__(256) void cn_bn_group_bwd_apply_kernel(const CnBnGroupArgs a, int bx_per_group) {
  const int g = MAXG == 1 ? 0 : blockIdx.x / bx_per_group, bx = blockIdx.x - g * bx_per_group;
  const int c = blockIdx.y, b = blockIdx.z;
  double s1, s2;
  cn_bn_sum_parts(a.part + ((long)g * a.C + c) * a.splits * 2, a.splits, s1, s2);
  if (bx == 0 && b == 0 && threadIdx.x == 0) {
    if (a.accumulate_params) {
      a.dgamma[g][c] += (float)s2;
      a.dbeta[g][c] += (float)s1;
    } else {
      a.dgamma[g][c] = (float)s2;
      a.dbeta[g][c] = (float)s1;
    }
  }
  if (a.dx[g] == nullptr) return;
  const double count = (double)a.B * a.L;
  const float m = a.mean[g][c], rs = a.rstd[g][c], ga = a.gamma[g][c], be = a.beta[g][c];
  const float c1 = a.training ? (float)(s1 / count) : 0.f, c2 = a.training ? (float)(s2 / count) : 0.f;
  const long r0 = (long)c * a.L;
  const float* xp = a.x[g] + b * a.xbs + r0;
  const float* dp = a.dy[g] + b * a.dybs + r0;
  float* dxp = a.dx[g] + b * a.dxbs + r0;
  const int acc = a.accumulate_dx[g];
  const float gs = ga * rs;
  auto grad = [&](float xv, float dv, float prev) {
    const float xh = (xv - m) * rs;
    float dz = dv;
    if (a.act == 1) dz *= cn_silu_grad(ga * xh + be);
    float gr = (dz - c1 - xh * c2) * gs;
    if (acc) gr += prev;
    return gr;
  };
  if (a.vec4) {
    const float4* x4 = reinterpret_cast<const float4*>(xp);
    const float4* d4 = reinterpret_cast<const float4*>(dp);
    float4* o4 = reinterpret_cast<float4*>(dxp);
    const float4 z = {0.f, 0.f, 0.f, 0.f};
    for (int l = bx * 256 + threadIdx.x; l < (a.L >> 2); l += bx_per_group * 256) {
      const float4 xv = x4[l], dv = d4[l];
      const float4 pv = acc ? o4[l] : z;
      float4 o;
      o.x = grad(xv.x, dv.x, pv.x); o.y = grad(xv.y, dv.y, pv.y);
      o.z = grad(xv.z, dv.z, pv.z); o.w = grad(xv.w, dv.w, pv.w);
      o4[l] = o;
    }
    return;
  }
  for (int l = bx * 256 + threadIdx.x; l < a.L; l += bx_per_group * 256) dxp[l] = grad(xp[l], dp[l], acc ? dxp[l] : 0.f);
}

// May a call use 16-byte accesses? L and every batch stride a multiple of 4 floats, every plane base 16-byte aligned.
// tabs: pointer tables of CnBnGroupArgs (unused slots are NULL and pass, as a NULL `one` does). One flag covers both
// passes of a call.
static int bn_vec4(int L, std::initializer_list<long> strides, std::initializer_list<const float* const*> tabs,
                   const float* one = nullptr) {
  bool ok = L % 4 == 0 && reinterpret_cast<uintptr_t>(one) % 16 == 0;
  for (long s : strides) ok = ok && s % 4 == 0;
  for (const float* const* t : tabs)
    for (int g = 0; g < BN_MAX_GROUPS; ++g) ok = ok && reinterpret_cast<uintptr_t>(t[g]) % 16 == 0;
  return ok;
}

// The argument block of a single call: G = 1 and up to BN_SPLIT_MAX partial rows. The forward and the backward entry
// add their own operands.
static CnBnGroupArgs bn_single_args(const float* x, long xbs, const float* gamma, const float* beta, const float* mean,
                                    const float* rstd, double* ws, int B, int C, int L, int training, int act) {
  CnBnGroupArgs a = {};
  a.x[0] = x; a.gamma[0] = gamma; a.beta[0] = beta;
  a.mean[0] = const_cast<float*>(mean); a.rstd[0] = const_cast<float*>(rstd);
  a.xbs = xbs; a.G = 1; a.B = B; a.C = C; a.L = L; a.act = act; a.training = training;
  a.part = ws; a.splits = bn_splits_wide(C, L);
  return a;
}

// A two-pass kernel on 256 threads: the instance of a single call or the grouped one.
#define BN_2P_LAUNCH(kernel_, grid_, ...)                                                           \
  do {                                                                                              \
    if (a.G == 1) CN_LAUNCH((kernel_<1>), grid_, dim3(256), 0, stream, a, ##__VA_ARGS__);           \
    else CN_LAUNCH((kernel_<BN_MAX_GROUPS>), grid_, dim3(256), 0, stream, a, ##__VA_ARGS__);        \
  } while (0)

// Forward of a filled argument block: resident where bn_resident_plan allows, else the partial sums (training only) and
// the apply launch.
static int bn_forward(CnBnGroupArgs& a, hipStream_t stream) {
  for (int g = 0; g < a.G; ++g)
    if (!a.training && (a.running_mean[g] == nullptr || a.running_var[g] == nullptr)) return CN_ERR_ARG;
  a.vec4 = bn_vec4(a.L, {a.xbs, a.ybs, a.res ? a.rbs : 0}, {a.x, a.y}, a.res);
  if (a.training) {
    const CnBnPlan p = bn_resident_plan(false, a.G, a.sum_outputs != 0, a.B, a.C, a.L, a.vec4 != 0);
    if (p.NV != 0 && bn_resident_launch<false>(p, a, stream)) return cn_check_launch();
    BN_2P_LAUNCH(cn_bn_group_partial_kernel, dim3(a.C, a.splits, a.G));
  }
  BN_2P_LAUNCH(cn_bn_group_apply_kernel, plane_grid(a.B, a.C, a.L));
  return cn_check_launch();
}

// Backward of a filled argument block. With no dx wanted at all the apply launch shrinks to one block per channel and
// group: the parameter gradients alone.
static int bn_backward(CnBnGroupArgs& a, hipStream_t stream) {
  bool any_dx = false;
  for (int g = 0; g < a.G; ++g) any_dx |= a.dx[g] != nullptr;
  a.vec4 = bn_vec4(a.L, {a.xbs, a.dybs, any_dx ? a.dxbs : 0}, {a.x, a.dy, a.dx});
  const CnBnPlan p = bn_resident_plan(true, a.G, false, a.B, a.C, a.L, a.vec4 != 0);
  if (p.NV != 0 && bn_resident_launch<true>(p, a, stream)) return cn_check_launch();
  const dim3 pg = any_dx ? plane_grid(a.B, a.C, a.L) : dim3(1, a.C, 1);
  BN_2P_LAUNCH(cn_bn_group_bwd_partial_kernel, dim3(a.C, a.splits, a.G));
  BN_2P_LAUNCH(cn_bn_group_bwd_apply_kernel, dim3(pg.x * a.G, pg.y, pg.z), (int)pg.x);
  return cn_check_launch();
}

// Forward. x,y viewed as [B][C][L] (L = H*W for BatchNorm2d, T*H*W for BatchNorm3d).
// training != 0: batch statistics (saved to mean/rstd [C]) and running stats updated in place; == 0: the running
// statistics (required), copied to mean / rstd for the backward. ws: workspace of cn_bn_workspace_doubles(C) doubles.
extern "C" int cn_bn_act_fwd_f32(const float* x, long xbs, const float* gamma, const float* beta,
                                 float* running_mean, float* running_var, const float* res, long rbs, float* y,
                                 long ybs, float* mean, float* rstd, double* ws, int B, int C, int L, int training,
                                 float momentum, float eps, int act, void* stream_) {
  if (B <= 0 || C <= 0 || L <= 0) return CN_OK;
  CnBnGroupArgs a = bn_single_args(x, xbs, gamma, beta, mean, rstd, ws, B, C, L, training, act);
  a.running_mean[0] = running_mean; a.running_var[0] = running_mean != nullptr ? running_var : nullptr;
  a.y[0] = y; a.ybs = ybs; a.res = res; a.rbs = rbs; a.sum_outputs = res != nullptr;  // y = res + act(bn(x))
  a.eps = eps; a.momentum = momentum;
  return bn_forward(a, (hipStream_t)stream_);
}

// Backward. dgamma/dbeta (+)= per accumulate_params; dx (+)= per accumulate_dx; dx may be NULL (parameters only).
// coef: unused, kept for the ABI (may be NULL); ws as in forward.
extern "C" int cn_bn_act_bwd_f32(const float* x, long xbs, const float* dy, long dybs, const float* mean,
                                 const float* rstd, const float* gamma, const float* beta, float* dx, long dxbs,
                                 float* dgamma, float* dbeta, float* coef, double* ws, int B, int C, int L,
                                 int training, int act, int accumulate_dx, int accumulate_params, void* stream_) {
  (void)coef;
  if (B <= 0 || C <= 0 || L <= 0) return CN_OK;
  CnBnGroupArgs a = bn_single_args(x, xbs, gamma, beta, mean, rstd, ws, B, C, L, training, act);
  a.dy[0] = dy; a.dybs = dybs; a.dx[0] = dx; a.dxbs = dxbs; a.accumulate_dx[0] = accumulate_dx;
  a.dgamma[0] = dgamma; a.dbeta[0] = dbeta; a.accumulate_params = accumulate_params;
  return bn_backward(a, (hipStream_t)stream_);
}

// Host arrays of G device pointers; ws: G * cn_bn_workspace_doubles(C) doubles.
// sum_outputs == 0: ys[g] = act(bn_g(xs[g])) (res must be NULL); != 0: ys[0] = res + sum_g act(bn_g(xs[g])).
extern "C" int cn_bn_act_group_fwd_f32(int G, const float* const* xs, long xbs, const float* const* gammas,
                                       const float* const* betas, float* const* running_means,
                                       float* const* running_vars, const float* res, long rbs, float* const* ys,
                                       long ybs, float* const* means, float* const* rstds, double* ws, int B, int C,
                                       int L, int training, float momentum, float eps, int act, int sum_outputs,
                                       void* stream_) {
  if (G < 1 || G > BN_MAX_GROUPS || (!sum_outputs && res != nullptr)) return CN_ERR_ARG;
  if (B <= 0 || C <= 0 || L <= 0) return CN_OK;
  CnBnGroupArgs a = {};
  for (int g = 0; g < G; ++g) {
    a.x[g] = xs[g]; a.gamma[g] = gammas[g]; a.beta[g] = betas[g];
    a.running_mean[g] = running_means ? running_means[g] : nullptr;
    a.running_var[g] = running_vars ? running_vars[g] : nullptr;
    a.mean[g] = means[g]; a.rstd[g] = rstds[g];
    a.y[g] = sum_outputs ? ys[0] : ys[g];
  }
  a.xbs = xbs; a.ybs = ybs; a.rbs = rbs; a.res = res;
  a.G = G; a.B = B; a.C = C; a.L = L; a.act = act; a.training = training; a.sum_outputs = sum_outputs;
  a.eps = eps; a.momentum = momentum; a.part = ws;
  a.splits = bn_splits(C * G, L);
  return bn_forward(a, (hipStream_t)stream_);
}

// dys: per-group output gradients (the same pointer G times after a summed forward). dxs[g] may be NULL.
extern "C" int cn_bn_act_group_bwd_f32(int G, const float* const* xs, long xbs, const float* const* dys, long dybs,
                                       const float* const* means, const float* const* rstds,
                                       const float* const* gammas, const float* const* betas, float* const* dxs,
                                       long dxbs, const int* accumulate_dx, float* const* dgammas,
                                       float* const* dbetas, double* ws, int B, int C, int L, int training, int act,
                                       int accumulate_params, void* stream_) {
  if (G < 1 || G > BN_MAX_GROUPS) return CN_ERR_ARG;
  if (B <= 0 || C <= 0 || L <= 0) return CN_OK;
  CnBnGroupArgs a = {};
  for (int g = 0; g < G; ++g) {
    a.x[g] = xs[g]; a.dy[g] = dys[g]; a.gamma[g] = gammas[g]; a.beta[g] = betas[g];
    a.mean[g] = const_cast<float*>(means[g]); a.rstd[g] = const_cast<float*>(rstds[g]);
    a.dx[g] = dxs ? dxs[g] : nullptr; a.dgamma[g] = dgammas[g]; a.dbeta[g] = dbetas[g];
    a.accumulate_dx[g] = accumulate_dx ? accumulate_dx[g] : 0;
  }
  a.xbs = xbs; a.dybs = dybs; a.dxbs = dxbs;
  a.G = G; a.B = B; a.C = C; a.L = L; a.act = act; a.training = training; a.accumulate_params = accumulate_params;
  a.part = ws;
  a.splits = bn_splits(C * G, L);
  return bn_backward(a, (hipStream_t)stream_);
}

// ---------------------------------------------------------------------------
// Per-channel sum over [B][C][L] (bias gradients): out[c] (+)= sum x[b,c,l]
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cn_channel_sum_kernel(const float* __restrict__ x, long xbs, int B, int C,
                                                            int L, int splits, float* __restrict__ out) {
  __shared__ double scratch[4];
  const int c = blockIdx.x, sp = blockIdx.y;
  const int per = (L + splits - 1) / splits;
  const int beg = sp * per;
  const int end = (beg + per < L) ? beg + per : L;
  double s = 0.0;
  for (int b = 0; b < B; ++b) {
    const float* xp = x + b * xbs + (long)c * L;
    for (int l = beg + threadIdx.x; l < end; l += 256) s += xp[l];
  }
  s = cn_block_sum<double, 256>(s, scratch);
  if (threadIdx.x == 0) atomicAdd(out + c, (float)s);
}

extern "C" int cn_channel_sum_f32(const float* x, long xbs, int B, int C, int L, float* out, int accumulate,
                                  void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (C <= 0) return CN_OK;
  if (!accumulate && hipMemsetAsync(out, 0, sizeof(float) * C, stream) != hipSuccess) return CN_ERR_LAUNCH;
  const int splits = bn_splits(C, L);
  CN_LAUNCH(cn_channel_sum_kernel, dim3(C, splits), dim3(256), 0, stream, x, xbs, B, C, L, splits, out);
  return cn_check_launch();
}

// ---------------------------------------------------------------------------
// LayerNorm over C for NCHW tensors: one lane per pixel, values strided by L.
//   y = (x - mu) * rstd * w[c] + b[c] (+ residual);  mu/rstd saved per pixel [B][L].
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cn_ln_fwd_kernel(const float* __restrict__ x, long xbs,
                                                       const float* __restrict__ w, const float* __restrict__ bvec,
                                                       const float* __restrict__ res, long rbs,
                                                       float* __restrict__ y, long ybs, float* __restrict__ mu,
                                                       float* __restrict__ rstd, int B, int C, int L, float eps) {
  const long p = blockIdx.x * 256L + threadIdx.x;
  if (p >= (long)B * L) return;
  const long b = p / L, l = p - b * L;
  const float* xp = x + b * xbs + l;
  float s = 0.f;
  for (int c = 0; c < C; ++c) s += xp[(long)c * L];
  const float m = s / C;
  float v = 0.f;
  for (int c = 0; c < C; ++c) {
    const float d = xp[(long)c * L] - m;
    v += d * d;
  }
  const float rs = 1.0f / sqrtf(v / C + eps);
  mu[p] = m;
  rstd[p] = rs;
  float* yp = y + b * ybs + l;
  const float* rp = res ? res + b * rbs + l : nullptr;
  for (int c = 0; c < C; ++c) {
    float o = (xp[(long)c * L] - m) * rs * w[c] + bvec[c];
    if (rp) o += rp[(long)c * L];
    yp[(long)c * L] = o;
  }
}

// dx (+)= rstd * (g - mean_c(g) - xhat * mean_c(g*xhat)), g = dy*w; dw/db via block partials + atomics.
template <int MAXC>
__global__ __launch_bounds__(256) void cn_ln_bwd_kernel(const float* __restrict__ x, long xbs,
                                                       const float* __restrict__ dy, long dybs,
                                                       const float* __restrict__ w, const float* __restrict__ mu,
                                                       const float* __restrict__ rstd, float* __restrict__ dx,
                                                       long dxbs, float* __restrict__ dw, float* __restrict__ db,
                                                       int B, int C, int L, int accumulate_dx) {
  __shared__ float red[2][4][MAXC];
  const long p = blockIdx.x * 256L + threadIdx.x;
  const bool ok = p < (long)B * L;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  long b = 0, l = 0;
  float m = 0.f, rs = 0.f;
  if (ok) {
    b = p / L;
    l = p - b * L;
    m = mu[p];
    rs = rstd[p];
  }
  const float* xp = x + b * xbs + l;
  const float* dp = dy + b * dybs + l;
  float s1 = 0.f, s2 = 0.f;
  for (int c = 0; c < C; ++c) {
    float g = 0.f, xh = 0.f, d = 0.f;
    if (ok) {
      d = dp[(long)c * L];
      xh = (xp[(long)c * L] - m) * rs;
      g = d * w[c];
    }
    s1 += g;
    s2 += g * xh;
    // per-channel parameter gradients: wave reduce, then one LDS slot per wave
    const float dwv = cn_wave_sum(d * xh);
    const float dbv = cn_wave_sum(d);
    if (lane == 0) {
      red[0][wid][c] = dwv;
      red[1][wid][c] = dbv;
    }
  }
  if (ok) {
    const float a1 = s1 / C, a2 = s2 / C;
    float* dxp = dx + b * dxbs + l;
    for (int c = 0; c < C; ++c) {
      const float xh = (xp[(long)c * L] - m) * rs;
      float g = rs * (dp[(long)c * L] * w[c] - a1 - xh * a2);
      if (accumulate_dx) g += dxp[(long)c * L];
      dxp[(long)c * L] = g;
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    atomicAdd(dw + c, red[0][0][c] + red[0][1][c] + red[0][2][c] + red[0][3][c]);
    atomicAdd(db + c, red[1][0][c] + red[1][1][c] + red[1][2][c] + red[1][3][c]);
  }
}

// ---- C <= 128: 64 pixels per block, the channels split over the 4 waves (CPW each) and held in registers, so x
// (and dy) are read ONCE and a 100x100 chip batch gives ~5 waves per SIMD instead of ~1. The per-pixel statistics
// are combined through LDS (two passes over the registers: mean, then centred variance, like the reference).
template <int CPW>
__global__ __launch_bounds__(256) void cn_ln_fwd_reg_kernel(const float* __restrict__ x, long xbs,
                                                           const float* __restrict__ w,
                                                           const float* __restrict__ bvec,
                                                           const float* __restrict__ res, long rbs,
                                                           float* __restrict__ y, long ybs, float* __restrict__ mu,
                                                           float* __restrict__ rstd, int B, int C, int L, float eps) {
  __shared__ float red[2][4][64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const long p = blockIdx.x * 64L + lane;
  const bool ok = p < (long)B * L;
  const long b = ok ? p / L : 0, l = ok ? p - b * L : 0;
  const int c0 = wid * CPW;
  const float* xp = x + b * xbs + l + (long)c0 * L;
  const float* rp = res ? res + b * rbs + l + (long)c0 * L : nullptr;
  float xv[CPW], rv[CPW];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < CPW; ++i) {
    xv[i] = (ok && c0 + i < C) ? xp[(long)i * L] : 0.f;
    s += xv[i];
  }
  // The residual is fetched here, with x, and held: read next to the stores at the end, each load waited for the store
  // before it and the launch ran at half the bandwidth of the one without a residual.
#pragma unroll
  for (int i = 0; i < CPW; ++i) rv[i] = (rp && ok && c0 + i < C) ? rp[(long)i * L] : 0.f;
  red[0][wid][lane] = s;
  __syncthreads();
  const float m = (red[0][0][lane] + red[0][1][lane] + red[0][2][lane] + red[0][3][lane]) / C;
  float v = 0.f;
#pragma unroll
  for (int i = 0; i < CPW; ++i) {
    const float d = xv[i] - m;
    v += (c0 + i < C) ? d * d : 0.f;
  }
  red[1][wid][lane] = v;
  __syncthreads();
  const float rs = 1.0f / sqrtf((red[1][0][lane] + red[1][1][lane] + red[1][2][lane] + red[1][3][lane]) / C + eps);
  if (!ok) return;
  if (wid == 0) {
    mu[p] = m;
    rstd[p] = rs;
  }
  float* yp = y + b * ybs + l + (long)c0 * L;
#pragma unroll
  for (int i = 0; i < CPW; ++i) {
    if (c0 + i < C) {
      float o = (xv[i] - m) * rs * w[c0 + i] + bvec[c0 + i];
      if (rp) o += rv[i];
      yp[(long)i * L] = o;
    }
  }
}

// Backward: tiles of 64 pixels (grid-stride), the channels split over the block's 8 waves (CPW each: 4 / 8 / 16 for
// C <= 32 / 64 / 128) and held in registers. With 4 waves of 32 channels the kernel held 220 VGPRs, two blocks per
// CU, and every block ran one tile: load, barrier, store, 64 wave trees, each phase waiting for the one before it with
// nothing else on the SIMD (1.3 TB/s at 100 x 100). Eight waves of 16 channels hold 128 VGPRs (4 waves per
// SIMD), and ln_bwd_blocks() gives a block several tiles, so the wave trees run once per block, not once per tile.
// The old dx of an accumulating launch is fetched with x and dy, not next to the stores (see the forward kernel).
// The parameter gradients are kept per lane across the block's tiles, reduced once per block and written to the
// workspace part[block][2][C] (same-address float atomics serialise at ~200 ns each); cn_ln_param_finalize_kernel
// sums the partials.
// Lengths of the fp32 chains: per pixel CPW products in a lane, then a tree over the 8 waves (3): CPW + 3. dw / db:
// ceil(ntiles / nblk) tiles in a lane, the wave tree (6), then the finalize kernel (ceil(nblk / 128) + 8 + 16); at
// [8, 128, 100, 100] that is 3 + 6 + 4 + 24 = 37.
#define LN_BWD_WAVES 8
template <int CPW, bool ACC>  // ACC: dx += the gradient
__global__ __launch_bounds__(64 * LN_BWD_WAVES) __attribute__((amdgpu_waves_per_eu(4, 8))) void cn_ln_bwd_reg_kernel(
    const float* __restrict__ x, long xbs, const float* __restrict__ dy, long dybs, const float* __restrict__ w,
    const float* __restrict__ mu, const float* __restrict__ rstd, float* __restrict__ dx, long dxbs,
    float* __restrict__ part, int B, int C, int L, int ntiles) {
  __shared__ float red[2][2][LN_BWD_WAVES][64];  // [tile parity]: one barrier per tile
  __shared__ float wsh[LN_BWD_WAVES * CPW];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int c0 = wid * CPW;
  float dwacc[CPW], dbacc[CPW];
#pragma unroll
  for (int i = 0; i < CPW; ++i) dwacc[i] = dbacc[i] = 0.f;
  if (threadIdx.x < LN_BWD_WAVES * CPW) wsh[threadIdx.x] = threadIdx.x < C ? w[threadIdx.x] : 0.f;
  __syncthreads();
  int par = 0;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x, par ^= 1) {
    const long p = tile * 64L + lane;
    const bool ok = p < (long)B * L;
    const long b = ok ? p / L : 0, l = ok ? p - b * L : 0;
    const float* xp = x + b * xbs + l + (long)c0 * L;
    const float* dp = dy + b * dybs + l + (long)c0 * L;
    float* dxp = dx + b * dxbs + l + (long)c0 * L;
    float xh[CPW], g[CPW], old[CPW];
#pragma unroll
    for (int i = 0; i < CPW; ++i) {
      const bool cok = ok && c0 + i < C;
      g[i] = cok ? dp[(long)i * L] : 0.f;
      xh[i] = cok ? xp[(long)i * L] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < CPW; ++i) old[i] = (ACC && ok && c0 + i < C) ? dxp[(long)i * L] : 0.f;
    const float m = ok ? mu[p] : 0.f, rs = ok ? rstd[p] : 0.f;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < CPW; ++i) {
      const bool cok = ok && c0 + i < C;
      const float d = g[i];
      xh[i] = cok ? (xh[i] - m) * rs : 0.f;
      g[i] = d * wsh[c0 + i];
      s1 += g[i];
      s2 += g[i] * xh[i];
      dwacc[i] = fmaf(d, xh[i], dwacc[i]);
      dbacc[i] += d;
    }
    red[par][0][wid][lane] = s1;
    red[par][1][wid][lane] = s2;
    __syncthreads();  // the next tile writes the other half of red[]; its barrier is behind this tile's readers
    if (ok) {
      const float(*r1)[64] = red[par][0];
      const float(*r2)[64] = red[par][1];
      const float a1 = (((r1[0][lane] + r1[1][lane]) + (r1[2][lane] + r1[3][lane])) +
                        ((r1[4][lane] + r1[5][lane]) + (r1[6][lane] + r1[7][lane]))) / C;
      const float a2 = (((r2[0][lane] + r2[1][lane]) + (r2[2][lane] + r2[3][lane])) +
                        ((r2[4][lane] + r2[5][lane]) + (r2[6][lane] + r2[7][lane]))) / C;
#pragma unroll
      for (int i = 0; i < CPW; ++i) {
        if (c0 + i < C) {
          float o = rs * (g[i] - a1 - xh[i] * a2);
          if (ACC) o += old[i];
          dxp[(long)i * L] = o;
        }
      }
    }
  }
  float* pw = part + (long)blockIdx.x * 2 * C;
#pragma unroll
  for (int i = 0; i < CPW; ++i) {
    const float dwv = cn_wave_sum_to_lane63(dwacc[i]);
    const float dbv = cn_wave_sum_to_lane63(dbacc[i]);
    if (lane == 63 && c0 + i < C) {
      pw[c0 + i] = dwv;
      pw[C + c0 + i] = dbv;
    }
  }
}

// dw[c] += sum_blocks part[blk][0][c], db[c] += sum_blocks part[blk][1][c]; grid = (ceil(2C / 32), 16): a block
// sums 1/16 of the block list for 32 values (8 sub-slices, LDS reduce) and issues one atomic per value.
__global__ __launch_bounds__(256) void cn_ln_param_finalize_kernel(const float* __restrict__ part, int nblk, int C,
                                                                  float* __restrict__ dw, float* __restrict__ db) {
  __shared__ float red[8][32];
  const int v = blockIdx.x * 32 + (threadIdx.x & 31), slice = blockIdx.y * 8 + (threadIdx.x >> 5);
  float s = 0.f;
  if (v < 2 * C)
    for (int k = slice; k < nblk; k += 8 * gridDim.y) s += part[(long)k * 2 * C + v];
  red[threadIdx.x >> 5][threadIdx.x & 31] = s;
  __syncthreads();
  if ((threadIdx.x >> 5) == 0 && v < 2 * C) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) t += red[k][threadIdx.x & 31];
    atomicAdd(v < C ? dw + v : db + (v - C), t);
  }
}

extern "C" int cn_layernorm_c_fwd_f32(const float* x, long xbs, const float* w, const float* b, const float* res,
                                      long rbs, float* y, long ybs, float* mu, float* rstd, int B, int C, int L,
                                      float eps, void* stream) {
  const long P = (long)B * L;
  if (P <= 0) return CN_OK;
  if (C <= 128) {
    const dim3 grid((unsigned)((P + 63) / 64));
#define CN_LN_FWD(CPW_)                                                                                             \
  CN_LAUNCH((cn_ln_fwd_reg_kernel<CPW_>), grid, dim3(256), 0, (hipStream_t)stream, x, xbs, w, b, res, rbs, y, \
                     ybs, mu, rstd, B, C, L, eps)
    if (C <= 32) CN_LN_FWD(8);
    else if (C <= 64) CN_LN_FWD(16);
    else CN_LN_FWD(32);
#undef CN_LN_FWD
    return cn_check_launch();
  }
  CN_LAUNCH(cn_ln_fwd_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, xbs,
                     w, b, res, rbs, y, ybs, mu, rstd, B, C, L, eps);
  return cn_check_launch();
}

// Blocks of the C <= 128 backward for `ntiles` tiles of 64 pixels. Two blocks of 8 waves fit a CU (256 CUs): up to 512
// blocks every tile has its own; beyond that a block walks ceil(ntiles / 512) tiles, and past 4096 tiles eight, so
// that the per-lane chain behind dw / db stays short (1250 tiles of a [8, 128, 100, 100] batch: 512 blocks of 2 - 3).
static long ln_bwd_blocks(long ntiles) {
  long nblk = ntiles < 512 ? ntiles : 512;
  if (ntiles / 8 > nblk) nblk = ntiles / 8;
  return nblk < 2048 ? nblk : 2048;
}

// Workspace of cn_layernorm_c_bwd_f32 in floats (per-block partial parameter gradients).
extern "C" int cn_layernorm_c_workspace_floats(int B, int C, int L) {
  const long ntiles = ((long)B * L + 63) / 64;
  return C <= 128 ? (int)(ln_bwd_blocks(ntiles) * 2 * C) : 0;
}

// dw/db are ACCUMULATED: zero them first for a fresh gradient. ws: cn_layernorm_c_workspace_floats(B, C, L)
// floats of scratch (C <= 128; wider layers use the atomic kernel and ignore it).
extern "C" int cn_layernorm_c_bwd_f32(const float* x, long xbs, const float* dy, long dybs, const float* w,
                                      const float* mu, const float* rstd, float* dx, long dxbs, float* dw,
                                      float* db, int B, int C, int L, int accumulate_dx, float* ws, long ws_floats,
                                      void* stream) {
  const long P = (long)B * L;
  if (P <= 0) return CN_OK;
  if (C > 512) return CN_ERR_ARG;
  if (C <= 128) {
    const long ntiles = (P + 63) / 64;
    const int nblk = (int)ln_bwd_blocks(ntiles);
    if (ws == nullptr || ws_floats < (long)nblk * 2 * C) return CN_ERR_ARG;
    const dim3 grid((unsigned)nblk);
#define CN_LN_BWD(CPW_)                                                                                           \
  do {                                                                                                            \
    if (accumulate_dx)                                                                                            \
      CN_LAUNCH((cn_ln_bwd_reg_kernel<CPW_, true>), grid, dim3(64 * LN_BWD_WAVES), 0, (hipStream_t)stream, x,     \
                xbs, dy, dybs, w, mu, rstd, dx, dxbs, ws, B, C, L, (int)ntiles);                                  \
    else                                                                                                          \
      CN_LAUNCH((cn_ln_bwd_reg_kernel<CPW_, false>), grid, dim3(64 * LN_BWD_WAVES), 0, (hipStream_t)stream, x,    \
                xbs, dy, dybs, w, mu, rstd, dx, dxbs, ws, B, C, L, (int)ntiles);                                  \
  } while (0)
    if (C <= 32) CN_LN_BWD(4);
    else if (C <= 64) CN_LN_BWD(8);
    else CN_LN_BWD(16);
#undef CN_LN_BWD
    CN_LAUNCH(cn_ln_param_finalize_kernel, dim3((2 * C + 31) / 32, 16), dim3(256), 0, (hipStream_t)stream, ws,
                       nblk, C, dw, db);
    return cn_check_launch();
  }
  CN_LAUNCH((cn_ln_bwd_kernel<512>), dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     x, xbs, dy, dybs, w, mu, rstd, dx, dxbs, dw, db, B, C, L, accumulate_dx);
  return cn_check_launch();
}


// ---------------------------------------------------------------------------------------------------------------
// Eval-mode BatchNorm folded into the convolution in front of it (ConvBlock2d, convolution.py:71-120, in inference
// mode): scale[c] = gamma[c] / sqrt(running_var[c] + eps), shift[c] = beta[c] - running_mean[c] * scale[c]
// (+ conv_bias[c] * scale[c] when the convolution has a bias). The packed weights are multiplied by `scale`
// (cn_pack_weights_scaled_bf16) and `shift` becomes the fused launch's bias.
// ---------------------------------------------------------------------------------------------------------------
__global__ void cn_bn_fold_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                                  const float* __restrict__ mean, const float* __restrict__ var,
                                  const float* __restrict__ conv_bias, float eps, int C, float* __restrict__ scale,
                                  float* __restrict__ shift) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float s = gamma[c] / sqrtf(var[c] + eps);
  scale[c] = s;
  shift[c] = beta[c] - mean[c] * s + (conv_bias != nullptr ? conv_bias[c] * s : 0.f);
}

extern "C" int cn_bn_fold_f32(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                              const float* conv_bias, float eps, int C, float* scale, float* shift, void* stream) {
  if (C <= 0) return CN_OK;
  if (!gamma || !beta || !running_mean || !running_var || !scale || !shift) return CN_ERR_ARG;
  CN_LAUNCH(cn_bn_fold_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, gamma, beta, running_mean,
            running_var, conv_bias, eps, C, scale, shift);
  return cn_check_launch();
}
