// Per-sample training augmentation fused into the input prologue (EdgeDataset.get,
// data/datasets.py:443-488, and AugmenterModule.__call__, augment/augmenters.py:25-35):
//   v = clip(raw * scale, lo, hi)  ->  one augmentation  ->  x.clip(lo, hi), bdist.clip(0, hi), y as int64  ->  z-score
// for the nine augmenters that need no parcel labelling (augment/augmenters.py:166-330). The random CHOICES are drawn on
// the host and arrive as a plan table; only the per-element noise is generated here (counter-based, never stored), so the
// kernels keep no state. Two launches per batch: one over x, one over bdist + y. The op is uniform per block
// (blockIdx.z = sample), a block owns a band of CN_AUG_BR output rows of one plane, and every write is coalesced along W.
// A tenth op, `roll` (augment/augmenters.py:154-163, augment/augmenter_utils.py:57-108,168-193), shifts each labelled
// parcel along T by its own amount: it reads the parcel labels of cn_label_parcels_i32 (cn_parcels.hip) and a table of
// CN_AUG_PARCELS shifts per sample, and is reached through cn_augment_parcels_f32 only.
// The four time-series ops (tswarp, tsnoise, tsdrift, tspeaks; augment_time, augment/augmenter_utils.py:111-165) work on
// whole pixel series and have a kernel of their own, cn_augment_series_kernel, reached through cn_augment_series_f32 only:
// the plane kernel leaves a series sample alone, the target kernel treats it as `none`.
// The `_log_f32` entry points run the same kernels with EdgeDataset.get's log transform (data/datasets.py:481-484) in the
// final store of x (CnChipStore<true>, cn_chip_store.h); bdist and y are never transformed.
//
// Plan table: CN_AUG_PLAN_WORDS int32 words per sample
//   [0] op   [1] div   [2] top   [3] left   [4] r   [5] sigma (float bits)   [6] noise seed, low word   [7] high word
// Perlin angle tables: CN_AUG_PERLIN_FLOATS floats per sample, theta [2][r+1][r+1] then phi [2][r+1][r+1], compact.
//
// Rotations. v2.RandomRotation(degrees=[d, d]) rotates counter-clockwise by d about the image centre; for a square
// plane and d a multiple of 90 the inverse affine grid lands exactly on pixel centres, so bilinear and nearest sampling
// both reduce to the index permutation of torch.rot90(k = d / 90, dims = (-2, -1)):
//   rot90 : out[i][j] = in[j][N-1-i]      rot270 : out[i][j] = in[N-1-j][i]      rot180 : out[i][j] = in[N-1-i][N-1-j]
// (torchvision is not available to the test suite; this equivalence is argued here, the permutation itself is tested.)
// On a non-square plane the reference fills the uncovered corners with zeros; that case is refused (CN_ERR_ARG).
#include "cn_common.h"
#include "cn_chip_store.h"

#include <type_traits>

#define CN_AUG_NONE 0
#define CN_AUG_ROT90 1
#define CN_AUG_ROT180 2
#define CN_AUG_ROT270 3
#define CN_AUG_FLIPLR 4
#define CN_AUG_FLIPUD 5
#define CN_AUG_GAUSSIAN 6
#define CN_AUG_SALTPEPPER 7
#define CN_AUG_CROPRESIZE 8
#define CN_AUG_PERLIN 9
#define CN_AUG_ROLL 10
#define CN_AUG_NOPS 11                      // ops of the plane kernel
#define CN_AUG_TSWARP 11                    // the series ops: cn_augment_series_kernel, cn_augment_series_f32 only
#define CN_AUG_TSNOISE 12
#define CN_AUG_TSDRIFT 13
#define CN_AUG_TSPEAKS 14
#define CN_AUG_TMAX 64                      // longest series the series kernel holds
#define CN_AUG_SERIES_NT 256                // pixels per block of the series kernel, halved while two columns do not fit LDS

#define CN_AUG_PLAN_WORDS 8
#define CN_AUG_RMAX 10
#define CN_AUG_PARCELS 256                  // shifts per sample: the reference keeps its segments as uint8
#define CN_AUG_PERLIN_FLOATS (4 * (CN_AUG_RMAX + 1) * (CN_AUG_RMAX + 1))
#define CN_AUG_BR 32                        // output rows per block
#define CN_AUG_TILE (32 * 33)               // rotation tile, padded against bank conflicts
#define CN_AUG_MAX_LDS (64 * 1024)

// raw value -> [lo, hi] float, the first step of the prologue (same arithmetic as cn_prepare_chips_kernel)
template <typename TIn>
struct CnAugLoad {
  const TIn* p;
  float scale, lo, hi;
  __device__ __forceinline__ float operator()(long i) const {
    const float v = (float)p[i] * scale;
    return fminf(fmaxf(v, lo), hi);
  }
};

// bdist / y arrive in any of the stored dtypes; the switch is uniform over the launch
struct CnAugLoadAny {
  const void* p;
  int dtype;  // 0 f32, 1 i32, 2 i16, 3 u16
  float scale, lo, hi;
  __device__ __forceinline__ float operator()(long i) const {
    float v;
    switch (dtype) {
      case 0: v = ((const float*)p)[i]; break;
      case 1: v = (float)((const int*)p)[i]; break;
      case 2: v = (float)((const short*)p)[i]; break;
      default: v = (float)((const unsigned short*)p)[i]; break;
    }
    v *= scale;
    return fminf(fmaxf(v, lo), hi);
  }
};

struct CnAugLoadLabel {
  const void* p;
  int dtype;  // 1 i32, 2 i16, 3 u16, 4 i64
  __device__ __forceinline__ long long operator()(long i) const {
    switch (dtype) {
      case 1: return ((const int*)p)[i];
      case 2: return ((const short*)p)[i];
      case 3: return ((const unsigned short*)p)[i];
      default: return ((const long long*)p)[i];
    }
  }
};

// final clip (+ log transform) + z-score (x), final clip (bdist: m = 0, inv = 1): CnChipStore (cn_chip_store.h), shared
// with cn_edges.hip; or a plain store (labels)
struct CnAugStoreLabel {
  long long* p;
  __device__ __forceinline__ void operator()(long i, long long v) const { p[i] = v; }
  __device__ __forceinline__ const CnAugStoreLabel& values() const { return *this; }
  __device__ __forceinline__ void finish(long) const {}
};

struct CnAugCrop {
  int div, top, left;
};

// The ops every tensor of a sample goes through: none, flips, rotations, crop + resize. One plane [H][W] at `base`,
// output rows [r0, r1). V = float (bilinear resize) or long long (nearest resize). `tile` holds CN_AUG_TILE values.
template <typename V, typename Ld, typename St>
__device__ __forceinline__ void cn_aug_geometry(int op, const Ld& ld, const St& st, long base, int H, int W, int r0, int r1,
                                                CnAugCrop crop, V* tile) {
  const int tid = threadIdx.x;
  const int n = (r1 - r0) * W;
  if (op == CN_AUG_ROT90 || op == CN_AUG_ROT270) {
    // H == W == N. The block's band of output rows is a band of input COLUMNS: it goes through a 32 x 32 LDS tile so
    // that both the global reads and the global writes run along W.
    const int N = W, ii = tid & 31, ty = tid >> 5;
    for (int j0 = 0; j0 < N; j0 += 32) {
      for (int jj = ty; jj < 32; jj += 8) {
        if (r0 + ii < r1 && j0 + jj < N) {
          const long src = op == CN_AUG_ROT90 ? (long)(j0 + jj) * N + (N - 1 - (r0 + ii))
                                              : (long)(N - 1 - (j0 + jj)) * N + (r0 + ii);
          tile[jj * 33 + ii] = ld(base + src);
        }
      }
      __syncthreads();
      for (int i2 = ty; i2 < 32; i2 += 8) {  // lane = output column j0 + (tid & 31)
        if (r0 + i2 < r1 && j0 + ii < N) st(base + (long)(r0 + i2) * N + j0 + ii, tile[ii * 33 + i2]);
      }
      __syncthreads();
    }
    return;
  }
  if (op == CN_AUG_CROPRESIZE) {
    // v2.RandomCrop((H // div, W // div)) at (top, left), then v2.Resize back to (H, W). torch's scales are float32.
    const int ch = H / crop.div, cw = W / crop.div;
    const float sh = (float)ch / (float)H, sw = (float)cw / (float)W;
    const long cbase = base + (long)crop.top * W + crop.left;
    for (int idx = tid; idx < n; idx += 256) {
      const int h = r0 + idx / W, w = idx % W;
      if constexpr (std::is_same<V, float>::value) {
        // bilinear, align_corners = False: source = max((d + 0.5) * s - 0.5, 0), each step rounded to float32
        const float fy = fmaxf(__fsub_rn(__fmul_rn((float)h + 0.5f, sh), 0.5f), 0.f);
        const float fx = fmaxf(__fsub_rn(__fmul_rn((float)w + 0.5f, sw), 0.5f), 0.f);
        const int y0 = min((int)fy, ch - 1), x0 = min((int)fx, cw - 1);
        const int y1 = min(y0 + 1, ch - 1), x1 = min(x0 + 1, cw - 1);
        const float ly = fy - (float)y0, lx = fx - (float)x0;
        const float hy = 1.f - ly, hx = 1.f - lx;
        const float v00 = ld(cbase + (long)y0 * W + x0), v01 = ld(cbase + (long)y0 * W + x1);
        const float v10 = ld(cbase + (long)y1 * W + x0), v11 = ld(cbase + (long)y1 * W + x1);
        st.values()(base + (long)h * W + w, hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11));
      } else {
        // nearest: source = min(floor(d * s), size - 1) with the float32 product
        const int y0 = min((int)floorf(__fmul_rn((float)h, sh)), ch - 1);
        const int x0 = min((int)floorf(__fmul_rn((float)w, sw)), cw - 1);
        st(base + (long)h * W + w, ld(cbase + (long)y0 * W + x0));
      }
    }
    if constexpr (std::is_same<V, float>::value)
      for (int idx = tid; idx < n; idx += 256) st.finish(base + (long)(r0 + idx / W) * W + idx % W);
    return;
  }
  const bool fh = op == CN_AUG_FLIPUD || op == CN_AUG_ROT180, fw = op == CN_AUG_FLIPLR || op == CN_AUG_ROT180;
  if (!fh && !fw) {  // none: the band is one contiguous run
    const long b0 = base + (long)r0 * W;
    for (int idx = tid; idx < n; idx += 256) st(b0 + idx, ld(b0 + idx));
    return;
  }
  for (int idx = tid; idx < n; idx += 256) {
    const int h = r0 + idx / W, w = idx % W;
    const int hs = fh ? H - 1 - h : h, ws = fw ? W - 1 - w : w;
    st(base + (long)h * W + w, ld(base + (long)hs * W + ws));
  }
}

// Plan rows come from the host, which has validated them (cn_augment_chips_f32); a row that does not fit the plane is
// still never followed out of bounds: it degrades to `none`.
__device__ __forceinline__ int cn_aug_checked_op(const int* __restrict__ row, int H, int W, bool have_perlin, bool have_parcels,
                                                 CnAugCrop& crop) {
  int op = row[0];
  crop.div = row[1]; crop.top = row[2]; crop.left = row[3];
  if (op < 0 || op >= CN_AUG_NOPS) op = CN_AUG_NONE;
  if ((op == CN_AUG_ROT90 || op == CN_AUG_ROT270) && H != W) op = CN_AUG_NONE;
  if (op == CN_AUG_CROPRESIZE) {
    const int ch = crop.div > 0 ? H / crop.div : 0, cw = crop.div > 0 ? W / crop.div : 0;
    if (ch < 1 || cw < 1 || crop.top < 0 || crop.left < 0 || crop.top + ch > H || crop.left + cw > W) op = CN_AUG_NONE;
  }
  if (op == CN_AUG_PERLIN) {
    const int r = row[4];
    if (!have_perlin || r < 1 || r > CN_AUG_RMAX || H % r != 0 || W % r != 0) op = CN_AUG_NONE;
  }
  if (op == CN_AUG_ROLL && !have_parcels) op = CN_AUG_NONE;
  if (op == CN_AUG_GAUSSIAN && (H < 2 || W < 2 || (CN_AUG_BR + 2) * (W + 2) * (int)sizeof(float) > CN_AUG_MAX_LDS)) op = CN_AUG_NONE;
  return op;
}

// grid (bands, C * T, B); dynamic LDS: max(rotation tile, blur band, perlin gradients, parcel shifts)
template <typename TIn, bool LOG>
__global__ __launch_bounds__(256) void cn_augment_x_kernel(const TIn* __restrict__ x, float* __restrict__ out,
                                                          const int* __restrict__ plan, const float* __restrict__ perlin,
                                                          const int* __restrict__ labels, const int* __restrict__ parcel,
                                                          const float* __restrict__ mean, const float* __restrict__ stdv,
                                                          int T, int H, int W, float scale, float lo, float hi,
                                                          CnChipLog<LOG> lg) {
  extern __shared__ float smem[];
  const int tid = threadIdx.x, plane = blockIdx.y, b = blockIdx.z;
  const int c = plane / T, t = plane - c * T;
  const int r0 = blockIdx.x * CN_AUG_BR, r1 = min(r0 + CN_AUG_BR, H);
  const int* row = plan + (long)b * CN_AUG_PLAN_WORDS;
  if (row[0] >= CN_AUG_TSWARP && row[0] <= CN_AUG_TSPEAKS) return;  // cn_augment_series_kernel writes this sample
  CnAugCrop crop;
  const int op = cn_aug_checked_op(row, H, W, perlin != nullptr, labels != nullptr && parcel != nullptr, crop);
  const long HW = (long)H * W;
  const long base = ((long)b * gridDim.y + plane) * HW;
  const CnAugLoad<TIn> ld{x, scale, lo, hi};
  const CnChipStore<LOG> st{out, lo, hi, mean ? mean[c] : 0.f, stdv ? 1.0f / stdv[c] : 1.f, lg};
  const auto sv = st.values();  // the ops that compute in front of the store: see CnChipStore::values
  const int n = (r1 - r0) * W;

  if (op == CN_AUG_GAUSSIAN) {
    // v2.GaussianBlur(kernel_size=3, sigma): taps exp(-0.5 (k / sigma)^2), k = -1, 0, 1, normalised; reflect padding.
    // The band and its one-pixel halo are staged once; each output reads its 3 x 3 neighbourhood from LDS.
    const float sigma = __int_as_float(row[5]);
    const float e = expf(-0.5f / (sigma * sigma));
    const float k1 = 1.0f / (1.0f + 2.0f * e), k0 = e * k1;
    const int SW = W + 2, rows = r1 - r0 + 2;
    for (int idx = tid; idx < rows * SW; idx += 256) {
      int h = r0 - 1 + idx / SW, w = idx % SW - 1;
      h = h < 0 ? -h : (h >= H ? 2 * H - 2 - h : h);
      w = w < 0 ? -w : (w >= W ? 2 * W - 2 - w : w);
      smem[idx] = ld(base + (long)h * W + w);
    }
    __syncthreads();
    for (int idx = tid; idx < n; idx += 256) {
      const int hl = idx / W, w = idx % W;
      const float* p = smem + hl * SW + w;  // top-left of the 3 x 3 window
      const float a = k0 * p[0] + k1 * p[1] + k0 * p[2];
      const float m = k0 * p[SW] + k1 * p[SW + 1] + k0 * p[SW + 2];
      const float z = k0 * p[2 * SW] + k1 * p[2 * SW + 1] + k0 * p[2 * SW + 2];
      sv(base + (long)(r0 + hl) * W + w, k0 * a + k1 * m + k0 * z);
    }
    for (int idx = tid; idx < n; idx += 256) st.finish(base + (long)r0 * W + idx);
    return;
  }
  if (op == CN_AUG_SALTPEPPER) {
    // x + 0.01 * n, n standard normal by Box-Muller on two 24-bit uniforms of the element's counter
    // (u1 in (0, 1], u2 in [0, 1)); accurate logf / sqrtf / cosf: the test tolerance relies on them.
    const unsigned long long seed = ((unsigned long long)(unsigned)row[7] << 32) | (unsigned)row[6];
    for (int idx = tid; idx < n; idx += 256) {
      const long off = (long)r0 * W + idx;
      const unsigned long long i = (unsigned long long)(plane * HW + off);
      const float u1 = (float)((cn_splitmix64(seed + 2ull * i) >> 40) + 1ull) * 0x1p-24f;
      const float u2 = (float)(cn_splitmix64(seed + 2ull * i + 1ull) >> 40) * 0x1p-24f;
      const float nrm = sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
      sv(base + off, ld(base + off) + 0.01f * nrm);
    }
    for (int idx = tid; idx < n; idx += 256) st.finish(base + (long)r0 * W + idx);
    return;
  }
  if (op == CN_AUG_PERLIN) {
    // generate_perlin_noise_3d(shape=(T, H, W), res=(1, r, r), out_range=(-0.03, 0.03)), augmenter_utils.py:211-360:
    // corner gradients (sin phi cos theta, sin phi sin theta, cos phi), quintic interpolant, 0.06 * value.
    const int r = row[4], R1 = r + 1, ng = 2 * R1 * R1;
    const float* tab = perlin + (long)b * CN_AUG_PERLIN_FLOATS;
    if (tid < ng) {
      const float th = tab[tid], ph = tab[ng + tid];
      const float sp = sinf(ph);
      smem[3 * tid] = sp * cosf(th);
      smem[3 * tid + 1] = sp * sinf(th);
      smem[3 * tid + 2] = cosf(ph);
    }
    __syncthreads();
    const int dH = H / r, dW = W / r;
    const float ft = (float)t / (float)T;
    const float qt = ft * ft * ft * (ft * (ft * 6.f - 15.f) + 10.f);
    for (int idx = tid; idx < n; idx += 256) {
      const int h = r0 + idx / W, w = idx % W;
      const int ih = h / dH, iw = w / dW;
      const float fh = (float)(h - ih * dH) / (float)dH, fw = (float)(w - iw * dW) / (float)dW;
      const float qh = fh * fh * fh * (fh * (fh * 6.f - 15.f) + 10.f);
      const float qw = fw * fw * fw * (fw * (fw * 6.f - 15.f) + 10.f);
      float nv[2][2][2];
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int d = 0; d < 2; ++d) {
            const float* g = smem + 3 * ((k * R1 + ih + a) * R1 + iw + d);
            nv[k][a][d] = (ft - (float)k) * g[0] + (fh - (float)a) * g[1] + (fw - (float)d) * g[2];
          }
      const float n00 = nv[0][0][0] * (1.f - qt) + qt * nv[1][0][0];
      const float n10 = nv[0][1][0] * (1.f - qt) + qt * nv[1][1][0];
      const float n01 = nv[0][0][1] * (1.f - qt) + qt * nv[1][0][1];
      const float n11 = nv[0][1][1] * (1.f - qt) + qt * nv[1][1][1];
      const float n0 = (1.f - qh) * n00 + qh * n10;
      const float n1 = (1.f - qh) * n01 + qh * n11;
      const long off = (long)h * W + w;
      sv(base + off, ld(base + off) + 0.06f * ((1.f - qw) * n0 + qw * n1));
    }
    for (int idx = tid; idx < n; idx += 256) st.finish(base + (long)r0 * W + idx);
    return;
  }
  if (op == CN_AUG_ROLL) {
    // torch.roll(xseg, s, dims=2) where segments == prop.label: out[t] = in[(t - s) mod T], s the shift of the pixel's
    // parcel. The segments are uint8 in the reference, so label k shares the shift of k & 255 and 256, 512, ... stay put.
    // A shift that does not fit T degrades to 0 (the host has refused it already).
    int* shift = (int*)smem;
    if (tid < CN_AUG_PARCELS) {
      const int s = parcel[(long)b * CN_AUG_PARCELS + tid];
      shift[tid] = (tid == 0 || s <= -T || s >= T) ? 0 : s;
    }
    __syncthreads();
    const long lbase = (long)b * HW, cbase = base - (long)t * HW;  // plane t = 0 of this channel
    for (int idx = tid; idx < n; idx += 256) {
      const long off = (long)r0 * W + idx;
      int ts = t - shift[labels[lbase + off] & (CN_AUG_PARCELS - 1)];
      ts += ts < 0 ? T : 0;
      ts -= ts >= T ? T : 0;
      st(base + off, ld(cbase + (long)ts * HW + off));
    }
    return;
  }
  cn_aug_geometry<float>(op, ld, st, base, H, W, r0, r1, crop, smem);
}

// grid (bands, 2, B): blockIdx.y = 0 -> bdist (same geometry as x, no noise / blur, clip to [0, hi]), 1 -> labels
__global__ __launch_bounds__(256) void cn_augment_target_kernel(const void* __restrict__ bdist, int bdtype,
                                                               const void* __restrict__ y, int ydtype,
                                                               float* __restrict__ bdist_out, long long* __restrict__ y_out,
                                                               const int* __restrict__ plan, int H, int W, float scale,
                                                               float lo, float hi) {
  __shared__ long long tile[CN_AUG_TILE];
  const int b = blockIdx.z;
  const int r0 = blockIdx.x * CN_AUG_BR, r1 = min(r0 + CN_AUG_BR, H);
  CnAugCrop crop;
  int op = cn_aug_checked_op(plan + (long)b * CN_AUG_PLAN_WORDS, H, W, true, true, crop);
  if (op == CN_AUG_GAUSSIAN || op == CN_AUG_SALTPEPPER || op == CN_AUG_PERLIN || op == CN_AUG_ROLL) op = CN_AUG_NONE;  // x only
  const long base = (long)b * H * W;
  if (blockIdx.y == 0) {
    if (bdist == nullptr) return;
    const CnAugLoadAny ld{bdist, bdtype, scale, lo, hi};
    const CnChipStore<false> st{bdist_out, 0.f, hi, 0.f, 1.f, {}};  // bdist is never log-transformed
    cn_aug_geometry<float>(op, ld, st, base, H, W, r0, r1, crop, (float*)tile);
  } else {
    const CnAugLoadLabel ld{y, ydtype};
    const CnAugStoreLabel st{y_out};
    cn_aug_geometry<long long>(op, ld, st, base, H, W, r0, r1, crop, tile);
  }
}

// The four time-series ops of the parcel augmenters (augment_time, augment/augmenter_utils.py:111-165, with tsaug's
// TimeWarp / Drift / AddNoise): tswarp, tsnoise, tsdrift, tspeaks. The random CURVES are drawn on the host, one set per
// parcel slot k = label & 255 (the reference's uint8 segments, as in `roll`), and arrive as a packed table per series
// sample (`row` of them, `rows[row]` = the sample):
//   pos [256][T] source times in [0, T-1]   drift [256][C][T]   nscale [256]      slot 0 holds the identity
// A thread owns one pixel of one channel and keeps its whole series in a column of LDS (element t at [t * tile + tid]:
// consecutive lanes, consecutive banks), a second column holds the result while its range is taken. With v the
// prologue's load:
//   u = tspeaks && k != 0 ? concat(resize(v, T / 2), resize(v, T - T / 2)) : v (F.interpolate, linear, align_corners=False)
//   w[t] = warp ? u[j] + (p - j) (u[j1] - u[j]),  p = pos[k][t], j = min(floor p, T-1), j1 = min(j + 1, T-1)  :  u[t]
//   d[t] = w[t] + drift[k][c][t] (max w - min w)                                (tsdrift only)
//   e[t] = d[t] + n nscale[k] (max d - min d)                                   (where nscale[k] > 0; n as in saltpepper)
//   out[t] = store(clip(e[t], 0, 1))
// With identity tables every step returns its input bit for bit (p - j = 0, drift = 0), so such a pixel equals
// cn_prepare_chips_f32. A thread touches its own columns only: there is no barrier. grid (pixel tiles, C, series rows).
template <typename TIn, bool LOG>
__global__ __launch_bounds__(CN_AUG_SERIES_NT) void cn_augment_series_kernel(
    const TIn* __restrict__ x, float* __restrict__ out, const int* __restrict__ plan, const int* __restrict__ labels,
    const float* __restrict__ tables, const int* __restrict__ rows, const float* __restrict__ mean,
    const float* __restrict__ stdv, int B, int T, int H, int W, float scale, float lo, float hi, CnChipLog<LOG> lg) {
  extern __shared__ float smem[];
  const int tile = blockDim.x, tid = threadIdx.x, C = gridDim.y, c = blockIdx.y;
  const int b = rows[blockIdx.z];
  const long HW = (long)H * W, pix = (long)blockIdx.x * tile + tid;
  if (b < 0 || b >= B || pix >= HW) return;
  const int* row = plan + (long)b * CN_AUG_PLAN_WORDS;
  const int op = row[0];
  const CnAugLoad<TIn> ld{x, scale, lo, hi};
  const CnChipStore<LOG> st{out, lo, hi, mean ? mean[c] : 0.f, stdv ? 1.0f / stdv[c] : 1.f, lg};
  const long base = ((long)b * C + c) * T * HW + pix;
  float* v = smem + tid;
  float* e = smem + T * tile + tid;
#pragma unroll 4
  for (int t = 0; t < T; ++t) v[t * tile] = ld(base + (long)t * HW);  // several loads in flight

  const int k = labels[(long)b * HW + pix] & (CN_AUG_PARCELS - 1);
  const bool peaks = op == CN_AUG_TSPEAKS && k != 0;  // slot 0 is no prop: augment_time never sees those pixels
  const bool warp = op == CN_AUG_TSWARP || op == CN_AUG_TSPEAKS;
  const float* tab = tables + (long)blockIdx.z * CN_AUG_PARCELS * (T + C * T + 1);
  const float* pos = tab + k * T;
  const float* drift = tab + CN_AUG_PARCELS * T + (k * C + c) * T;
  const float nscale = tab[CN_AUG_PARCELS * T * (1 + C) + k];

  // u[i]: the series itself, or for tspeaks its two halves, each the whole series resized
  const int Ta = T / 2;
  const float sa = (float)T / (float)Ta, sb = (float)T / (float)(T - Ta);
  auto u_at = [&](int i) -> float {
    if (!peaks) return v[i * tile];
    const int ii = i < Ta ? i : i - Ta;
    const float s = fmaxf(((float)ii + 0.5f) * (i < Ta ? sa : sb) - 0.5f, 0.f);
    const int i0 = min((int)s, T - 1), i1 = min(i0 + 1, T - 1);
    const float l = s - (float)i0;
    return (1.f - l) * v[i0 * tile] + l * v[i1 * tile];
  };
  float mn = INFINITY, mx = -INFINITY;
  for (int t = 0; t < T; ++t) {
    float w;
    if (warp) {
      // the host has refused a source time outside [0, T-1]; it is clamped all the same, so that no column is left
      const float p = fminf(fmaxf(pos[t], 0.f), (float)(T - 1));
      const int j = min((int)p, T - 1), j1 = min(j + 1, T - 1);
      const float a = u_at(j);
      w = a + (p - (float)j) * (u_at(j1) - a);
    } else {
      w = v[t * tile];
    }
    e[t * tile] = w;
    mn = fminf(mn, w);
    mx = fmaxf(mx, w);
  }
  if (op == CN_AUG_TSDRIFT) {
    const float r = mx - mn;
    mn = INFINITY;
    mx = -INFINITY;
    for (int t = 0; t < T; ++t) {
      const float d = e[t * tile] + drift[t] * r;
      e[t * tile] = d;
      mn = fminf(mn, d);
      mx = fmaxf(mx, d);
    }
  }
  if (nscale > 0.f) {  // the counter and the Box-Muller step of saltpepper
    const unsigned long long seed = ((unsigned long long)(unsigned)row[7] << 32) | (unsigned)row[6];
    const float amp = nscale * (mx - mn);
    for (int t = 0; t < T; ++t) {
      const unsigned long long i = (unsigned long long)(((long)c * T + t) * HW + pix);
      const float u1 = (float)((cn_splitmix64(seed + 2ull * i) >> 40) + 1ull) * 0x1p-24f;
      const float u2 = (float)(cn_splitmix64(seed + 2ull * i + 1ull) >> 40) * 0x1p-24f;
      const float nrm = sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
      e[t * tile] += nrm * amp;
    }
  }
  for (int t = 0; t < T; ++t) st(base + (long)t * HW, fminf(fmaxf(e[t * tile], 0.f), 1.f));
}

// x: [B][C][T][H][W] raw (xdtype: 0 f32, 1 i32, 2 i16, 3 u16) -> x_out fp32, z-scored (mean / stdv nullable);
// bdist: [B][H][W] raw (bdtype as xdtype; nullable together with bdist_out) -> bdist_out fp32 in [0, hi];
// y: [B][H][W] labels (ydtype: 1 i32, 2 i16, 3 u16, 4 i64) -> y_out int64.
// plan_host / plan_dev: the SAME [B][CN_AUG_PLAN_WORDS] table in host memory (validated here, before anything is
// launched) and in device memory (read by the kernels); perlin_dev: [B][CN_AUG_PERLIN_FLOATS], nullable when no sample
// is `perlin`. labels_dev: [B][H][W] parcel labels (cn_label_parcels_i32); parcel_host / parcel_dev: the SAME
// [B][CN_AUG_PARCELS] table of shifts in host and in device memory; all three nullable when no sample is `roll`.
// series_host / series_dev: the SAME [nrows][256 * (T + C * T + 1)] packed tables of the series samples (pos, drift,
// nscale; see cn_augment_series_kernel) in host and in device memory; rows_host / rows_dev: the SAME [nrows] sample
// indices, increasing, one per series sample; all nullable with nrows = 0, and a series op is then an unknown op.
// logt: EdgeDataset.get's log transform (data/datasets.py:481-484) in the final store of x, w = max(log(v * gain + 1), floor)
// between the last clip and the z-score (CnChipStore<true>); bdist and y are never transformed.
// Two launches, three with a series sample; no allocation, no synchronisation.
static int cn_augment_run(const void* x, int xdtype, const void* bdist, int bdtype, const void* y, int ydtype,
                          float* x_out, float* bdist_out, long long* y_out, const int* plan_host, const int* plan_dev,
                          const float* perlin_dev, const int* labels_dev, const int* parcel_host, const int* parcel_dev,
                          const float* series_host, const float* series_dev, const int* rows_host, const int* rows_dev,
                          int nrows, const float* mean, const float* stdv, int B, int C, int T, int H, int W,
                          float scale, float lo, float hi, bool logt, float gain, float floor, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (logt && !(gain > 0.f)) return CN_ERR_ARG;
  if (B <= 0 || C <= 0 || T <= 0 || H <= 0 || W <= 0) return CN_OK;
  if (x == nullptr || x_out == nullptr || y == nullptr || y_out == nullptr || plan_host == nullptr || plan_dev == nullptr) return CN_ERR_ARG;
  if ((bdist == nullptr) != (bdist_out == nullptr)) return CN_ERR_ARG;
  if (xdtype < 0 || xdtype > 3 || (bdist != nullptr && (bdtype < 0 || bdtype > 3)) || ydtype < 1 || ydtype > 4) return CN_ERR_ARG;
  if ((long)C * T > 65535 || B > 65535) return CN_ERR_ARG;
  if (nrows < 0 || nrows > B) return CN_ERR_ARG;
  if (nrows > 0) {
    if (series_host == nullptr || series_dev == nullptr || rows_host == nullptr || rows_dev == nullptr || labels_dev == nullptr) return CN_ERR_ARG;
    if (T < 2 || T > CN_AUG_TMAX) return CN_ERR_ARG;
    const long per_row = (long)CN_AUG_PARCELS * ((long)T + (long)C * T + 1);
    for (int r = 0; r < nrows; ++r) {
      const int b = rows_host[r];
      if (b < 0 || b >= B || (r > 0 && b <= rows_host[r - 1])) return CN_ERR_ARG;
      const int op = plan_host[(long)b * CN_AUG_PLAN_WORDS];
      if (op < CN_AUG_TSWARP || op > CN_AUG_TSPEAKS) return CN_ERR_ARG;
      const float* pos = series_host + r * per_row;
      const float* drift = pos + CN_AUG_PARCELS * T;
      const float* nscale = drift + (long)CN_AUG_PARCELS * C * T;
      for (long i = 0; i < (long)CN_AUG_PARCELS * T; ++i)
        if (!(pos[i] >= 0.f && pos[i] <= (float)(T - 1))) return CN_ERR_ARG;  // refuses NaN too
      for (long i = 0; i < (long)CN_AUG_PARCELS * C * T; ++i)
        if (!(fabsf(drift[i]) <= 3.4028234663852886e38f)) return CN_ERR_ARG;
      for (int k = 0; k < CN_AUG_PARCELS; ++k)
        if (!(nscale[k] >= 0.f && nscale[k] <= 3.4028234663852886e38f)) return CN_ERR_ARG;
      for (int t = 0; t < T; ++t)  // slot 0: background, and parcels 256, 512, ...
        if (pos[t] != (float)t) return CN_ERR_ARG;
      for (int i = 0; i < C * T; ++i)
        if (drift[i] != 0.f) return CN_ERR_ARG;
      if (nscale[0] != 0.f) return CN_ERR_ARG;
    }
  }
  bool blur = false;
  int nseries = 0;
  for (int b = 0; b < B; ++b) {
    const int* row = plan_host + (long)b * CN_AUG_PLAN_WORDS;
    switch (row[0]) {
      case CN_AUG_TSWARP: case CN_AUG_TSNOISE: case CN_AUG_TSDRIFT: case CN_AUG_TSPEAKS:
        ++nseries;  // every one of them must own a row of the tables: the rows are distinct series samples, so count
        break;
      case CN_AUG_NONE: case CN_AUG_ROT180: case CN_AUG_FLIPLR: case CN_AUG_FLIPUD: case CN_AUG_SALTPEPPER: break;
      case CN_AUG_ROT90: case CN_AUG_ROT270:
        if (H != W) return CN_ERR_ARG;
        break;
      case CN_AUG_GAUSSIAN: {
        float sigma;
        __builtin_memcpy(&sigma, &row[5], sizeof(float));
        if (!(sigma > 0.f) || H < 2 || W < 2) return CN_ERR_ARG;
        blur = true;
        break;
      }
      case CN_AUG_CROPRESIZE: {
        const int div = row[1], top = row[2], left = row[3];
        if (div <= 0) return CN_ERR_ARG;
        const int ch = H / div, cw = W / div;
        if (ch < 1 || cw < 1 || top < 0 || left < 0 || top + ch > H || left + cw > W) return CN_ERR_ARG;
        break;
      }
      case CN_AUG_PERLIN: {
        const int r = row[4];
        if (perlin_dev == nullptr || r < 1 || r > CN_AUG_RMAX || H % r != 0 || W % r != 0) return CN_ERR_ARG;
        break;
      }
      case CN_AUG_ROLL: {
        if (labels_dev == nullptr || parcel_host == nullptr || parcel_dev == nullptr) return CN_ERR_ARG;
        const int* tab = parcel_host + (long)b * CN_AUG_PARCELS;
        if (tab[0] != 0) return CN_ERR_ARG;
        for (int k = 1; k < CN_AUG_PARCELS; ++k)
          if (tab[k] <= -T || tab[k] >= T) return CN_ERR_ARG;
        break;
      }
      default: return CN_ERR_ARG;
    }
  }
  if (nseries != nrows) return CN_ERR_ARG;
  size_t lds = CN_AUG_TILE * sizeof(float);  // covers the perlin gradients (2 * 11 * 11 * 3 floats) and the parcel shifts too
  if (blur) {
    const size_t band = (size_t)(CN_AUG_BR + 2) * (W + 2) * sizeof(float);
    if (band > CN_AUG_MAX_LDS) return CN_ERR_LDS;
    if (band > lds) lds = band;
  }
  const int bands = cn_cdiv(H, CN_AUG_BR);
  const dim3 grid(bands, C * T, B), block(256);
  const CnChipLog<true> lg{gain, floor};
#define CN_AUG_X(TY, LOG, LG) CN_LAUNCH((cn_augment_x_kernel<TY, LOG>), grid, block, lds, stream, (const TY*)x, x_out, plan_dev, \
                                   perlin_dev, labels_dev, parcel_dev, mean, stdv, T, H, W, scale, lo, hi, LG)
#define CN_AUG_X2(TY) do { if (logt) CN_AUG_X(TY, true, lg); else CN_AUG_X(TY, false, CnChipLog<false>{}); } while (0)
  switch (xdtype) {
    case 0: CN_AUG_X2(float); break;
    case 1: CN_AUG_X2(int); break;
    case 2: CN_AUG_X2(short); break;
    default: CN_AUG_X2(unsigned short); break;
  }
#undef CN_AUG_X2
#undef CN_AUG_X
  int rc = cn_check_launch();
  if (rc != CN_OK) return rc;
  if (nrows > 0) {
    // two columns of T floats per pixel: 256 pixels up to T = 32, 128 beyond
    const int nt = 2 * T * CN_AUG_SERIES_NT * (int)sizeof(float) <= CN_AUG_MAX_LDS ? CN_AUG_SERIES_NT : CN_AUG_SERIES_NT / 2;
    const size_t slds = (size_t)2 * T * nt * sizeof(float);
    const dim3 sgrid(cn_cdiv((long)H * W, nt), C, nrows), sblock(nt);
#define CN_AUG_S(TY, LOG, LG) CN_LAUNCH((cn_augment_series_kernel<TY, LOG>), sgrid, sblock, slds, stream, (const TY*)x, x_out, \
                                   plan_dev, labels_dev, series_dev, rows_dev, mean, stdv, B, T, H, W, scale, lo, hi, LG)
#define CN_AUG_S2(TY) do { if (logt) CN_AUG_S(TY, true, lg); else CN_AUG_S(TY, false, CnChipLog<false>{}); } while (0)
    switch (xdtype) {
      case 0: CN_AUG_S2(float); break;
      case 1: CN_AUG_S2(int); break;
      case 2: CN_AUG_S2(short); break;
      default: CN_AUG_S2(unsigned short); break;
    }
#undef CN_AUG_S2
#undef CN_AUG_S
    rc = cn_check_launch();
    if (rc != CN_OK) return rc;
  }
  CN_LAUNCH(cn_augment_target_kernel, dim3(bands, 2, B), block, 0, stream, bdist, bdtype, y, ydtype, bdist_out, y_out,
            plan_dev, H, W, scale, lo, hi);
  return cn_check_launch();
}

// The ten ops of the plane kernel: a series row is CN_ERR_ARG here, as every unknown op.
extern "C" int cn_augment_parcels_f32(const void* x, int xdtype, const void* bdist, int bdtype, const void* y, int ydtype,
                                      float* x_out, float* bdist_out, long long* y_out, const int* plan_host,
                                      const int* plan_dev, const float* perlin_dev, const int* labels_dev,
                                      const int* parcel_host, const int* parcel_dev, const float* mean, const float* stdv,
                                      int B, int C, int T, int H, int W, float scale, float lo, float hi, void* stream_) {
  return cn_augment_run(x, xdtype, bdist, bdtype, y, ydtype, x_out, bdist_out, y_out, plan_host, plan_dev, perlin_dev,
                        labels_dev, parcel_host, parcel_dev, nullptr, nullptr, nullptr, nullptr, 0, mean, stdv, B, C, T, H, W,
                        scale, lo, hi, false, 0.f, 0.f, stream_);
}

// cn_augment_parcels_f32 plus the four series ops (11 tswarp, 12 tsnoise, 13 tsdrift, 14 tspeaks). CN_ERR_ARG with
// nothing launched: T outside [2, 64]; a source time that is not in [0, T-1]; a drift or noise scale that is not finite,
// a negative noise scale; slot 0 not the identity; a series row without labels or without its row of the tables.
extern "C" int cn_augment_series_f32(const void* x, int xdtype, const void* bdist, int bdtype, const void* y, int ydtype,
                                     float* x_out, float* bdist_out, long long* y_out, const int* plan_host,
                                     const int* plan_dev, const float* perlin_dev, const int* labels_dev,
                                     const int* parcel_host, const int* parcel_dev, const float* series_host,
                                     const float* series_dev, const int* rows_host, const int* rows_dev, int nrows,
                                     const float* mean, const float* stdv, int B, int C, int T, int H, int W, float scale,
                                     float lo, float hi, void* stream_) {
  return cn_augment_run(x, xdtype, bdist, bdtype, y, ydtype, x_out, bdist_out, y_out, plan_host, plan_dev, perlin_dev,
                        labels_dev, parcel_host, parcel_dev, series_host, series_dev, rows_host, rows_dev, nrows, mean, stdv,
                        B, C, T, H, W, scale, lo, hi, false, 0.f, 0.f, stream_);
}

// The nine ops that need no parcel labelling: a `roll` row is CN_ERR_ARG here, as every unknown op.
extern "C" int cn_augment_chips_f32(const void* x, int xdtype, const void* bdist, int bdtype, const void* y, int ydtype,
                                    float* x_out, float* bdist_out, long long* y_out, const int* plan_host,
                                    const int* plan_dev, const float* perlin_dev, const float* mean, const float* stdv,
                                    int B, int C, int T, int H, int W, float scale, float lo, float hi, void* stream_) {
  return cn_augment_parcels_f32(x, xdtype, bdist, bdtype, y, ydtype, x_out, bdist_out, y_out, plan_host, plan_dev, perlin_dev,
                                nullptr, nullptr, nullptr, mean, stdv, B, C, T, H, W, scale, lo, hi, stream_);
}

// The three entry points above with EdgeDataset.get's log transform (data/datasets.py:481-484) in the final store of x,
// between the last clip and the z-score; bdist and y come out as from the plain entries. log_gain <= 0 is CN_ERR_ARG.
extern "C" int cn_augment_series_log_f32(const void* x, int xdtype, const void* bdist, int bdtype, const void* y, int ydtype,
                                         float* x_out, float* bdist_out, long long* y_out, const int* plan_host,
                                         const int* plan_dev, const float* perlin_dev, const int* labels_dev,
                                         const int* parcel_host, const int* parcel_dev, const float* series_host,
                                         const float* series_dev, const int* rows_host, const int* rows_dev, int nrows,
                                         const float* mean, const float* stdv, int B, int C, int T, int H, int W,
                                         float scale, float lo, float hi, float log_gain, float log_floor, void* stream_) {
  return cn_augment_run(x, xdtype, bdist, bdtype, y, ydtype, x_out, bdist_out, y_out, plan_host, plan_dev, perlin_dev,
                        labels_dev, parcel_host, parcel_dev, series_host, series_dev, rows_host, rows_dev, nrows, mean, stdv,
                        B, C, T, H, W, scale, lo, hi, true, log_gain, log_floor, stream_);
}

extern "C" int cn_augment_parcels_log_f32(const void* x, int xdtype, const void* bdist, int bdtype, const void* y, int ydtype,
                                          float* x_out, float* bdist_out, long long* y_out, const int* plan_host,
                                          const int* plan_dev, const float* perlin_dev, const int* labels_dev,
                                          const int* parcel_host, const int* parcel_dev, const float* mean,
                                          const float* stdv, int B, int C, int T, int H, int W, float scale, float lo,
                                          float hi, float log_gain, float log_floor, void* stream_) {
  return cn_augment_series_log_f32(x, xdtype, bdist, bdtype, y, ydtype, x_out, bdist_out, y_out, plan_host, plan_dev,
                                   perlin_dev, labels_dev, parcel_host, parcel_dev, nullptr, nullptr, nullptr, nullptr, 0,
                                   mean, stdv, B, C, T, H, W, scale, lo, hi, log_gain, log_floor, stream_);
}

extern "C" int cn_augment_chips_log_f32(const void* x, int xdtype, const void* bdist, int bdtype, const void* y, int ydtype,
                                        float* x_out, float* bdist_out, long long* y_out, const int* plan_host,
                                        const int* plan_dev, const float* perlin_dev, const float* mean, const float* stdv,
                                        int B, int C, int T, int H, int W, float scale, float lo, float hi, float log_gain,
                                        float log_floor, void* stream_) {
  return cn_augment_parcels_log_f32(x, xdtype, bdist, bdtype, y, ydtype, x_out, bdist_out, y_out, plan_host, plan_dev,
                                    perlin_dev, nullptr, nullptr, nullptr, mean, stdv, B, C, T, H, W, scale, lo, hi,
                                    log_gain, log_floor, stream_);
}
