// Geometry of one fp32 implicit-GEMM launch (passed by value as a kernel argument), and below it the host-side
// convolution geometry that the fp32 and the bf16 contraction files share.
#pragma once
#define CN_MAX_TAPS 9
#define CN_MAX_CLASSES 16
#define CN_MAX_GROUPS 4

// One parity class of the output grid (a plain convolution has exactly one).
//   input coord = g*is + d[t],  output coord = g*os + o0
struct CnConvClass {
  int Hg, Wg;        // logical pixel grid of this class (per image)
  int oy0, ox0;
  int ntaps;
  int dy[CN_MAX_TAPS], dx[CN_MAX_TAPS], wt[CN_MAX_TAPS];  // input offsets; tap index in packed weights
  int min_dy, min_dx;
  int pitch, plane;  // LDS halo plane of this class (plane = rows * pitch <= NI*256)
  int vplane;        // 16-byte path: floats of the flattened-row image (multiple of 4)
  int rows;          // input rows staged per tile
  int tiles_per_img;
  int block_begin;   // first blockIdx.x of this class
  int grp;           // which (input, weights, bias, output) set this class works on
};

struct CnConvGeom {
  // gathered tensor [B, Cin, Hin, Win] and written tensor [B, Cout, Hout, Wout]
  int B, Cin, Hin, Win;
  int Cout, Hout, Wout;
  long xbs, ybs;  // batch strides in elements (channel stride is H*W)
  int is, os;
  int Kpad, Npad;           // packed weights [T][Kpad][Npad]
  int w_lds_off;            // float offset of the weight tile in LDS (after KC * max plane)
  int tap_lds_off;          // float offset of the per-class tap table in LDS
  int chunks_per_split;     // K-chunks (of 8 channels) per grid.z slice
  int atomic_out;           // split-K: accumulate with atomics into a pre-initialised output
  int accumulate, has_bias;
  // groups: G independent (input, weights, bias, output) sets in one launch; each class names its group
  // (CnConvClass::grp), so groups may differ in taps (dilation). shared_y: all groups sum into one output.
  int G, splits, shared_y;
  int odd_planes;      // H*W % 4 == 1: the 16-byte staging kernel runs its odd-plane variant (RP == 3)
  int want_interleave; // the launch asks for it (strided scatter); cn_plan grants it when the classes' tile counts agree
  int interleave;      // != 0: logical block l = tile * ncls + class (every class has the same number of tiles), classes in
                       // order of DESCENDING taps: the blocks of one cell tile sit next to each other (shared halo in L2) and
                       // every XCD / dispatch round gets the same mix of heavy and light parity classes
  float* part;         // split-K partial slices [(grp * splits + split)][B][Cout][Hout][Wout] (slice_stride != 0)
  long slice_stride;
  int grid_x, grid_y;  // logical grid (pixel tiles, N tiles); z = splits. Launched 1-D in XCD-aware order
  const float* gx[CN_MAX_GROUPS];
  const float* gwp[CN_MAX_GROUPS];
  const float* gbias[CN_MAX_GROUPS];
  float* gy[CN_MAX_GROUPS];
  int ncls;
  CnConvClass cls[CN_MAX_CLASSES];
};

// ---- host-side geometry shared by the fp32 (cn_conv / cn_wgrad) and the bf16 (cn_bconv / cn_bwgrad) contraction files.
// Plain C++ without HIP types: a host compiler can include this header alone (tests/conv_geom_check.cpp does).
static inline int cn_conv_out(int in, int k, int stride, int pad, int dil) {
  return (in + 2 * pad - dil * (k - 1) - 1) / stride + 1;
}
// out_pad = nn.ConvTranspose2d's output_padding
static inline int cn_convt_out(int in, int k, int stride, int pad, int out_pad) {
  return (in - 1) * stride - 2 * pad + k + out_pad;
}
static inline int cn_floordiv(int a, int b) { return (a >= 0) ? a / b : -((-a + b - 1) / b); }

// Gather form (Conv2d forward, ConvTranspose2d backward-data), input coord = o*stride + d[t]: the dense tap table,
// d = k*dil - pad, wt = ky*KW + kx. Returns the tap count KH*KW (<= CN_MAX_TAPS: the caller checks).
static inline int cn_gather_taps(int KH, int KW, int pad, int dil, int* dy, int* dx, int* wt) {
  for (int ky = 0; ky < KH; ++ky)
    for (int kx = 0; kx < KW; ++kx) {
      const int t = ky * KW + kx;
      dy[t] = ky * dil - pad; dx[t] = kx * dil - pad; wt[t] = t;
    }
  return KH * KW;
}

// Scatter form (Conv2d backward-data, ConvTranspose2d forward): out[o] += src[(o + pad - k*dil) / s] * W[k] where
// divisible. The outputs o = g*s + p of parity class p (0 <= p < s) all divide for the same taps k, so a class is a
// dense gather on its own grid of cn_parity_extent cells: input coord = g + d[t], d = (p + pad - k*dil) / s.
static inline int cn_parity_extent(int out, int p, int stride) { return (out - p + stride - 1) / stride; }

// Taps of class (py, px) in (ky, kx) order; returns their number (0: the class only receives the bias).
static inline int cn_parity_taps(int py, int px, int KH, int KW, int stride, int pad, int dil, int* dy, int* dx,
                                 int* wt) {
  int nt = 0;
  for (int ky = 0; ky < KH; ++ky) {
    const int ny = py + pad - ky * dil;
    if (((ny % stride) + stride) % stride != 0) continue;
    for (int kx = 0; kx < KW; ++kx) {
      const int nx = px + pad - kx * dil;
      if (((nx % stride) + stride) % stride != 0) continue;
      dy[nt] = cn_floordiv(ny, stride); dx[nt] = cn_floordiv(nx, stride); wt[nt] = ky * KW + kx;
      ++nt;
    }
  }
  return nt;
}

// Heavy classes first: stable insertion sort by descending ntaps (<= CN_MAX_CLASSES entries).
template <typename Class>
static inline void cn_sort_heavy_first(Class* cls, int n) {
  for (int i = 1; i < n; ++i) {
    const Class key = cls[i];
    int j = i - 1;
    while (j >= 0 && cls[j].ntaps < key.ntaps) { cls[j + 1] = cls[j]; --j; }
    cls[j + 1] = key;
  }
}
