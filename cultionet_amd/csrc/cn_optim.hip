// Fused optimizer step over the flat parameter / gradient buffers (gfx950, HBM-bound).
//
// Reference: torch.optim.AdamW(lr, weight_decay, eps, betas=(0.9, 0.98)) configured at
// /root/reference/src/cultionet/models/lightning.py:622-629 and gradient_clip_val=1.0
// (norm clipping) at /root/reference/src/cultionet/model.py:84,173.
// All parameters live in ONE contiguous fp32 buffer (and so do grads, exp_avg, exp_avg_sq), so the
// whole step is two launches: a sum-of-squares reduction and the update. The clip coefficient is
// computed on the device from the reduced norm -- no host synchronisation.
#include "cn_common.h"

__global__ __launch_bounds__(256) void cn_sumsq_kernel(const float* __restrict__ g, long n, double* __restrict__ out) {
  __shared__ double scratch[4];
  double s = 0.0;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float v = g[i];
    s += (double)v * v;
  }
  s = cn_block_sum<double, 256>(s, scratch);
  if (threadIdx.x == 0) atomicAdd(out, s);
}

// out[0] += sum g^2 (zeroed here first)
extern "C" int cn_grad_sumsq_f32(const float* g, long n, double* out, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (hipMemsetAsync(out, 0, sizeof(double), stream) != hipSuccess) return CN_ERR_LAUNCH;
  if (n <= 0) return CN_OK;
  long bx = (n + 2047) / 2048;
  if (bx > 1024) bx = 1024;
  CN_LAUNCH(cn_sumsq_kernel, dim3((unsigned)bx), dim3(256), 0, stream, g, n, out);
  return cn_check_launch();
}

// torch.optim.AdamW single-tensor semantics (amsgrad=False, maximize=False):
//   p *= 1 - lr*wd ; m = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g*g
//   p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
// g is first scaled by grad_scale (e.g. 1/world_size) and by the clip coefficient
//   min(1, max_norm / (sqrt(sumsq)*grad_scale + 1e-6))   when sumsq != nullptr  (clip_grad_norm_).
__global__ __launch_bounds__(256) void cn_adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                      float* __restrict__ m, float* __restrict__ v, long n, float lr,
                                                      float b1, float b2, float eps, float wd, float bc1,
                                                      float bc2_sqrt, float grad_scale, const double* sumsq,
                                                      float max_norm) {
  float gs = grad_scale;
  if (sumsq != nullptr) {
    const float norm = (float)sqrt(*sumsq) * grad_scale;
    const float coef = max_norm / (norm + 1e-6f);
    gs *= fminf(coef, 1.0f);
  }
  const float step = lr / bc1;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float gi = g[i] * gs;
    float pi = p[i] * (1.f - lr * wd);
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    pi -= step * mi / (sqrtf(vi) / bc2_sqrt + eps);
    p[i] = pi;
    m[i] = mi;
    v[i] = vi;
  }
}

extern "C" int cn_adamw_step_f32(float* p, const float* g, float* m, float* v, long n, float lr, float beta1,
                                 float beta2, float eps, float weight_decay, int step, float grad_scale,
                                 const double* sumsq, float max_norm, void* stream) {
  if (n <= 0) return CN_OK;
  const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
  const float bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step));
  long bx = (n + 1023) / 1024;
  if (bx > 2048) bx = 2048;
  CN_LAUNCH(cn_adamw_kernel, dim3((unsigned)bx), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, lr, beta1,
                     beta2, eps, weight_decay, bc1, bc2_sqrt, grad_scale, sumsq, max_norm);
  return cn_check_launch();
}

// ---- segmented step: frozen parameters (transfer learning, partial training) ------------------------------------------
// torch.optim.AdamW skips a parameter whose .grad is None and clip_grad_norm_ only sees parameters with a gradient, so a
// step with frozen parameters touches the TRAINABLE runs of the flat buffers only, each with its own AdamW step count.
// The host passes a table of segments (runs of adjacent trainable parameters sharing a step count, merged across the
// 16-byte slice padding, whose elements are zero in every buffer and stay zero). Each segment is cut into chunks of
// CN_SEG_CHUNK elements; chunk0 is the index of a segment's first chunk (an exclusive prefix sum over the table), so a
// block maps its chunk to its segment by a binary search: one 300 K-element run and 300 one-element runs both spread
// over the grid, and nothing walks the table serially.
struct CnSeg {
  long off;    // first element in the flat buffers
  long len;    // elements
  int step;    // AdamW step count of the segment's parameters (after this step's increment)
  int chunk0;  // index of the segment's first chunk
};
static_assert(sizeof(CnSeg) == 24, "CnSeg is a 24-byte record of the host table");

#define CN_SEG_CHUNK 4096

__device__ __forceinline__ int cn_seg_find(const CnSeg* __restrict__ segs, int nseg, int chunk) {
  int lo = 0, hi = nseg - 1;  // last segment with chunk0 <= chunk
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (segs[mid].chunk0 <= chunk) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void cn_sumsq_seg_kernel(const float* __restrict__ g, long n,
                                                           const CnSeg* __restrict__ segs, int nseg, int nchunks,
                                                           double* __restrict__ out) {
  __shared__ double scratch[4];
  double s = 0.0;
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const CnSeg sg = segs[cn_seg_find(segs, nseg, c)];
    const long lo = sg.off + (long)(c - sg.chunk0) * CN_SEG_CHUNK;
    long hi = sg.off + sg.len;
    if (hi > lo + CN_SEG_CHUNK) hi = lo + CN_SEG_CHUNK;
    if (hi > n) hi = n;
    for (long i = lo + threadIdx.x; i < hi; i += 256) {
      const float v = g[i];
      s += (double)v * v;
    }
  }
  s = cn_block_sum<double, 256>(s, scratch);
  if (threadIdx.x == 0 && s != 0.0) atomicAdd(out, s);
}

static long cn_seg_grid(int nchunks, long cap) { return nchunks < cap ? nchunks : cap; }

// out[0] = sum over the segments of g^2 (zeroed here first)
extern "C" int cn_grad_sumsq_seg_f32(const float* g, long n, const void* segs, int nseg, int nchunks, double* out,
                                     void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (nseg < 0 || nchunks < 0 || n < 0) return CN_ERR_ARG;
  if (hipMemsetAsync(out, 0, sizeof(double), stream) != hipSuccess) return CN_ERR_LAUNCH;
  if (nseg == 0 || nchunks == 0) return CN_OK;
  CN_LAUNCH(cn_sumsq_seg_kernel, dim3((unsigned)cn_seg_grid(nchunks, 1024)), dim3(256), 0, stream, g, n,
            (const CnSeg*)segs, nseg, nchunks, out);
  return cn_check_launch();
}

// The update of cn_adamw_kernel per segment, with the segment's own bias corrections (computed in double from its step
// + step_add, as the host does for the unsegmented step: a table stays valid while its trainable set is unchanged, since
// all its parameters advance together, and the host passes the steps taken since it was built). The clip coefficient comes from the segmented sum of squares.
__global__ __launch_bounds__(256) void cn_adamw_seg_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ m, float* __restrict__ v, long n,
                                                          const CnSeg* __restrict__ segs, int nseg, int nchunks,
                                                          int step_add, float lr, float b1, float b2, float eps, float wd,
                                                          float grad_scale, const double* sumsq, float max_norm) {
  float gs = grad_scale;
  if (sumsq != nullptr) {
    const float norm = (float)sqrt(*sumsq) * grad_scale;
    const float coef = max_norm / (norm + 1e-6f);
    gs *= fminf(coef, 1.0f);
  }
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const CnSeg sg = segs[cn_seg_find(segs, nseg, c)];
    const long lo = sg.off + (long)(c - sg.chunk0) * CN_SEG_CHUNK;
    long hi = sg.off + sg.len;
    if (hi > lo + CN_SEG_CHUNK) hi = lo + CN_SEG_CHUNK;
    if (hi > n) hi = n;
    const double t = (double)sg.step + step_add;
    const float bc1 = (float)(1.0 - pow((double)b1, t));
    const float bc2_sqrt = (float)sqrt(1.0 - pow((double)b2, t));
    const float step = lr / bc1;
    for (long i = lo + threadIdx.x; i < hi; i += 256) {
      const float gi = g[i] * gs;
      float pi = p[i] * (1.f - lr * wd);
      const float mi = b1 * m[i] + (1.f - b1) * gi;
      const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
      pi -= step * mi / (sqrtf(vi) / bc2_sqrt + eps);
      p[i] = pi;
      m[i] = mi;
      v[i] = vi;
    }
  }
}

extern "C" int cn_adamw_step_seg_f32(float* p, const float* g, float* m, float* v, long n, const void* segs, int nseg,
                                     int nchunks, int step_add, float lr, float beta1, float beta2, float eps, float weight_decay,
                                     float grad_scale, const double* sumsq, float max_norm, void* stream) {
  if (nseg < 0 || nchunks < 0 || n < 0) return CN_ERR_ARG;
  if (nseg == 0 || nchunks == 0) return CN_OK;
  CN_LAUNCH(cn_adamw_seg_kernel, dim3((unsigned)cn_seg_grid(nchunks, 2048)), dim3(256), 0, (hipStream_t)stream, p, g,
            m, v, n, (const CnSeg*)segs, nseg, nchunks, step_add, lr, beta1, beta2, eps, weight_decay, grad_scale, sumsq,
            max_norm);
  return cn_check_launch();
}

extern "C" int cn_version() { return 101; }
