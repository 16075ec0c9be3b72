// Fused optimizer step over the flat parameter / gradient buffers (gfx950, HBM-bound).
//
// Reference: torch.optim.AdamW(lr, weight_decay, eps, betas=(0.9, 0.98)) configured at
// /root/reference/src/cultionet/models/lightning.py:622-629 and gradient_clip_val=1.0
// (norm clipping) at /root/reference/src/cultionet/model.py:84,173.
// All parameters live in ONE contiguous fp32 buffer (and so do grads, exp_avg, exp_avg_sq), so the
// whole step is two launches: a sum-of-squares reduction and the update. The clip coefficient is
// computed on the device from the reduced norm -- no host synchronisation.
// The reference's other choices -- Adam, RAdam, SGD (lightning.py:611-655) and value clipping -- follow the AdamW pair
// below: cn_optim_step_f32 / cn_optim_step_seg_f32 (Adam with norm clipping is the AdamW kernel with weight_decay 0;
// value clipping happens inside the update and needs no reduction launch).
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

// ---- every optimizer and clip mode of the reference's command line ------------------------------------------------------
// --optimizer Adam | AdamW | RAdam | SGD and gradient_clip_algorithm norm | value (lightning.py:611-655, model.py:84,173)
// over the same flat buffers and the same CnSeg table as the AdamW pair above. torch 2.10 single-tensor semantics,
// maximize=False, no amsgrad / nesterov / dampening:
//   CN_OPT_ADAMW  the rule above (Adam is weight_decay = 0: p * 1 is exact)
//   CN_OPT_SGD    g += wd*p ; buf = mu*buf + g ; p -= lr*buf      (mu arrives as beta1: OneCycleLR cycles it; torch's
//                 first-step buf = g equals mu*0 + g, so a zero-initialised buffer needs no branch; v is never touched)
//   CN_OPT_RADAM  p *= 1 - lr*wd ; m, v as AdamW ; rho_t = rho_inf - 2 t b2^t / (1 - b2^t)
//                 rho_t > 5:  p -= (lr/bc1) * m * rect * sqrt(bc2) / (sqrt(v) + eps)     else  p -= (lr/bc1) * m
// The gradient an element sees is g * grad_scale, then times the norm-clip coefficient (CN_CLIP_NORM, sumsq as above) or
// clamped to [-clip, clip] (CN_CLIP_VALUE: clip_grad_value_, no reduction launch at all). Everything that depends on
// the step count alone is computed once per launch (per chunk when segmented) in double.
// HBM streaming: 16-byte accesses over the 16-byte-aligned body of a run, scalar head / tail (a run of the segment
// table may start anywhere; ParamStore slices start on 16 bytes).
enum { CN_OPT_ADAMW = 0, CN_OPT_SGD = 1, CN_OPT_RADAM = 2 };
enum { CN_CLIP_NONE = 0, CN_CLIP_NORM = 1, CN_CLIP_VALUE = 2 };

struct CnOptCoef {
  float decay;  // 1 - lr*wd (decoupled)            | SGD: wd
  float step;   // lr / bc1                         | SGD: lr
  float adapt;  // AdamW sqrt(bc2); RAdam rect*sqrt(bc2), or 0 while the variance is not rectified yet
  float b1, b2, eps;
};

__host__ __device__ inline CnOptCoef cn_opt_coef(int kind, float lr, float b1, float b2, float eps, float wd, double t) {
  CnOptCoef c;
  c.b1 = b1, c.b2 = b2, c.eps = eps;
  if (kind == CN_OPT_SGD) {
    c.decay = wd, c.step = lr, c.adapt = 0.f;
    return c;
  }
  const double b2t = pow((double)b2, t);
  const double bc2 = 1.0 - b2t;
  c.decay = 1.f - lr * wd;
  c.step = lr / (float)(1.0 - pow((double)b1, t));
  c.adapt = (float)sqrt(bc2);
  if (kind == CN_OPT_RADAM) {
    const double rho_inf = 2.0 / (1.0 - (double)b2) - 1.0;
    const double rho_t = rho_inf - 2.0 * t * b2t / bc2;
    c.adapt = rho_t > 5.0 ? (float)(sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf /
                                         ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t)) * sqrt(bc2))
                          : 0.f;
  }
  return c;
}

template <int KIND, int CLIP>
__device__ __forceinline__ void cn_opt_elem(float& p, float g, float& m, float& v, const CnOptCoef& c, float gs,
                                            float clip) {
  g *= gs;
  if (CLIP == CN_CLIP_VALUE) g = fminf(fmaxf(g, -clip), clip);
  if (KIND == CN_OPT_SGD) {
    g += c.decay * p;
    m = c.b1 * m + g;
    p -= c.step * m;
    return;
  }
  p *= c.decay;
  m = c.b1 * m + (1.f - c.b1) * g;
  v = c.b2 * v + (1.f - c.b2) * g * g;
  if (KIND == CN_OPT_ADAMW) {
    p -= c.step * m / (sqrtf(v) / c.adapt + c.eps);
  } else if (c.adapt != 0.f) {
    p -= c.step * m * c.adapt / (sqrtf(v) + c.eps);
  } else {
    p -= c.step * m;
  }
}

template <int KIND, int CLIP>
__device__ __forceinline__ void cn_opt_one(float* p, const float* g, float* m, float* v, long i, const CnOptCoef& c,
                                           float gs, float clip) {
  float pi = p[i], mi = m[i], vi = KIND == CN_OPT_SGD ? 0.f : v[i];
  cn_opt_elem<KIND, CLIP>(pi, g[i], mi, vi, c, gs, clip);
  p[i] = pi;
  m[i] = mi;
  if (KIND != CN_OPT_SGD) v[i] = vi;
}

template <int KIND, int CLIP>
__device__ __forceinline__ void cn_opt_four(float* p, const float* g, float* m, float* v, long i, const CnOptCoef& c,
                                            float gs, float clip) {
  float4 p4 = *reinterpret_cast<float4*>(p + i), m4 = *reinterpret_cast<float4*>(m + i);
  const float4 g4 = *reinterpret_cast<const float4*>(g + i);
  float4 v4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (KIND != CN_OPT_SGD) v4 = *reinterpret_cast<float4*>(v + i);
  cn_opt_elem<KIND, CLIP>(p4.x, g4.x, m4.x, v4.x, c, gs, clip);
  cn_opt_elem<KIND, CLIP>(p4.y, g4.y, m4.y, v4.y, c, gs, clip);
  cn_opt_elem<KIND, CLIP>(p4.z, g4.z, m4.z, v4.z, c, gs, clip);
  cn_opt_elem<KIND, CLIP>(p4.w, g4.w, m4.w, v4.w, c, gs, clip);
  *reinterpret_cast<float4*>(p + i) = p4;
  *reinterpret_cast<float4*>(m + i) = m4;
  if (KIND != CN_OPT_SGD) *reinterpret_cast<float4*>(v + i) = v4;
}

// elements [lo, hi) by one block; `vec` when the four base pointers are 16-byte aligned
template <int KIND, int CLIP>
__device__ __forceinline__ void cn_opt_run(float* p, const float* g, float* m, float* v, long lo, long hi, long first,
                                           long stride, bool vec, const CnOptCoef& c, float gs, float clip) {
  long alo = hi, ahi = hi;  // [alo, ahi): the aligned body
  if (vec) {
    alo = (lo + 3) & ~3L;
    if (alo > hi) alo = hi;
    ahi = alo + ((hi - alo) & ~3L);
  }
  for (long i = lo + first; i < alo; i += stride) cn_opt_one<KIND, CLIP>(p, g, m, v, i, c, gs, clip);
  for (long i = alo + 4 * first; i < ahi; i += 4 * stride) cn_opt_four<KIND, CLIP>(p, g, m, v, i, c, gs, clip);
  for (long i = ahi + first; i < hi; i += stride) cn_opt_one<KIND, CLIP>(p, g, m, v, i, c, gs, clip);
}

__device__ __forceinline__ float cn_clip_scale(int clip_mode, float grad_scale, const double* sumsq, float clip) {
  if (clip_mode != CN_CLIP_NORM) return grad_scale;
  const float norm = (float)sqrt(*sumsq) * grad_scale;
  return grad_scale * fminf(clip / (norm + 1e-6f), 1.0f);
}

template <int KIND, int CLIP>
__global__ __launch_bounds__(256) void cn_optim_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                      float* __restrict__ m, float* __restrict__ v, long n, CnOptCoef c,
                                                      float grad_scale, const double* sumsq, float clip, int vec) {
  const float gs = cn_clip_scale(CLIP, grad_scale, sumsq, clip);
  cn_opt_run<KIND, CLIP>(p, g, m, v, 0, n, blockIdx.x * 256L + threadIdx.x, (long)gridDim.x * 256, vec != 0, c, gs,
                         clip);
}

// Loss scaling (torch.amp.GradScaler, the reference's default precision "16-mixed") without a host synchronisation: the
// scaler leaves three device words and the kernel reads them at block start, one wave-uniform load each.
//   found_inf   != 0: this step is skipped -- every block returns before its first store, p / m / v keep their bits
//   loss_scale  the gradient still carries it: an element sees g * grad_scale / *loss_scale, and the norm of
//               CN_CLIP_NORM is sqrt(*sumsq) * grad_scale / *loss_scale (sumsq taken over the scaled gradient)
//   skipped     steps skipped so far, which the host's step counts include: the coefficients use step - *skipped
// Null means 1, 0 and 0: cn_optim_step_seg_f32 is this kernel with the three of them null.
template <int KIND, int CLIP>
__global__ __launch_bounds__(256) void cn_optim_seg_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ m, float* __restrict__ v, long n,
                                                          const CnSeg* __restrict__ segs, int nseg, int nchunks,
                                                          int step_add, float lr, float b1, float b2, float eps, float wd,
                                                          float grad_scale, const float* __restrict__ loss_scale,
                                                          const float* __restrict__ found_inf,
                                                          const int* __restrict__ skipped, const double* sumsq,
                                                          float clip, int vec) {
  if (found_inf != nullptr && *found_inf != 0.f) return;
  if (loss_scale != nullptr) grad_scale *= 1.f / *loss_scale;
  if (skipped != nullptr) step_add -= *skipped;
  const float gs = cn_clip_scale(CLIP, grad_scale, sumsq, clip);
  for (int ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const CnSeg sg = segs[cn_seg_find(segs, nseg, ch)];
    const long lo = sg.off + (long)(ch - sg.chunk0) * CN_SEG_CHUNK;
    long hi = sg.off + sg.len;
    if (hi > lo + CN_SEG_CHUNK) hi = lo + CN_SEG_CHUNK;
    if (hi > n) hi = n;
    const CnOptCoef c = cn_opt_coef(KIND, lr, b1, b2, eps, wd, (double)sg.step + step_add);
    cn_opt_run<KIND, CLIP>(p, g, m, v, lo, hi, threadIdx.x, 256, vec != 0, c, gs, clip);
  }
}

// ++*skipped when the scaler found an inf / NaN (after the step that read both words, on the same stream)
__global__ void cn_amp_count_skip_kernel(const float* __restrict__ found_inf, int* __restrict__ skipped) {
  if (*found_inf != 0.f) *skipped = *skipped + 1;
}

static bool cn_opt_args_ok(int kind, int clip_mode, const void* v, const double* sumsq) {
  if (kind < CN_OPT_ADAMW || kind > CN_OPT_RADAM || clip_mode < CN_CLIP_NONE || clip_mode > CN_CLIP_VALUE) return false;
  if (kind != CN_OPT_SGD && v == nullptr) return false;
  return clip_mode != CN_CLIP_NORM || sumsq != nullptr;
}

static int cn_opt_vec(const void* p, const void* g, const void* m, const void* v) {
  return (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
}

#define CN_OPT_DISPATCH(KERNEL, kind, clip_mode, ...)                                                     \
  do {                                                                                                    \
    switch ((kind) * 3 + (clip_mode)) {                                                                   \
      case 0: CN_LAUNCH((KERNEL<CN_OPT_ADAMW, CN_CLIP_NONE>), __VA_ARGS__); break;                        \
      case 1: CN_LAUNCH((KERNEL<CN_OPT_ADAMW, CN_CLIP_NORM>), __VA_ARGS__); break;                        \
      case 2: CN_LAUNCH((KERNEL<CN_OPT_ADAMW, CN_CLIP_VALUE>), __VA_ARGS__); break;                       \
      case 3: CN_LAUNCH((KERNEL<CN_OPT_SGD, CN_CLIP_NONE>), __VA_ARGS__); break;                          \
      case 4: CN_LAUNCH((KERNEL<CN_OPT_SGD, CN_CLIP_NORM>), __VA_ARGS__); break;                          \
      case 5: CN_LAUNCH((KERNEL<CN_OPT_SGD, CN_CLIP_VALUE>), __VA_ARGS__); break;                         \
      case 6: CN_LAUNCH((KERNEL<CN_OPT_RADAM, CN_CLIP_NONE>), __VA_ARGS__); break;                        \
      case 7: CN_LAUNCH((KERNEL<CN_OPT_RADAM, CN_CLIP_NORM>), __VA_ARGS__); break;                        \
      default: CN_LAUNCH((KERNEL<CN_OPT_RADAM, CN_CLIP_VALUE>), __VA_ARGS__); break;                      \
    }                                                                                                     \
  } while (0)

// kind: CN_OPT_*; clip_mode: CN_CLIP_* (`clip` is max_norm or clip_value; sumsq is read under CN_CLIP_NORM only).
// v is not touched (may be null) for CN_OPT_SGD, whose momentum arrives as beta1.
extern "C" int cn_optim_step_f32(int kind, int clip_mode, float* p, const float* g, float* m, float* v, long n, float lr,
                                 float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                                 const double* sumsq, float clip, void* stream) {
  if (n < 0 || !cn_opt_args_ok(kind, clip_mode, v, sumsq)) return CN_ERR_ARG;
  if (n == 0) return CN_OK;
  const CnOptCoef c = cn_opt_coef(kind, lr, beta1, beta2, eps, weight_decay, (double)step);
  long bx = (n + 1023) / 1024;
  if (bx > 2048) bx = 2048;
  CN_OPT_DISPATCH(cn_optim_kernel, kind, clip_mode, dim3((unsigned)bx), dim3(256), 0, (hipStream_t)stream, p, g, m, v,
                  n, c, grad_scale, sumsq, clip, cn_opt_vec(p, g, m, v));
  return cn_check_launch();
}

extern "C" int cn_optim_step_seg_f32(int kind, int clip_mode, float* p, const float* g, float* m, float* v, long n,
                                     const void* segs, int nseg, int nchunks, int step_add, float lr, float beta1,
                                     float beta2, float eps, float weight_decay, float grad_scale, const double* sumsq,
                                     float clip, void* stream) {
  if (nseg < 0 || nchunks < 0 || n < 0 || !cn_opt_args_ok(kind, clip_mode, v, sumsq)) return CN_ERR_ARG;
  if (nseg == 0 || nchunks == 0) return CN_OK;
  CN_OPT_DISPATCH(cn_optim_seg_kernel, kind, clip_mode, dim3((unsigned)cn_seg_grid(nchunks, 2048)), dim3(256), 0,
                  (hipStream_t)stream, p, g, m, v, n, (const CnSeg*)segs, nseg, nchunks, step_add, lr, beta1, beta2, eps,
                  weight_decay, grad_scale, (const float*)nullptr, (const float*)nullptr, (const int*)nullptr, sumsq, clip,
                  cn_opt_vec(p, g, m, v));
  return cn_check_launch();
}

// The segmented step under a loss scaler: loss_scale / found_inf / skipped are DEVICE words (each may be null), see
// cn_optim_seg_kernel. A whole, unfrozen model is a table of one segment.
extern "C" int cn_optim_step_amp_f32(int kind, int clip_mode, float* p, const float* g, float* m, float* v, long n,
                                     const void* segs, int nseg, int nchunks, int step_add, float lr, float beta1,
                                     float beta2, float eps, float weight_decay, float grad_scale,
                                     const float* loss_scale, const float* found_inf, const int* skipped,
                                     const double* sumsq, float clip, void* stream) {
  if (nseg < 0 || nchunks < 0 || n < 0 || !cn_opt_args_ok(kind, clip_mode, v, sumsq)) return CN_ERR_ARG;
  if (nseg == 0 || nchunks == 0) return CN_OK;
  CN_OPT_DISPATCH(cn_optim_seg_kernel, kind, clip_mode, dim3((unsigned)cn_seg_grid(nchunks, 2048)), dim3(256), 0,
                  (hipStream_t)stream, p, g, m, v, n, (const CnSeg*)segs, nseg, nchunks, step_add, lr, beta1, beta2, eps,
                  weight_decay, grad_scale, loss_scale, found_inf, skipped, sumsq, clip, cn_opt_vec(p, g, m, v));
  return cn_check_launch();
}

extern "C" int cn_amp_count_skip(const float* found_inf, int* skipped, void* stream) {
  if (found_inf == nullptr || skipped == nullptr) return CN_ERR_ARG;
  CN_LAUNCH(cn_amp_count_skip_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, found_inf, skipped);
  return cn_check_launch();
}

extern "C" int cn_version() { return 104; }
