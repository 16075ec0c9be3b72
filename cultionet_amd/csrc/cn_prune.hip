// Global magnitude pruning over the flat parameter buffer: what torch.nn.utils.prune.global_unstructured(...,
// L1Unstructured, amount) decides (the ModelPruning callback of the reference, callbacks.py:268-269),
// restated over integers, plus the masked copy that keeps pruned entries at +0.0 during training.
//
// flags: one byte per flat element, bit 0 = alive, bit 1 = prunable. An element takes part in a selection when both are
// set; its key is bits(|w|) (31 bits: -0.0 and +0.0 share key 0, non-finite values order by bit pattern, above every
// finite one). A round prunes the k eligible elements of smallest key; among the elements whose key equals the k-th
// smallest (the threshold T) the lowest flat index goes first, so exactly k bits are cleared.
//
//   cn_prune_magnitude_u8   nine launches, no host synchronisation, no allocation:
//     3 x (histogram, pick)   radix selection over 11 + 10 + 10 key bits. The histogram pass is a grid-stride kernel with
//                             an LDS-private histogram (one LDS atomic per run of equal bins, non-zero bins flushed with
//                             integer global atomics: the pattern of cn_chip_hist_kernel); the one-block pick narrows
//                             ws[0] = key prefix, ws[1] = remaining k, and leaves the histogram zero.
//                             After the third pick ws[0] = T and ws[1] = r, the number of ties to prune (>= 1).
//     tie count               elements with key == T per chunk of CN_PRUNE_CHUNK flat elements (plain stores)
//     scan                    exclusive scan of the chunk counts, one block
//     commit                  clears bit 0 where key < T, or key == T and the element's rank among the ties (chunk
//                             offset + ballot / popcount prefix inside the chunk) is < r
//   cn_mask_select_f32      dst[i] = pruned(i) ? +0.0 : src[i], a select on bit patterns (dst == src allowed)
//   cn_prune_reset_f32      p[i] = prunable(i) ? (alive(i) ? snapshot[i] : +0.0) : p[i]  (lottery-ticket reset)
//   cn_prune_count_u32      out[0] += eligible elements
// Every sum is an integer: the result does not depend on arrival order.
#include "cn_common.h"

#define CN_PRUNE_NT 256
#define CN_PRUNE_BINS 2048             // pass 0: 11 bits; passes 1 and 2: 10 bits
#define CN_PRUNE_MIN_PER_BLOCK 65536L  // elements behind one histogram flush (at most 2048 global atomics)
#define CN_PRUNE_MAX_BLOCKS 512
#define CN_PRUNE_CHUNK 2048            // flat elements per chunk of the ordered tie-break
#define CN_PRUNE_HEAD 8                // words in front of the histogram: [0] prefix / T, [1] remaining k / r
#define CN_PRUNE_SCAN_NT 1024

typedef unsigned int u32;
typedef unsigned long long u64;

__device__ __forceinline__ u32 cn_prune_key(float w) { return __float_as_uint(w) & 0x7fffffffu; }
__device__ __forceinline__ bool cn_prune_eligible(u32 flag) { return (flag & 3u) == 3u; }
__device__ __forceinline__ bool cn_prune_pruned(u32 flag) { return (flag & 3u) == 2u; }

// Block-wide exclusive scan of one value per thread, in thread order. wave_tot: NT / 64 words.
template <int NT>
__device__ __forceinline__ u32 cn_prune_block_scan(u32 mine, u32* wave_tot) {
  const int lane = threadIdx.x & (CN_WAVE - 1), wid = threadIdx.x / CN_WAVE;
  u32 incl = mine;
#pragma unroll
  for (int off = 1; off < CN_WAVE; off <<= 1) {
    const u32 up = __shfl_up(incl, off, CN_WAVE);
    if (lane >= off) incl += up;
  }
  if (lane == CN_WAVE - 1) wave_tot[wid] = incl;
  __syncthreads();
  u32 before = incl - mine;
#pragma unroll
  for (int i = 0; i < NT / CN_WAVE; ++i) before += i < wid ? wave_tot[i] : 0;
  return before;
}

// ---- radix selection ----------------------------------------------------------------------------------------
// One pass: hist[(key >> shift) & (nb - 1)] += 1 over the eligible elements whose key >> hi_shift equals the prefix the
// earlier picks left in head[0] (pass 0, hi_shift 31: every eligible element).
__global__ __launch_bounds__(CN_PRUNE_NT) void cn_prune_hist_kernel(const float* __restrict__ w,
                                                                   const unsigned char* __restrict__ flags, long n,
                                                                   int shift, int nb, int hi_shift,
                                                                   const u32* __restrict__ head, u32* __restrict__ hist) {
  __shared__ u32 bins[CN_PRUNE_BINS];
  const int tid = threadIdx.x;
  for (int k = tid; k < nb; k += CN_PRUNE_NT) bins[k] = 0;
  __syncthreads();
  const u32 prefix = hi_shift >= 31 ? 0u : head[0];
  const u32 mask = (u32)nb - 1u;
  CnHistRun run{0, 0};
  const long n4 = n >> 2;
  const float4* w4 = (const float4*)w;
  const u32* f4 = (const u32*)flags;
  for (long i = blockIdx.x * (long)CN_PRUNE_NT + tid; i < n4; i += (long)gridDim.x * CN_PRUNE_NT) {
    const u32 f = f4[i];
    const float4 q = w4[i];
    const float v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const u32 key = cn_prune_key(v[e]);
      if (cn_prune_eligible(f >> (8 * e)) && (key >> hi_shift) == prefix) run.add(bins, (int)((key >> shift) & mask));
    }
  }
  if (blockIdx.x == 0 && tid < (int)(n & 3)) {  // the elements after the last whole vector
    const long i = (n4 << 2) + tid;
    const u32 key = cn_prune_key(w[i]);
    if (cn_prune_eligible(flags[i]) && (key >> hi_shift) == prefix) run.add(bins, (int)((key >> shift) & mask));
  }
  run.flush(bins);
  __syncthreads();
  for (int k = tid; k < nb; k += CN_PRUNE_NT) {
    const u32 c = bins[k];
    if (c) __hip_atomic_fetch_add(hist + k, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One block. The bin that holds the element of sorted rank k - 1 among those counted: head[0] = (prefix << bits) | bin,
// head[1] = k - (elements in the bins below it), in [1, hist[bin]]. k_in >= 0 (pass 0): k comes from the host and the
// prefix is empty. The histogram is left zero for the next pass. The caller guarantees 1 <= k <= counted elements.
__global__ __launch_bounds__(CN_PRUNE_NT) void cn_prune_pick_kernel(u32* __restrict__ head, u32* __restrict__ hist, int nb,
                                                                   int bits, long k_in) {
  __shared__ u32 wave_tot[CN_PRUNE_NT / CN_WAVE];
  const int tid = threadIdx.x;
  const u32 k = k_in >= 0 ? (u32)k_in : head[1];
  const u32 prefix = k_in >= 0 ? 0u : head[0];
  const int per = nb / CN_PRUNE_NT;  // 8 or 4 adjacent bins per thread
  u32 h[CN_PRUNE_BINS / CN_PRUNE_NT];
  u32 mine = 0;
#pragma unroll
  for (int j = 0; j < CN_PRUNE_BINS / CN_PRUNE_NT; ++j) {
    h[j] = 0;
    if (j < per) {
      h[j] = hist[tid * per + j];
      hist[tid * per + j] = 0;
      mine += h[j];
    }
  }
  const u32 before = cn_prune_block_scan<CN_PRUNE_NT>(mine, wave_tot);  // (its barrier: reads of head above, writes below)
  if (before < k && k <= before + mine) {
    u32 cum = before;
#pragma unroll
    for (int j = 0; j < CN_PRUNE_BINS / CN_PRUNE_NT; ++j) {
      if (j < per && cum < k && k <= cum + h[j]) {
        head[0] = (prefix << bits) | (u32)(tid * per + j);
        head[1] = k - cum;
      }
      cum += h[j];
    }
  }
}

// ---- ordered tie-break and commit ---------------------------------------------------------------------------
// grid (chunks): counts[chunk] = eligible elements of the chunk with key == T
__global__ __launch_bounds__(CN_PRUNE_NT) void cn_prune_tie_count_kernel(const float* __restrict__ w,
                                                                        const unsigned char* __restrict__ flags, long n,
                                                                        const u32* __restrict__ head,
                                                                        u32* __restrict__ counts) {
  __shared__ u32 scratch[CN_PRUNE_NT / CN_WAVE];
  const u32 thr = head[0];
  const long base = (long)blockIdx.x * CN_PRUNE_CHUNK;
  u32 c = 0;
#pragma unroll
  for (int j = 0; j < CN_PRUNE_CHUNK / CN_PRUNE_NT; ++j) {
    const long i = base + j * CN_PRUNE_NT + threadIdx.x;
    if (i < n && cn_prune_eligible(flags[i]) && cn_prune_key(w[i]) == thr) ++c;
  }
  c = cn_block_sum<u32, CN_PRUNE_NT>(c, scratch);
  if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

// One block: counts[c] = sum of counts[0 .. c), in place.
__global__ __launch_bounds__(CN_PRUNE_SCAN_NT) void cn_prune_scan_kernel(u32* __restrict__ counts, int nchunks) {
  __shared__ u32 wave_tot[CN_PRUNE_SCAN_NT / CN_WAVE];
  const int per = (nchunks + CN_PRUNE_SCAN_NT - 1) / CN_PRUNE_SCAN_NT;
  const long k0 = (long)threadIdx.x * per;
  const long k1 = k0 + per < nchunks ? k0 + per : nchunks;
  u32 mine = 0;
  for (long k = k0; k < k1; ++k) mine += counts[k];
  u32 cum = cn_prune_block_scan<CN_PRUNE_SCAN_NT>(mine, wave_tot);
  for (long k = k0; k < k1; ++k) {
    const u32 c = counts[k];
    counts[k] = cum;
    cum += c;
  }
}

// grid (chunks): a block walks its chunk in flat order, CN_PRUNE_NT elements at a time, one element per lane, and every
// lane stores its own byte only.
__global__ __launch_bounds__(CN_PRUNE_NT) void cn_prune_commit_kernel(const float* __restrict__ w,
                                                                     unsigned char* __restrict__ flags, long n,
                                                                     const u32* __restrict__ head,
                                                                     const u32* __restrict__ offsets) {
  __shared__ u32 wave_cnt[2][CN_PRUNE_NT / CN_WAVE];
  const int tid = threadIdx.x, lane = tid & (CN_WAVE - 1), wid = tid / CN_WAVE;
  const u32 thr = head[0], quota = head[1];
  const long base = (long)blockIdx.x * CN_PRUNE_CHUNK;
  u32 rank0 = offsets[blockIdx.x];  // ties in front of this chunk
#pragma unroll
  for (int j = 0; j < CN_PRUNE_CHUNK / CN_PRUNE_NT; ++j) {
    const long i = base + j * CN_PRUNE_NT + tid;
    u32 f = 0, key = 0;
    if (i < n) {
      f = flags[i];
      key = cn_prune_key(w[i]);
    }
    const bool eligible = i < n && cn_prune_eligible(f);
    const bool tie = eligible && key == thr;
    const u64 ties = __ballot(tie);
    if (lane == 0) wave_cnt[j & 1][wid] = (u32)__popcll(ties);
    __syncthreads();  // (the buffer written two rounds later is this one: every wave has passed the next barrier by then)
    u32 before = 0, total = 0;
#pragma unroll
    for (int v = 0; v < CN_PRUNE_NT / CN_WAVE; ++v) {
      const u32 c = wave_cnt[j & 1][v];
      before += v < wid ? c : 0;
      total += c;
    }
    const u32 rank = rank0 + before + (u32)__popcll(ties & ((1ull << lane) - 1ull));
    if (eligible && (key < thr || (tie && rank < quota))) flags[i] = (unsigned char)(f & ~1u);
    rank0 += total;
  }
}

extern "C" long cn_prune_workspace_words(long n) {
  if (n <= 0) return -1;
  return CN_PRUNE_HEAD + CN_PRUNE_BINS + (n + CN_PRUNE_CHUNK - 1) / CN_PRUNE_CHUNK;
}

// Clears bit 0 of the k eligible elements (flags & 3 == 3) of smallest |w|, ties by lowest index. The caller guarantees
// 1 <= k <= eligible elements (it tracks that count on the host). ws: cn_prune_workspace_words(n) words, ZERO-FILLED
// before its first use (every call leaves the histogram zero), not shared with a call in flight on another stream.
extern "C" int cn_prune_magnitude_u8(const float* w, unsigned char* flags, long n, long k, unsigned int* ws, long ws_words,
                                     void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (w == nullptr || flags == nullptr || ws == nullptr) return CN_ERR_ARG;
  if (n <= 0 || n >= (1L << 31) || k < 1 || k > n) return CN_ERR_ARG;
  if ((uintptr_t)w % 16 != 0 || (uintptr_t)flags % 4 != 0 || (uintptr_t)ws % 4 != 0) return CN_ERR_ARG;
  if (ws_words < cn_prune_workspace_words(n)) return CN_ERR_ARG;
  u32* head = ws;
  u32* hist = ws + CN_PRUNE_HEAD;
  u32* counts = hist + CN_PRUNE_BINS;
  long nblk = n / CN_PRUNE_MIN_PER_BLOCK;
  nblk = nblk < 1 ? 1 : (nblk > CN_PRUNE_MAX_BLOCKS ? CN_PRUNE_MAX_BLOCKS : nblk);
  const int shifts[3] = {20, 10, 0}, bits[3] = {11, 10, 10}, hi_shifts[3] = {31, 20, 10};
  for (int p = 0; p < 3; ++p) {
    CN_LAUNCH(cn_prune_hist_kernel, dim3((unsigned)nblk), dim3(CN_PRUNE_NT), 0, stream, w, (const unsigned char*)flags, n,
              shifts[p], 1 << bits[p], hi_shifts[p], (const u32*)head, hist);
    CN_LAUNCH(cn_prune_pick_kernel, dim3(1), dim3(CN_PRUNE_NT), 0, stream, head, hist, 1 << bits[p], bits[p],
              p == 0 ? k : -1L);
  }
  const int nchunks = (int)((n + CN_PRUNE_CHUNK - 1) / CN_PRUNE_CHUNK);
  CN_LAUNCH(cn_prune_tie_count_kernel, dim3((unsigned)nchunks), dim3(CN_PRUNE_NT), 0, stream, w,
            (const unsigned char*)flags, n, (const u32*)head, counts);
  CN_LAUNCH(cn_prune_scan_kernel, dim3(1), dim3(CN_PRUNE_SCAN_NT), 0, stream, counts, nchunks);
  CN_LAUNCH(cn_prune_commit_kernel, dim3((unsigned)nchunks), dim3(CN_PRUNE_NT), 0, stream, w, flags, n, (const u32*)head,
            (const u32*)counts);
  return cn_check_launch();
}

// ---- masked copy ----------------------------------------------------------------------------------------------
// RESET = false: dst[i] = pruned ? +0.0 : src[i]. RESET = true: dst[i] = prunable ? (alive ? src[i] : +0.0) : dst[i].
// Selects on the loaded words: a kept value keeps its bit pattern (NaN payloads included), a pruned inf / NaN becomes +0.0.
template <bool RESET>
__device__ __forceinline__ float cn_mask_pick(u32 flag, float src, float own) {
  if (RESET) return (flag & 2u) ? ((flag & 1u) ? src : 0.0f) : own;
  return cn_prune_pruned(flag) ? 0.0f : src;
}

template <bool RESET>
__global__ __launch_bounds__(256) void cn_mask_select_kernel(float* dst, const float* src, const unsigned char* flags,
                                                             long n) {
  const long n4 = n >> 2;
  const u32* f4 = (const u32*)flags;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const u32 f = f4[i];
    const float4 q = ((const float4*)src)[i];
    float4 d = q;
    if (RESET) d = ((const float4*)dst)[i];
    float4 o;
    o.x = cn_mask_pick<RESET>(f, q.x, d.x);
    o.y = cn_mask_pick<RESET>(f >> 8, q.y, d.y);
    o.z = cn_mask_pick<RESET>(f >> 16, q.z, d.z);
    o.w = cn_mask_pick<RESET>(f >> 24, q.w, d.w);
    ((float4*)dst)[i] = o;
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(n & 3)) {
    const long i = (n4 << 2) + threadIdx.x;
    dst[i] = cn_mask_pick<RESET>(flags[i], src[i], dst[i]);
  }
}

template <bool RESET>
static int cn_mask_launch(float* dst, const float* src, const unsigned char* flags, long n, void* stream) {
  if (n <= 0) return CN_OK;
  if (dst == nullptr || src == nullptr || flags == nullptr) return CN_ERR_ARG;
  if ((uintptr_t)dst % 16 != 0 || (uintptr_t)src % 16 != 0 || (uintptr_t)flags % 4 != 0) return CN_ERR_ARG;
  long bx = (n + 1023) / 1024;
  if (bx > 4096) bx = 4096;
  CN_LAUNCH(cn_mask_select_kernel<RESET>, dim3((unsigned)bx), dim3(256), 0, (hipStream_t)stream, dst, src, flags, n);
  return cn_check_launch();
}

// dst, src 16-byte aligned, flags 4-byte aligned; dst == src allowed (no other overlap). One launch.
extern "C" int cn_mask_select_f32(float* dst, const float* src, const unsigned char* flags, long n, void* stream) {
  return cn_mask_launch<false>(dst, src, flags, n, stream);
}

extern "C" int cn_prune_reset_f32(float* p, const float* snapshot, const unsigned char* flags, long n, void* stream) {
  if (p == snapshot) return CN_ERR_ARG;
  return cn_mask_launch<true>(p, snapshot, flags, n, stream);
}

// ---- count ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cn_prune_count_kernel(const unsigned char* __restrict__ flags, long n,
                                                             u32* __restrict__ out) {
  __shared__ u32 scratch[256 / CN_WAVE];
  const long n4 = n >> 2;
  const u32* f4 = (const u32*)flags;
  u32 c = 0;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const u32 f = f4[i];
    c += (u32)__popc(f & (f >> 1) & 0x01010101u);
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(n & 3)) c += cn_prune_eligible(flags[(n4 << 2) + threadIdx.x]) ? 1u : 0u;
  c = cn_block_sum<u32, 256>(c, scratch);
  if (threadIdx.x == 0 && c) __hip_atomic_fetch_add(out, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// out[0] += elements with both bits set (the caller zeroes it). flags 4-byte aligned, n < 2^31. One launch.
extern "C" int cn_prune_count_u32(const unsigned char* flags, long n, unsigned int* out, void* stream) {
  if (flags == nullptr || out == nullptr || n <= 0 || n >= (1L << 31)) return CN_ERR_ARG;
  if ((uintptr_t)flags % 4 != 0) return CN_ERR_ARG;
  long bx = (n + 16383) / 16384;
  if (bx > 1024) bx = 1024;
  CN_LAUNCH(cn_prune_count_kernel, dim3((unsigned)bx), dim3(256), 0, (hipStream_t)stream, flags, n, out);
  return cn_check_launch();
}
