// Dataset normalization statistics on the device: what NormValues.from_dataset (utils/normalize.py:118-213) computes on
// the CPU with Variance(method='median') and Quantile(r=6144) (utils/stats.py:236-683), restated over integers.
//
// Stored reflectances are integers and EdgeDataset.get maps them through (x / 10000).clip(1e-9, 1)
// (data/datasets.py:443), so a channel takes at most 10001 distinct values and its histogram over bin = clamp(v, 0, 10000)
// holds everything from_dataset reads: the batch median, the centred second moment, every quantile and the mean.
// Everything written here is an integer and every sum is an integer atomic or a fixed-order sum, so the results do not
// depend on arrival order; the floating-point arithmetic happens once, on the host (cultionet_amd/normalize.py).
//
//   cn_chip_hist_u32       x [B][C][L] -> batch histogram [C][nbins] uint32 (added into)
//   cn_hist_batch_reduce   batch histogram -> one record per channel, dataset histogram += batch histogram, batch
//                          histogram = 0
//   cn_label_counts_i64    y [N] -> class tallies [nlab + 2] int64 (added into)
//
// cn_chip_hist_u32. grid (blocks per channel, C), block CN_HIST_NT, dynamic LDS of nbins words: ONE block-private
// histogram (40 KB at 10001 bins; DESIGN.md has the block sizes and ranges that were timed). A block owns a contiguous
// range of the B * L values of its channel and walks the planes that range meets. Within a plane a span is read as 16-byte vectors
// (8 int16 or 4 int32) from the first 16-byte-aligned address on; the elements before it (an int16 plane starts at a
// 2-byte-aligned address when L is odd) and the elements after the last whole vector are read one per thread.
// Reflectance planes are smooth: a thread merges the run of equal bins it holds -- across the elements of a vector and
// on from one vector to its next -- and issues one LDS atomic per run. The flush adds the NON-ZERO bins only to the
// global histogram, and the host picks the number of blocks per channel so that a block reads at least
// CN_HIST_MIN_PER_BLOCK values: a flush of every bin then costs at most a third of the atomics of the values behind it.
#include "cn_common.h"

#ifndef CN_HIST_NT  // the two tuning constants can be set on the compiler's command line for a timing build
#define CN_HIST_NT 1024
#endif
#ifndef CN_HIST_MIN_PER_BLOCK
#define CN_HIST_MIN_PER_BLOCK 32768L
#endif
#define CN_HIST_MAX_BINS 16384
#define CN_HIST_MAX_BLOCKS 64  // per channel
#define CN_RED_NT 512
#define CN_REC_WORDS 7
#define CN_LAB_NT 256
#define CN_LAB_MAX 1022  // nlab + 2 counters fit one block's static LDS
#define CN_LAB_MAX_BLOCKS 256
#define CN_LAB_STRETCH 16  // labels per thread, at least

typedef unsigned int u32;
typedef unsigned long long u64;
typedef unsigned __int128 u128;

__device__ __forceinline__ int cn_hist_bin(int v, int top) { return v < 0 ? 0 : (v > top ? top : v); }

// DT: 1 int32, 2 int16, 3 uint16 (the codes of cn_prepare_chips_f32)
template <int DT>
struct CnHistElem;
template <>
struct CnHistElem<1> {
  typedef int type;
  static constexpr int VEC = 4;
  static __device__ __forceinline__ int get(const uint4& q, int k) {
    return (int)(k == 0 ? q.x : k == 1 ? q.y : k == 2 ? q.z : q.w);
  }
};
template <>
struct CnHistElem<2> {
  typedef short type;
  static constexpr int VEC = 8;
  static __device__ __forceinline__ int get(const uint4& q, int k) {
    const u32 w = (k >> 1) == 0 ? q.x : (k >> 1) == 1 ? q.y : (k >> 1) == 2 ? q.z : q.w;
    return (int)(short)((k & 1) ? (w >> 16) : (w & 0xffffu));
  }
};
template <>
struct CnHistElem<3> {
  typedef unsigned short type;
  static constexpr int VEC = 8;
  static __device__ __forceinline__ int get(const uint4& q, int k) {
    const u32 w = (k >> 1) == 0 ? q.x : (k >> 1) == 1 ? q.y : (k >> 1) == 2 ? q.z : q.w;
    return (int)((k & 1) ? (w >> 16) : (w & 0xffffu));
  }
};

template <int DT>
__global__ __launch_bounds__(CN_HIST_NT) void cn_chip_hist_kernel(const void* __restrict__ x_, u32* __restrict__ hist, int C,
                                                                  long L, u64 total, u64 per_block, int nbins) {
  typedef CnHistElem<DT> E;
  typedef typename E::type elem_t;
  extern __shared__ u32 bins[];
  const int tid = threadIdx.x, c = blockIdx.y, top = nbins - 1;
  for (int k = tid; k < nbins; k += CN_HIST_NT) bins[k] = 0;
  __syncthreads();

  // this block's values of channel c: n in [n0, n1) of the B * L, n = b * L + l
  const u64 n0 = (u64)blockIdx.x * per_block;
  const u64 n1 = n0 + per_block < total ? n0 + per_block : total;
  CnHistRun run{0, 0};
  u64 n = n0;
  while (n < n1) {
    const u64 b = n / (u64)L, l0 = n - b * (u64)L;
    const u64 room = (u64)L - l0;
    const u64 count = n1 - n < room ? n1 - n : room;  // the span [l0, l0 + count) of plane (b, c)
    const elem_t* p = (const elem_t*)x_ + ((b * (u64)C + (u64)c) * (u64)L + l0);
    // elements in front of the first 16-byte-aligned address (p is aligned to its element)
    u64 head = ((16u - (u32)((uintptr_t)p & 15u)) & 15u) / sizeof(elem_t);
    if (head > count) head = count;
    const u64 nvec = (count - head) / E::VEC;
    const u64 tail0 = head + nvec * E::VEC;
    if ((u64)tid < head) run.add(bins, cn_hist_bin((int)p[tid], top));
    const uint4* pv = (const uint4*)(p + head);
    for (u64 i = tid; i < nvec; i += CN_HIST_NT) {
      const uint4 q = pv[i];
#pragma unroll
      for (int k = 0; k < E::VEC; ++k) run.add(bins, cn_hist_bin(E::get(q, k), top));
    }
    if (tail0 + (u64)tid < count) run.add(bins, cn_hist_bin((int)p[tail0 + tid], top));
    n += count;
  }
  run.flush(bins);
  __syncthreads();

  u32* out = hist + (size_t)c * nbins;
  for (int k = tid; k < nbins; k += CN_HIST_NT) {
    const u32 v = bins[k];
    if (v) __hip_atomic_fetch_add(out + k, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// x: [B][C][L] raw integers (dtype 1 i32, 2 i16, 3 u16; floats are refused) -> hist [C][nbins] uint32, ADDED into:
// hist[c][clamp(v, 0, nbins - 1)] += 1 for every value v of channel c. One launch.
extern "C" int cn_chip_hist_u32(const void* x, int dtype, unsigned int* hist, int B, int C, long L, int nbins, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (x == nullptr || hist == nullptr || B <= 0 || C <= 0 || L <= 0) return CN_ERR_ARG;
  if (dtype < 1 || dtype > 3) return CN_ERR_ARG;
  if (nbins < 2 || nbins > CN_HIST_MAX_BINS || C > 65535) return CN_ERR_ARG;
  if (L >= (1L << 32) || (u64)B * (u64)L >= (1ull << 32)) return CN_ERR_ARG;
  if ((uintptr_t)x % (dtype == 1 ? 4 : 2) != 0) return CN_ERR_ARG;
  const u64 total = (u64)B * (u64)L;
  long nblk = (long)(total / CN_HIST_MIN_PER_BLOCK);
  nblk = nblk < 1 ? 1 : (nblk > CN_HIST_MAX_BLOCKS ? CN_HIST_MAX_BLOCKS : nblk);
  const u64 per_block = (total + nblk - 1) / nblk;
  nblk = (long)((total + per_block - 1) / per_block);
  const dim3 grid((unsigned)nblk, (unsigned)C);
  const size_t lds = (size_t)nbins * sizeof(u32);
  if (dtype == 1)
    CN_LAUNCH(cn_chip_hist_kernel<1>, grid, dim3(CN_HIST_NT), lds, stream, x, hist, C, L, total, per_block, nbins);
  else if (dtype == 2)
    CN_LAUNCH(cn_chip_hist_kernel<2>, grid, dim3(CN_HIST_NT), lds, stream, x, hist, C, L, total, per_block, nbins);
  else
    CN_LAUNCH(cn_chip_hist_kernel<3>, grid, dim3(CN_HIST_NT), lds, stream, x, hist, C, L, total, per_block, nbins);
  return cn_check_launch();
}

// ---- per-batch record -------------------------------------------------------------------------------------
// grid (C), block CN_RED_NT. The channel's batch histogram is staged in LDS; thread t owns the bins [t * per, (t + 1) * per)
// so that an exclusive scan of the threads' counts gives every bin its sorted rank. The two weighted moments are 128-bit
// sums; they cross the block as four 32-bit limbs each, every limb summed in 64 bits (512 limbs cannot overflow).
__device__ __forceinline__ u64 cn_red_block_sum(u64 v, u64* scratch) { return cn_block_sum<u64, CN_RED_NT>(v, scratch); }

__device__ __forceinline__ u128 cn_red_block_sum128(u128 v, u64* scratch) {
  const u64 lo = (u64)v, hi = (u64)(v >> 64);
  const u64 l0 = cn_red_block_sum(lo & 0xffffffffull, scratch), l1 = cn_red_block_sum(lo >> 32, scratch);
  const u64 l2 = cn_red_block_sum(hi & 0xffffffffull, scratch), l3 = cn_red_block_sum(hi >> 32, scratch);
  return (u128)l0 + ((u128)l1 << 32) + ((u128)l2 << 64) + ((u128)l3 << 96);
}

__global__ __launch_bounds__(CN_RED_NT) void cn_hist_batch_reduce_kernel(u32* __restrict__ batch_hist,
                                                                       u64* __restrict__ dataset_hist,
                                                                       const long long* __restrict__ weights,
                                                                       long long* __restrict__ record, int nbins) {
  extern __shared__ u32 h[];  // nbins words
  __shared__ u64 scratch[CN_RED_NT / CN_WAVE];
  __shared__ u64 wave_count[CN_RED_NT / CN_WAVE];
  __shared__ int median_bin;
  const int tid = threadIdx.x, lane = tid & (CN_WAVE - 1), wid = tid / CN_WAVE, c = blockIdx.x;
  u32* bh = batch_hist + (size_t)c * nbins;
  u64* dh = dataset_hist + (size_t)c * nbins;
  for (int k = tid; k < nbins; k += CN_RED_NT) {
    const u32 v = bh[k];
    h[k] = v;
    if (v) dh[k] += v;  // this block is the only writer of the channel's rows
    bh[k] = 0;
  }
  if (tid == 0) median_bin = -1;
  __syncthreads();

  const int per = (nbins + CN_RED_NT - 1) / CN_RED_NT;
  const int k0 = tid * per, k1 = k0 + per < nbins ? k0 + per : nbins;
  u64 mine = 0;
  u128 s1 = 0, s2 = 0;
  for (int k = k0; k < k1; ++k) {
    const u32 v = h[k];
    if (v == 0) continue;
    mine += v;
    const u128 w = (u128)(u64)weights[k];
    const u128 vw = (u128)v * w;
    s1 += vw;
    s2 += vw * w;
  }
  // exclusive scan of `mine` over the block, in bin order
  u64 incl = mine;
#pragma unroll
  for (int off = 1; off < CN_WAVE; off <<= 1) {
    const u64 up = __shfl_up(incl, off, CN_WAVE);
    if (lane >= off) incl += up;
  }
  if (lane == CN_WAVE - 1) wave_count[wid] = incl;
  __syncthreads();
  u64 before = incl - mine, n = 0;
#pragma unroll
  for (int i = 0; i < CN_RED_NT / CN_WAVE; ++i) {
    const u64 wc = wave_count[i];
    before += i < wid ? wc : 0;
    n += wc;
  }
  // the element of sorted rank (n - 1) / 2: torch's lower median
  if (n > 0) {
    const u64 rank = (n - 1) / 2;
    if (before <= rank && rank < before + mine) {
      u64 cum = before;
      for (int k = k0; k < k1; ++k) {
        cum += h[k];
        if (rank < cum) { median_bin = k; break; }
      }
    }
  }
  const u128 t1 = cn_red_block_sum128(s1, scratch);
  const u128 t2 = cn_red_block_sum128(s2, scratch);
  __syncthreads();
  if (tid == 0) {
    long long* r = record + (size_t)c * CN_REC_WORDS;
    r[0] = (long long)n;
    r[1] = (long long)h[0];
    r[2] = median_bin;
    r[3] = (long long)(u64)t1;
    r[4] = (long long)(u64)(t1 >> 64);
    r[5] = (long long)(u64)t2;
    r[6] = (long long)(u64)(t2 >> 64);
  }
}

// batch_hist [C][nbins] uint32 -> records[batch_index][c][7] int64 = {n, count of bin 0, median bin (-1 when n = 0),
// S1 low, S1 high, S2 low, S2 high}, S1 = sum h_k w_k and S2 = sum h_k w_k^2 as 128-bit integers over the caller's
// weights [nbins] (0 <= w_k < 2^40); then dataset_hist [C][nbins] uint64 += batch_hist and batch_hist = 0. One launch.
extern "C" int cn_hist_batch_reduce(unsigned int* batch_hist, unsigned long long* dataset_hist, const long long* weights,
                                    long long* records, int batch_index, int capacity, int C, int nbins, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (batch_hist == nullptr || dataset_hist == nullptr || weights == nullptr || records == nullptr) return CN_ERR_ARG;
  if (C <= 0 || nbins < 2 || nbins > CN_HIST_MAX_BINS) return CN_ERR_ARG;
  if (batch_index < 0 || batch_index >= capacity) return CN_ERR_ARG;
  const size_t lds = (size_t)nbins * sizeof(u32);
  if (lds + 1024 > 64 * 1024)  // with the kernel's static words the block passes 64 KB
    (void)hipFuncSetAttribute((const void*)cn_hist_batch_reduce_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  CN_LAUNCH(cn_hist_batch_reduce_kernel, dim3(C), dim3(CN_RED_NT), lds, stream, batch_hist, dataset_hist, weights,
            records + (size_t)batch_index * C * CN_REC_WORDS, nbins);
  return cn_check_launch();
}

// ---- class tallies ----------------------------------------------------------------------------------------
__device__ __forceinline__ long long cn_stats_label(const void* y, int ydtype, u64 i) {
  switch (ydtype) {
    case 1: return ((const int*)y)[i];
    case 2: return ((const short*)y)[i];
    case 3: return ((const unsigned short*)y)[i];
    default: return ((const long long*)y)[i];
  }
}

// grid (blocks), block CN_LAB_NT: a block tallies a contiguous range into LDS (a thread merges the run of equal classes it
// meets over its own contiguous stretch: label planes are mostly constant), then flushes its non-zero counters.
__global__ __launch_bounds__(CN_LAB_NT) void cn_label_counts_kernel(const void* __restrict__ y, int ydtype, u64 N,
                                                                   u64 per_thread, u64* __restrict__ counts, int nlab) {
  __shared__ u32 tally[CN_LAB_MAX + 2];
  const int tid = threadIdx.x, nc = nlab + 2;
  for (int k = tid; k < nc; k += CN_LAB_NT) tally[k] = 0;
  __syncthreads();
  const u64 i0 = ((u64)blockIdx.x * CN_LAB_NT + tid) * per_thread;
  const u64 i1 = i0 + per_thread < N ? i0 + per_thread : N;
  CnHistRun run{0, 0};
  for (u64 i = i0; i < i1; ++i) {
    const long long v = cn_stats_label(y, ydtype, i);
    run.add(tally, v < 0 ? 0 : (v >= nlab ? nlab + 1 : (int)v + 1));
  }
  run.flush(tally);
  __syncthreads();
  for (int k = tid; k < nc; k += CN_LAB_NT) {
    const u32 v = tally[k];
    if (v) __hip_atomic_fetch_add(counts + k, (u64)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// y: [N] labels (ydtype 1 i32, 2 i16, 3 u16, 4 i64) -> counts [nlab + 2] int64, ADDED into: counts[0] for v < 0,
// counts[1 + v] for 0 <= v < nlab, counts[nlab + 1] for v >= nlab. One launch.
extern "C" int cn_label_counts_i64(const void* y, int ydtype, long N, long long* counts, int nlab, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (y == nullptr || counts == nullptr || N <= 0) return CN_ERR_ARG;
  if (ydtype < 1 || ydtype > 4 || nlab < 1 || nlab > CN_LAB_MAX) return CN_ERR_ARG;
  long nblk = (N + CN_LAB_NT * (long)CN_LAB_STRETCH - 1) / (CN_LAB_NT * (long)CN_LAB_STRETCH);
  nblk = nblk > CN_LAB_MAX_BLOCKS ? CN_LAB_MAX_BLOCKS : nblk;
  const u64 per_thread = ((u64)N + (u64)nblk * CN_LAB_NT - 1) / ((u64)nblk * CN_LAB_NT);
  if (per_thread * CN_LAB_NT >= (1ull << 32)) return CN_ERR_ARG;
  CN_LAUNCH(cn_label_counts_kernel, dim3((unsigned)nblk), dim3(CN_LAB_NT), 0, stream, y, ydtype, (u64)N, per_thread,
            (u64*)counts, nlab);
  return cn_check_launch();
}
