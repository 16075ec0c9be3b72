// Parcel labelling on the device: the 4-connected components of the crop pixels of y, numbered as
// scipy.ndimage.label numbers them (np.uint8(nd_label(y == 1)[0]) + regionprops, data/datasets.py:453-466, is what the
// five parcel augmenters of EdgeDataset.get start from): background 0, parcels 1..n in raster order of their first
// pixel, counts[b] = n.
//
// One workgroup per sample and one kernel body for every plane size. The union-find forest is a plane of H * W ints: in
// LDS when it fits CN_LBL_LDS_PIXELS (the training chip, 100 x 100, does), in the caller's `labels` plane otherwise. The
// phases below are chains of dependent reads of that plane, a handful per pixel and ten pixels per thread at 100 x 100,
// so the kernel runs at the plane's latency: that is what the LDS instance is for.
//   1. init     L[i] = start of i's horizontal run inside its 64-pixel wave segment (one ballot), -1 on background
//   2. union    runs that continue across a segment boundary, and each pixel with the pixel above it -- skipped when the
//               left and upper-left pixels are foreground too (the left pixel has made that link already). A link always
//               goes from the larger root to the smaller one (atomicMin), so the root of a component is its smallest
//               pixel index whatever the thread order: the result is deterministic.
//   3. flatten  L[i] = root(i)
//   4. rank     block-wide exclusive prefix sum of the root flags over raster-order tiles of CN_LBL_NT pixels; a root
//               keeps -(rank + 2) so that it stays distinguishable from background (-1) and from links (>= 0)
//   5. write    non-roots read their root's rank, then the negative entries (roots, background) are rewritten
// The phases are separated by __syncthreads(); the forest is always read with relaxed atomic loads (agent scope in global
// memory), so that a link made by another wave's atomic minimum is never served from a stale cache line.
#include "cn_common.h"

#define CN_LBL_NT 1024
#define CN_LBL_WAVES (CN_LBL_NT / CN_WAVE)
#define CN_LBL_LDS_PIXELS ((64 * 1024 - 256) / 4)  // dynamic LDS of one workgroup, less the scan's own words

// The forest plane: L points into LDS (SCOPE workgroup) or into global memory (SCOPE agent).
template <int SCOPE>
struct CnLblPlane {
  int* L;
  __device__ __forceinline__ int get(int i) const { return __hip_atomic_load(L + i, __ATOMIC_RELAXED, SCOPE); }
  __device__ __forceinline__ void put(int i, int v) const { __hip_atomic_store(L + i, v, __ATOMIC_RELAXED, SCOPE); }
  __device__ __forceinline__ int find(int a) const {
    for (int p = get(a); p != a; p = get(a)) a = p;
    return a;
  }
  // a and b are foreground pixels of one component-to-be
  __device__ __forceinline__ void unite(int a, int b) const {
    for (;;) {
      a = find(a);
      b = find(b);
      if (a == b) return;
      if (a < b) { const int t = a; a = b; b = t; }
      // a was a root when found; it may have been linked elsewhere since
      const int old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, SCOPE);
      if (old == a) return;
      a = old;
    }
  }
};

__device__ __forceinline__ long long cn_lbl_load(const void* y, int ydtype, long i) {
  switch (ydtype) {
    case 1: return ((const int*)y)[i];
    case 2: return ((const short*)y)[i];
    case 3: return ((const unsigned short*)y)[i];
    default: return ((const long long*)y)[i];
  }
}

// grid (B), block CN_LBL_NT; IN_LDS: dynamic LDS of H * W ints
template <bool IN_LDS>
__global__ __launch_bounds__(CN_LBL_NT) void cn_label_parcels_kernel(const void* __restrict__ y, int ydtype, long long crop,
                                                                    int* __restrict__ labels, int* __restrict__ counts,
                                                                    int H, int W) {
  extern __shared__ int forest[];
  __shared__ int wave_total[2][CN_LBL_WAVES];
  const int tid = threadIdx.x, lane = tid & (CN_WAVE - 1), wid = tid / CN_WAVE;
  const unsigned HW = (unsigned)H * (unsigned)W;  // < 2^31: base + tid and i + CN_LBL_NT below stay inside 32 bits
  const long plane = (long)blockIdx.x * HW;
  int* out = labels + plane;
  const CnLblPlane<IN_LDS ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT> f{IN_LDS ? forest : out};

  // 1. every lane of a wave takes part in the ballot; lanes past the plane are background.
  // The column of pixel i = base + tid is carried from tile to tile: one workgroup does all the arithmetic of a plane,
  // and a division per pixel in this phase and the next measured 1 us of 26 at 100 x 100.
  const unsigned w0 = (unsigned)tid % (unsigned)W, wstep = CN_LBL_NT % (unsigned)W;
  unsigned w = w0;
  for (unsigned base = 0; base < HW; base += CN_LBL_NT, w = w + wstep >= (unsigned)W ? w + wstep - W : w + wstep) {
    const unsigned i = base + tid;
    const bool fg = i < HW && cn_lbl_load(y, ydtype, plane + i) == crop;
    const unsigned long long fgm = __ballot(fg);
    const bool begins = fg && (lane == 0 || w == 0 || !((fgm >> (lane - 1)) & 1ull));
    const unsigned long long bm = __ballot(begins) & (~0ull >> (CN_WAVE - 1 - lane));  // run starts at or below this lane
    if (i < HW) f.L[i] = fg ? (int)(i - lane) + (CN_WAVE - 1 - __clzll(bm)) : -1;
  }
  __syncthreads();

  // 2. the sign of an entry never changes in this phase, so the foreground tests are stable
  w = w0;
  for (unsigned i = tid; i < HW; i += CN_LBL_NT, w = w + wstep >= (unsigned)W ? w + wstep - W : w + wstep) {
    if (f.get(i) < 0) continue;
    const bool left = w > 0 && f.get(i - 1) >= 0;
    if (left && (i & (CN_WAVE - 1)) == 0) f.unite((int)i, (int)i - 1);
    if (i >= (unsigned)W && f.get(i - W) >= 0 && !(left && f.get(i - W - 1) >= 0)) f.unite((int)i, (int)i - W);
  }
  __syncthreads();

  // 3. a concurrent reader sees either the old link or the root: both lead to the root
  for (unsigned i = tid; i < HW; i += CN_LBL_NT) {
    if (f.get(i) >= 0) f.put(i, f.find((int)i));
  }
  __syncthreads();

  // 4. each thread reads and writes its own pixel only
  int running = 0, buf = 0;
  for (unsigned base = 0; base < HW; base += CN_LBL_NT, buf ^= 1) {
    const unsigned i = base + tid;
    const bool root = i < HW && f.get(i) == (int)i;
    const unsigned long long rm = __ballot(root);
    if (lane == 0) wave_total[buf][wid] = __popcll(rm);
    __syncthreads();  // the other buffer is still being read by waves that are one tile behind
    int before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < CN_LBL_WAVES; ++k) {
      const int n = wave_total[buf][k];
      before += k < wid ? n : 0;
      total += n;
    }
    if (root) f.L[i] = -(running + before + __popcll(rm & ((1ull << lane) - 1ull)) + 2);
    running += total;
  }
  if (tid == 0) counts[blockIdx.x] = running;
  __syncthreads();

  // 5. links point at roots, roots are negative: non-roots first, then everything negative. (With the forest in the
  // output plane the first pass overwrites links, never a root; with the forest in LDS nothing of it is overwritten.)
  for (unsigned i = tid; i < HW; i += CN_LBL_NT) {
    const int v = f.get(i);
    if (v >= 0) out[i] = -f.get(v) - 1;
  }
  __syncthreads();
  for (unsigned i = tid; i < HW; i += CN_LBL_NT) {
    const int v = f.get(i);
    if (v < 0) out[i] = -v - 1;
  }
}

// y: [B][H][W] labels (ydtype: 1 i32, 2 i16, 3 u16, 4 i64), foreground y == crop_value, 4-neighbour connectivity ->
// labels [B][H][W] int32 (0 background, 1..n in raster order of the first pixel), counts [B] = n. One launch, no
// allocation, no synchronisation; the caller owns both outputs.
extern "C" int cn_label_parcels_i32(const void* y, int ydtype, long long crop_value, int* labels, int* counts, int B, int H,
                                    int W, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (y == nullptr || labels == nullptr || counts == nullptr) return CN_ERR_ARG;
  if (ydtype < 1 || ydtype > 4 || B <= 0 || H <= 0 || W <= 0) return CN_ERR_ARG;
  if ((long)H * W >= (1L << 31)) return CN_ERR_ARG;
  const long HW = (long)H * W;
  if (HW <= CN_LBL_LDS_PIXELS)
    CN_LAUNCH(cn_label_parcels_kernel<true>, dim3(B), dim3(CN_LBL_NT), (size_t)HW * sizeof(int), stream, y, ydtype, crop_value,
              labels, counts, H, W);
  else
    CN_LAUNCH(cn_label_parcels_kernel<false>, dim3(B), dim3(CN_LBL_NT), 0, stream, y, ydtype, crop_value, labels, counts, H, W);
  return cn_check_launch();
}
