// The body of the 16-byte LDS-DMA ("flattened rows") fp32 weight-gradient kernels. NOT a header: cn_wgrad.hip includes
// this text once inside each of cn_wgrad_vec_kernel<1, S_> (KR = 1) and cn_wgrad_vec3_kernel<S_> (KR = 3), with
//   constexpr int KR   kernel rows = taps per wave (a wave owns one kernel row ky of a KR x KR kernel), 4 * KR waves
//   int S_             stride (template parameter of both kernels)
//   S0, Bg0, dW0, g    the kernels' arguments
// in scope. It is compiled as part of the kernel itself on purpose: the same text as a __forceinline__ __device__
// function called from the two kernels costs the 3 x 3 kernel 870 instructions and its last spare register
// ("One body for the 16-byte weight-gradient kernels").
//
// Wave = (k-part, kernel row, cout tile): the waves of one (cout tile, kernel row) are a_tiles * KR apart.
// Columns of a wave's tile: n = j * 32 + lane % 32 (j < KR), channel n / KR, tap ky * KR + n % KR -- dW runs of KR floats.
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NW = 4 * KR;                    // waves per block
  constexpr int KS = (WG_DS + NW - 1) / NW;     // DMA instructions per wave for the S image  (8 / 3)
  constexpr int KB = (WG_DB + NW - 1) / NW;     // DMA instructions per wave for the Bg image (16 / 6)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, l31 = lane & 31;
  const int at = wid % g.a_tiles;
  const int ky = (wid / g.a_tiles) % KR;
  const int kp = wid / (g.a_tiles * KR), kparts = NW / (g.a_tiles * KR);
  int bx, by, bz;
  if (!cn_xcd_block(g.grid_x, g.grid_y, g.grid_x * g.grid_y * g.grid_z, bx, by, bz)) return;
  const int grp = g.G > 1 ? bz / g.spg : 0;
  const int split = bz - grp * g.spg;
  const float* __restrict__ S = g.G > 1 ? g.gS[grp] : S0;
  const float* __restrict__ Bg = g.G > 1 ? g.gB[grp] : Bg0;
  float* __restrict__ dW = (g.G > 1 && g.slice_stride == 0) ? g.gdW[grp] : dW0;
  const int a0 = by * g.a_tiles * 32;
  const int b0 = bx * WG_BC;
  const int npix = g.PR * g.Ws;    // unpadded, even, multiple of 4
  const int n4s = npix >> 2;       // float4 pieces per S row (<= 64)
  const int n4b = g.plane_b >> 2;  // float4 pieces per Bg channel image
  const float* zero = cn_zero_line16 + 4 * lane;

  int boff[KR], ox[KR];
#pragma unroll
  for (int j = 0; j < KR; ++j) {
    const int n = j * 32 + l31;
    const int bl = n / KR, t = ky * KR + (n - bl * KR);
    boff[j] = bl * g.plane_b + (g.offy[t] - g.min_oy) * g.Wb + (g.offx[t] - g.min_ox) + half * g.s;
    ox[j] = g.offx[t] + half * g.s;
  }
  const int aoff = (at * 32 + l31) * g.pitch_s + half;

  f32x16 acc[KR];
#pragma unroll
  for (int j = 0; j < KR; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  const int arows = g.a_tiles * 32;
  int chunk = split * g.chunks_per_split;
  int chunk_end = chunk + g.chunks_per_split;
  if (chunk_end > g.total_chunks) chunk_end = g.total_chunks;

  // dense LDS images: S [arows][npix], Bg [WG_BC][plane_b]; piece p of an image = its p-th 16 bytes, so one
  // DMA wave-instruction (64 consecutive pieces = 1 KiB) may span several rows / channels.
  // Per-lane BYTE offset of this lane's piece in DMA instruction k, relative to the chunk's base address (S: first
  // pixel of the chunk in channel 0 of image n; Bg: the 16-byte aligned start of the halo in channel 0), or WG_IDLE
  // for lanes past the image / past the channel count (their LDS rows only feed dW entries that are never stored).
  // Interior chunks -- all but the first / last rows of an image -- then stage with ONE instruction per KiB: scalar
  // base + per-lane offset, no per-chunk address arithmetic or bound checks (those took ~3000 cycles per chunk with
  // the matrix pipe idle: one wave per SIMD). Boundary chunks re-derive the piece index and zero-fill per piece.
  // (Measured and not kept, four waves, nine taps per wave: issuing an interior chunk's DMA instructions singly between
  // the MFMA groups instead of back to back -- each then stalls the wave ~330 instead of ~126 cycles: 252 -> 311 us at
  // 128->128, 100^2.)
  constexpr unsigned WG_IDLE = 0xFFFFFFFFu;
  unsigned so[KS], bo[KB];
  {
    const int nsp = arows * n4s, nbp = WG_BC * n4b;
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      const int p = (wid + NW * k) * 64 + lane;
      const int a = p / n4s, pc = p - a * n4s;
      so[k] = (p < nsp && (a0 + a) < g.A) ? (unsigned)(((long)(a0 + a) * g.scs + 4 * pc) * 4) : WG_IDLE;
    }
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      const int p = (wid + NW * k) * 64 + lane;
      const int bl = p / n4b, pi = p - bl * n4b;
      bo[k] = (p < nbp && (b0 + bl) < g.Bc) ? (unsigned)(((long)(b0 + bl) * g.bcs + 4 * pi) * 4) : WG_IDLE;
    }
  }
  // One unrolled loop over this wave's DMA instructions of an image; piece p reads zeros unless OK_; `inside` is wave-
  // uniform. KR == 1 (one wave per SIMD pays for every instruction): the test once, around the loop, the fill a select.
  // KR == 3 (three waves hide it): one loop. NOT interchangeable -- under WG_DMA3's spelling, hoisted or not, the 1 x 1
  // kernel runs 2-4 % slower (480->128, 8 x 100^2: 149.1 -> 152.2 / 154.8 us); under WG_DMA's the 3 x 3 one grows.
#define WG_DMA(N_, off_, lim_, base_, lds_, OK_)                                          \
  _Pragma("unroll") for (int k = 0; k < N_; ++k) {                                        \
    if ((wid + NW * k) * 64 < lim_ && off_[k] != WG_IDLE) {                               \
      const int p = (wid + NW * k) * 64 + lane;                                           \
      const float* src = (OK_) ? reinterpret_cast<const float*>(base_ + off_[k]) : zero;  \
      cn_glds16(src, lds_ + (wid + NW * k) * 256);                                        \
    }                                                                                     \
  }
#define WG_DMA3(N_, off_, lim_, base_, lds_, OK_)                                         \
  _Pragma("unroll") for (int k = 0; k < N_; ++k) {                                        \
    if ((wid + NW * k) * 64 < lim_ && off_[k] != WG_IDLE) {                               \
      const float* src = reinterpret_cast<const float*>(base_ + off_[k]);                 \
      if (!inside) {                                                                      \
        const int p = (wid + NW * k) * 64 + lane;                                         \
        if (!(OK_)) src = zero;                                                           \
      }                                                                                   \
      cn_glds16(src, lds_ + (wid + NW * k) * 256);                                        \
    }                                                                                     \
  }
#define WG_STAGE(N_, off_, lim_, base_, lds_, OK_)                                        \
  if constexpr (KR == 1) {                                                                \
    if (inside) { WG_DMA(N_, off_, lim_, base_, lds_, true) }                             \
    else { WG_DMA(N_, off_, lim_, base_, lds_, OK_) }                                     \
  } else {                                                                                \
    WG_DMA3(N_, off_, lim_, base_, lds_, OK_)                                             \
  }
  auto stage = [&](int ck, int buf) {
    float* s_lds = smem + buf * g.buf_stride;
    float* b_lds = s_lds + g.b_lds_off;
    const int n = ck / g.chunks_per_img;
    const int gy0 = (ck - n * g.chunks_per_img) * g.PR;
    const int nsp = arows * n4s, nbp = WG_BC * n4b;
    {
      const int fs0 = gy0 * g.Ws;
      const char* sbase = reinterpret_cast<const char*>(S + (long)n * g.sbs + fs0);
      const bool inside = fs0 + npix <= (int)g.scs;  // the whole chunk lies inside the plane
      WG_STAGE(KS, so, nsp, sbase, s_lds, (fs0 + 4 * (p % n4s) + 3) < (int)g.scs)
    }
    {
      const int start = (gy0 * g.s + g.min_oy) * g.Wb + g.min_ox;
      const int f0 = (start >> 2) << 2;
      const char* bbase = reinterpret_cast<const char*>(Bg + (long)n * g.bbs + f0);
      const bool inside = f0 >= 0 && f0 + g.plane_b <= (int)g.bcs;  // the halo lies inside the plane
      WG_STAGE(KB, bo, nbp, bbase, b_lds, f0 + 4 * (p % n4b) >= 0 && (f0 + 4 * (p % n4b) + 3) < (int)g.bcs)
    }
  };
#undef WG_STAGE
#undef WG_DMA3
#undef WG_DMA

  int cur = 0;
  if (chunk < chunk_end && g.nbuf == 2) stage(chunk, 0);
  for (; chunk < chunk_end; ++chunk) {
    if (g.nbuf == 1) {
      __syncthreads();
      stage(chunk, 0);
    }
    __syncthreads();
    // (3 x 3: the barrier puts the three waves of a SIMD in the same phase. Skewing them -- the waves of kernel row ky start
    // ky * 512 / 1024 / 2048 / 4096 cycles late -- was measured: 239 -> 245 / 245 / 249 / 260 us at 128 -> 128, 8 x 100^2;
    // moving a wave's DMA issue into its group pipeline costs registers the three-waves budget does not have.)
    // (Round 5, measured with tools/wgrad_bench.py at 8 x 100^2, same box: (a) the next chunk's nine DMA instructions
    // spread through this chunk's MFMA loop, three per iteration, 168 registers without scratch once the source pointers
    // were kept from being hoisted: 128 -> 128 240 -> 280 us, 160 -> 128 270-292 -> 346 us -- a DMA issue inside the
    // loop stalls the wave's in-order MFMA stream; (b) progress-based issue priority, s_setprio 3..0 by quarter of the
    // row so that the wave that is behind is served first: the three waves of a SIMD then finish their row together and
    // the chunk takes exactly as long: 243.0 -> 242.2 us, 160 -> 128 268.5 -> 297.4 us. Neither kept. Under this kernel the
    // shader clock reads ~1.97 GHz (s_memtime against the event time of the launch), not 2.4: its 0.62 of the nominal
    // f32 peak is ~0.75 of what the matrix pipes can deliver at that clock.)
    if (g.nbuf == 2 && chunk + 1 < chunk_end) stage(chunk + 1, cur ^ 1);
    const float* s_lds = smem + cur * g.buf_stride;
    const float* b_lds = s_lds + g.b_lds_off;
    const int gy0c = (chunk % g.chunks_per_img) * g.PR;
    const int start = (gy0c * g.s + g.min_oy) * g.Wb + g.min_ox;
    const int sh = start - ((start >> 2) << 2);
    // A wave issues everything in order, so instructions-per-MFMA bounds this loop: the pixel pairs of a row are
    // walked in unrolled groups whose LDS offsets are compile-time immediates (stride S_), bases are bumped once per
    // group, and the column masks are applied only on the first / last pairs of an image row.
    // The pixel pairs of every row are split over the k-part waves; pairs [0, mq_lo) and [mq_hi, nq_row) of a row can
    // reach outside [0, Wb) for some tap -> masked steps.
    const int nq_row = g.Ws >> 1;
    const int q_lo = (nq_row * kp) / kparts, q_hi = (nq_row * (kp + 1)) / kparts;
    const int seg0 = min(max(g.mq_lo, q_lo), q_hi), seg1 = max(min(g.mq_hi, q_hi), seg0);
    for (int r = 0; r < g.PR; ++r) {
      const float* ap = s_lds + aoff + r * g.Ws;  // indexed by absolute column
      const float* bp[KR];
#pragma unroll
      for (int j = 0; j < KR; ++j) bp[j] = b_lds + boff[j] + sh + (r * S_) * g.Wb;
      int q = q_lo;
      // masked and left-over single pairs: all KR + 1 operands are read before the first MFMA (read / wait / MFMA per
      // tap exposed one LDS round trip in front of every MFMA of the pair)
      for (; q < seg0; ++q) {  // leading masked pairs
        const float av = ap[2 * q];
        const int cs = 2 * q * S_;
        float bv[KR];
#pragma unroll
        for (int j = 0; j < KR; ++j) bv[j] = bp[j][cs];
#pragma unroll
        for (int j = 0; j < KR; ++j) {
          const float b_ = ((unsigned)(cs + ox[j]) < (unsigned)g.Wb) ? bv[j] : 0.f;
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b_, acc[j], 0, 0, 0);
        }
      }
      // interior pairs: no masks, immediate offsets
      if constexpr (KR == 1) {
        // one MFMA per k-step: the register pipeline below was measured slower (172 vs 161 us at 480->128, 100^2)
        for (; q + WG_U <= seg1; q += WG_U) {
          const float* apq = ap + 2 * q;
#pragma unroll
          for (int u = 0; u < WG_U; ++u)
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(apq[2 * u], (bp[0] + 2 * q * S_)[2 * u * S_], acc[0], 0, 0, 0);
        }
      } else {
        // Groups of GS k-steps with the operands double-buffered in registers: the LDS reads of the NEXT group are issued
        // before the GS * KR MFMAs of the current one; without this every group waited out the full LDS latency with
        // the matrix pipe idle (the compiler emitted read-all / s_waitcnt 0 / MFMA-all). (Folding the edge pairs into
        // this pipeline as well was measured slower, four waves, nine taps per wave: 252 -> 273 us at 128->128, 100^2
        // -- the extra live operands cost more moves than the two exposed LDS round trips per row.)
        // (A conflict-free A operand -- one ds_read_b128 per lane for four k-steps + two v_permlane32_swap, instead of
        // four dwords at a row pitch that puts 32 couts on 8 banks -- was built and measured: 239 -> 251 us at 128 -> 128,
        // 855 -> 899 at 480 -> 128, step 388 -> 383 chips/s: the bank conflicts are not what idles the pipe. Note for the
        // next attempt: __builtin_bit_cast(unsigned, v[i]) of an ext_vector ELEMENT expression yields element 0 / undef
        // with this compiler; copy the element to a scalar first.)
        constexpr int GS = 3;
        const int ng = (seg1 - q) / GS;
        if (ng > 0) {
          float a0[GS], a1[GS], b0[GS][KR], b1[GS][KR];
#define WG_LOADG(qq_, a_, b_)                                                    \
  {                                                                              \
    const float* apq_ = ap + 2 * (qq_);                                          \
    _Pragma("unroll") for (int u = 0; u < GS; ++u) a_[u] = apq_[2 * u];          \
    _Pragma("unroll") for (int j = 0; j < KR; ++j) {                             \
      const float* bq_ = bp[j] + 2 * (qq_) * S_;                                 \
      _Pragma("unroll") for (int u = 0; u < GS; ++u) b_[u][j] = bq_[2 * u * S_]; \
    }                                                                            \
  }
#define WG_MFMAG(a_, b_)                                                                                   \
  {                                                                                                        \
    _Pragma("unroll") for (int u = 0; u < GS; ++u)                                                         \
        _Pragma("unroll") for (int j = 0; j < KR; ++j)                                                     \
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_[u], b_[u][j], acc[j], 0, 0, 0);               \
  }
          WG_LOADG(q, a0, b0);
          int i = 0;
          for (; i + 2 <= ng; i += 2) {
            WG_LOADG(q + GS * (i + 1), a1, b1);
            WG_MFMAG(a0, b0);
            if (i + 2 < ng) WG_LOADG(q + GS * (i + 2), a0, b0);
            WG_MFMAG(a1, b1);
          }
          if (i < ng) WG_MFMAG(a0, b0);
#undef WG_LOADG
#undef WG_MFMAG
          q += GS * ng;
        }
      }
      for (; q < seg1; ++q) {  // left-over pairs
        const float av = ap[2 * q];
        float bv[KR];
#pragma unroll
        for (int j = 0; j < KR; ++j) bv[j] = bp[j][2 * q * S_];
#pragma unroll
        for (int j = 0; j < KR; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[j], acc[j], 0, 0, 0);
      }
      for (; q < q_hi; ++q) {  // trailing masked pairs
        const float av = ap[2 * q];
        const int cs = 2 * q * S_;
        float bv[KR];
#pragma unroll
        for (int j = 0; j < KR; ++j) bv[j] = bp[j][cs];
#pragma unroll
        for (int j = 0; j < KR; ++j) {
          const float b_ = ((unsigned)(cs + ox[j]) < (unsigned)g.Wb) ? bv[j] : 0.f;
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b_, acc[j], 0, 0, 0);
        }
      }
    }
    if (g.nbuf == 2) cur ^= 1;
  }

  // the k-part waves of a (cout tile, kernel row) hold partial sums of the SAME dW tile: add them up through LDS
  // (free after the main loop) so the block writes its tile once
  if (kparts > 1) {
    __syncthreads();
    float* red = smem;
    const int slot = ky * g.a_tiles + at;  // (cout tile, kernel row) within the block
    if (kp > 0) {
      float* rp = red + (long)((kp - 1) * g.a_tiles * KR + slot) * (KR * 16 * 64) + lane;
#pragma unroll
      for (int j = 0; j < KR; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) rp[(j * 16 + r) * 64] = acc[j][r];
    }
    __syncthreads();
    if (kp > 0) return;
    for (int k = 1; k < kparts; ++k) {
      const float* rp = red + (long)((k - 1) * g.a_tiles * KR + slot) * (KR * 16 * 64) + lane;
#pragma unroll
      for (int j = 0; j < KR; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] += rp[(j * 16 + r) * 64];
    }
  }
  // many splits on a small dW: same-address float atomics serialise (~200 ns each), so each split stores its
  // partial into a private workspace slice instead and cn_wgrad_reduce_kernel sums the slices
  float* dWs = dW + (long)bz * g.slice_stride;
#pragma unroll
  for (int j = 0; j < KR; ++j) {
    const int n = j * 32 + l31;
    const int bl = n / KR, t = ky * KR + (n - bl * KR);
    const bool bok = (b0 + bl) < g.Bc;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int a = a0 + at * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      if (bok && a < g.A) {
        float* d = (g.slice_stride != 0 ? dWs : dW) + (long)a * g.sa + (long)(b0 + bl) * (KR * KR) + t;
        if (g.slice_stride != 0) *d = acc[j][r];
        else atomicAdd(d, acc[j][r]);
      }
    }
  }
