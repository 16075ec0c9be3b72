// Stand-alone check of the host-side convolution geometry (cultionet_amd/csrc/cn_conv_geom.h) against brute-force
// definitions. Built and run by tests/test_conv_geom.py with -fsanitize=address,undefined; includes nothing else of the
// library. Prints one line "<check> cases=<n> failures=<m>" per check and exits non-zero when anything failed.
//
// Ranges: kernel 1..3 per axis, stride 1..4, pad 0..2, dilation 1..3, output sizes 1..9 per axis (sizes below the stride
// leave parity classes empty).
#include <algorithm>
#include <array>
#include <cstdio>
#include <vector>

#include "cn_conv_geom.h"

namespace {

struct Check {
  const char* name;
  long cases = 0, failures = 0;
  void fail(const char* what, int a = 0, int b = 0, int c = 0, int d = 0, int e = 0, int f = 0) {
    if (failures++ < 5) std::fprintf(stderr, "%s: %s (%d %d %d %d %d %d)\n", name, what, a, b, c, d, e, f);
  }
  int report() const {
    std::printf("%s cases=%ld failures=%ld\n", name, cases, failures);
    return failures != 0;
  }
};

struct Class {  // what both launch builders keep of a parity class, plus its place in the enumeration
  int py, px, Hg, Wg, ntaps, seq;
  int dy[CN_MAX_TAPS], dx[CN_MAX_TAPS], wt[CN_MAX_TAPS];
};

using Tap = std::array<int, 3>;  // (input y, input x, weight index)

constexpr int IN_LO = -12, IN_HI = 16;  // covers every (o + pad - k*dil) / s of the ranges above

// Scatter form from its forward definition, per axis: input i and tap k write output i*s + k*dil - pad. Returns the
// (i, k) pairs that write output o.
std::vector<std::array<int, 2>> scatter_sources_1d(int o, int K, int s, int pad, int dil) {
  std::vector<std::array<int, 2>> v;
  for (int k = 0; k < K; ++k)
    for (int i = IN_LO; i <= IN_HI; ++i)
      if (i * s + k * dil - pad == o) v.push_back({i, k});
  return v;
}

}  // namespace

int main() {
  Check cover{"cover"}, taps{"taps"}, order{"order"}, gather{"gather"}, sizes{"sizes"}, fdiv{"floordiv"};

  for (int KH = 1; KH <= 3; ++KH)
  for (int KW = 1; KW <= 3; ++KW)
  for (int s = 1; s <= 4; ++s)
  for (int pad = 0; pad <= 2; ++pad)
  for (int dil = 1; dil <= 3; ++dil) {
    // ---- dense tap table of the gather form: input = o*stride + k*dil - pad, weight index ky*KW + kx
    {
      ++gather.cases;
      int dy[CN_MAX_TAPS], dx[CN_MAX_TAPS], wt[CN_MAX_TAPS];
      const int n = cn_gather_taps(KH, KW, pad, dil, dy, dx, wt);
      if (n != KH * KW) gather.fail("tap count", KH, KW, n);
      for (int ky = 0; ky < KH; ++ky)
        for (int kx = 0; kx < KW; ++kx) {
          const int t = ky * KW + kx;
          if (dy[t] != ky * dil - pad || dx[t] != kx * dil - pad || wt[t] != t) gather.fail("tap", KH, KW, pad, dil, t);
        }
    }
    std::vector<std::array<int, 2>> srcy[9], srcx[9];
    for (int o = 0; o < 9; ++o) {
      srcy[o] = scatter_sources_1d(o, KH, s, pad, dil);
      srcx[o] = scatter_sources_1d(o, KW, s, pad, dil);
    }
    for (int Ho = 1; Ho <= 9; ++Ho)
    for (int Wo = 1; Wo <= 9; ++Wo) {
      // ---- enumerate the parity classes the way both launch builders do
      std::vector<Class> cls;
      for (int py = 0; py < s; ++py)
        for (int px = 0; px < s; ++px) {
          Class k = {};
          k.py = py; k.px = px;
          k.Hg = cn_parity_extent(Ho, py, s);
          k.Wg = cn_parity_extent(Wo, px, s);
          if (k.Hg <= 0 || k.Wg <= 0) continue;
          k.ntaps = cn_parity_taps(py, px, KH, KW, s, pad, dil, k.dy, k.dx, k.wt);
          k.seq = (int)cls.size();
          cls.push_back(k);
        }
      // ---- every output position belongs to exactly one class
      ++cover.cases;
      std::vector<int> owner(Ho * Wo, -1);
      for (const Class& k : cls)
        for (int gy = 0; gy < k.Hg; ++gy)
          for (int gx = 0; gx < k.Wg; ++gx) {
            const int oy = gy * s + k.py, ox = gx * s + k.px;
            if (oy >= Ho || ox >= Wo) { cover.fail("outside", Ho, Wo, s, oy, ox); continue; }
            if (owner[oy * Wo + ox] != -1) cover.fail("twice", Ho, Wo, s, oy, ox);
            owner[oy * Wo + ox] = k.seq;
          }
      for (int o = 0; o < Ho * Wo; ++o)
        if (owner[o] == -1) cover.fail("unowned", Ho, Wo, s, o);
      // ---- a class's taps are exactly the brute-force (input offset, k) pairs, each once
      for (const Class& k : cls) {
        if (k.ntaps < 0 || k.ntaps > KH * KW) { taps.fail("count", KH, KW, s, pad, dil, k.ntaps); continue; }
        for (int gy = 0; gy < k.Hg; ++gy)
          for (int gx = 0; gx < k.Wg; ++gx) {
            ++taps.cases;
            std::vector<Tap> got;
            for (int t = 0; t < k.ntaps; ++t) got.push_back({gy + k.dy[t], gx + k.dx[t], k.wt[t]});
            std::sort(got.begin(), got.end());
            std::vector<Tap> want;  // the 2-D sources are the products of the per-axis ones, weight index ky*KW + kx
            for (const auto& y : srcy[gy * s + k.py])
              for (const auto& x : srcx[gx * s + k.px]) want.push_back({y[0], x[0], y[1] * KW + x[1]});
            std::sort(want.begin(), want.end());
            if (got != want)
              taps.fail("mismatch", KH * 10 + KW, s, pad, dil, gy * s + k.py, gx * s + k.px);
          }
      }
      // ---- heavy classes first, ties in enumeration order
      ++order.cases;
      std::vector<Class> sorted = cls;
      cn_sort_heavy_first(sorted.data(), (int)sorted.size());
      std::vector<int> seen(cls.size(), 0);
      for (size_t i = 0; i < sorted.size(); ++i) {
        const Class& k = sorted[i];
        if (k.seq < 0 || k.seq >= (int)cls.size() || seen[k.seq]++ || k.ntaps != cls[k.seq].ntaps)
          order.fail("not a permutation", Ho, Wo, s, (int)i);
        if (i > 0 && (sorted[i - 1].ntaps < k.ntaps || (sorted[i - 1].ntaps == k.ntaps && sorted[i - 1].seq > k.seq)))
          order.fail("order", Ho, Wo, s, (int)i, sorted[i - 1].ntaps, k.ntaps);
      }
    }
    // ---- output sizes. Conv2d: the outputs o >= 0 whose last tap o*s + (k-1)*dil - pad still lies inside the padded input
    // (where the kernel fits at all); ConvTranspose2d: (in-1)*s + k positions written, cropped by pad on both sides, plus
    // out_pad; and Conv2d over a ConvTranspose2d output gives the input size back.
    for (int k = 1; k <= 3; ++k)
      for (int in = 1; in <= 9; ++in) {
        if (in + 2 * pad >= dil * (k - 1) + 1) {
          ++sizes.cases;
          int n = 0;
          for (int o = 0; o < 64; ++o)
            if (o * s + (k - 1) * dil - pad <= in - 1 + pad) ++n;
          if (cn_conv_out(in, k, s, pad, dil) != n) sizes.fail("conv", in, k, s, pad, dil, n);
          if (n != (in + 2 * pad - dil * (k - 1) - 1) / s + 1) sizes.fail("conv closed form", in, k, s, pad, dil, n);
        }
        for (int op = 0; op < s; ++op) {
          ++sizes.cases;
          const int out = cn_convt_out(in, k, s, pad, op);
          if (out != (in - 1) * s + k - 2 * pad + op) sizes.fail("convt", in, k, s, pad, op, out);
          if (out >= 1 && cn_conv_out(out, k, s, pad, 1) != in) sizes.fail("round trip", in, k, s, pad, op, out);
        }
      }
  }

  for (int b = 1; b <= 4; ++b)
    for (int a = -40; a <= 40; ++a) {
      ++fdiv.cases;
      int q = -100;
      while ((q + 1) * b <= a) ++q;  // largest q with q*b <= a
      if (cn_floordiv(a, b) != q) fdiv.fail("floor", a, b, q);
    }

  int bad = 0;
  for (const Check* c : {&cover, &taps, &order, &gather, &sizes, &fdiv}) bad |= c->report();
  return bad;
}
