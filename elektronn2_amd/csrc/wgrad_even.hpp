// wgrad_even.hpp -- the even split of a weight-gradient GEMM over G work-groups
// ("MT,NT,9,B,G" / "MT,NT,8,B,G" with B >= 1, conv_pw_wgrad.hip).  The T tiles of dW and the U
// 32-position units of each are ONE sequence of T * U (tile, unit) pairs; work-group g owns a
// contiguous range of them, the ranges differ by at most one pair.  A range that touches several
// tiles is walked as one SEGMENT per tile (units [u0, u0 + n) of `tile`): the kernel zeroes,
// multiplies, sums and flushes once per segment.
// Order of the pairs: B = 1 is tile-major, pair = tile * U + unit.  B > 1 cuts the units into B
// BANDS of `per` units (the last one shorter) and orders band-major, then tile, then unit: the
// work-groups of consecutive ranges then read the SAME positions of the gradient for different
// tiles, which is what keeps its rows in one L2 (DESIGN.md finding 59).
// The kernel and the host (tests, tools) share this one definition; plain C++, no HIP header.
#pragma once

#if defined(__HIPCC__)
#define E2_WG_HD __host__ __device__
#else
#define E2_WG_HD
#endif

struct WgEven {
  int T, U, G;
  int B, per;                                        // bands: units [b * per, min(U, (b + 1) * per))
  int base, extra;                                   // range of g: base pairs, + 1 for g < extra
};
struct WgRange { int b, e; };                        // pairs [b, e)
struct WgSeg { int tile, u0, n; };                   // units [u0, u0 + n) of one tile, n >= 1

// T * U < 2^31 (the caller checks); T, U, G, B >= 1.  Bands are whole rounds of the four waves.
E2_WG_HD inline WgEven wg_even_make(int T, int U, int G, int B) {
  const long total = (long)T * U;
  int per = (U + B - 1) / B;
  per = (per + 3) & ~3;
  return WgEven{T, U, G, (U + per - 1) / per, per, (int)(total / G), (int)(total % G)};
}

E2_WG_HD inline WgRange wg_even_range(const WgEven& ev, int g) {
  const int b = g * ev.base + (g < ev.extra ? g : ev.extra);
  return WgRange{b, b + ev.base + (g < ev.extra ? 1 : 0)};
}

// the segment at the start of a NON-EMPTY range; the next one starts at r.b + n
E2_WG_HD inline WgSeg wg_even_seg(const WgEven& ev, const WgRange& r) {
  const int full = (ev.B - 1) * ev.T * ev.per;       // pairs of the whole bands
  int band, i, len;
  if (r.b < full) { band = r.b / (ev.T * ev.per); i = r.b - band * (ev.T * ev.per); len = ev.per; }
  else { band = ev.B - 1; i = r.b - full; len = ev.U - band * ev.per; }
  const int tile = i / len, off = i - tile * len;
  const int left = r.e - r.b, room = len - off;
  return WgSeg{tile, band * ev.per + off, left < room ? left : room};
}
