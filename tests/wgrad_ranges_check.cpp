// Stand-alone check of csrc/wgrad_even.hpp (built and run by test_wgrad_ranges_host.py with
// -fsanitize=address,undefined): walks (T, U, G) -- tile-major order, B = 1, and a few band counts
// B > 1 -- and asserts, for the ranges and segments the weight-gradient kernel derives from the
// SAME header,
//   - the segments of all work-groups cover every (tile, unit) pair exactly once,
//   - no segment is empty and none leaves its tile (or its band),
//   - a work-group has at most ceil(range / U) + 1 segments (B > 1: U = the shortest band),
//   - range lengths differ by at most one unit,
//   - exactly one segment per tile holds the tile's last unit (the owner of the masked K % 32 step).
#include "wgrad_even.hpp"
#include <cstdio>
#include <vector>

static long cases = 0;

static bool check(int T, int U, int G, int B) {
  ++cases;
  const WgEven ev = wg_even_make(T, U, G, B);
  const int shortest = ev.U - (ev.B - 1) * ev.per;   // (the last band; B = 1: U)
  std::vector<unsigned char> seen((size_t)T * U, 0);
  std::vector<int> owners(T, 0);
  int lo = 1 << 30, hi = 0, end = 0;
#define FAIL(...) do { fprintf(stderr, "T %d U %d G %d B %d: ", T, U, G, B); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); return false; } while (0)
  for (int g = 0; g < G; ++g) {
    WgRange r = wg_even_range(ev, g);
    if (r.b != end) FAIL("range of %d starts at %d, the one before ended at %d", g, r.b, end);
    if (r.e < r.b) FAIL("range of %d is [%d, %d)", g, r.b, r.e);
    end = r.e;
    const int len = r.e - r.b;
    lo = len < lo ? len : lo; hi = len > hi ? len : hi;
    if (len == 0) continue;
    int segs = 0;
    do {
      const WgSeg s = wg_even_seg(ev, r);
      ++segs;
      if (s.n < 1) FAIL("work-group %d: empty segment", g);
      if (s.tile < 0 || s.tile >= T || s.u0 < 0 || s.u0 + s.n > U) FAIL("work-group %d: segment (%d, %d, %d)", g, s.tile, s.u0, s.n);
      for (int u = s.u0; u < s.u0 + s.n; ++u)
        if (seen[(size_t)s.tile * U + u]++) FAIL("pair (%d, %d) twice", s.tile, u);
      if (s.n >= 1 && s.u0 / ev.per != (s.u0 + s.n - 1) / ev.per) FAIL("work-group %d: segment (%d, %d, %d) leaves its band", g, s.tile, s.u0, s.n);
      if (s.u0 + s.n == U) ++owners[s.tile];
      r.b += s.n;
    } while (r.b < r.e);
    if (segs > (len + shortest - 1) / shortest + 1) FAIL("work-group %d: %d segments for %d pairs", g, segs, len);
  }
  if (end != T * U) FAIL("ranges end at %d of %d", end, T * U);
  if (hi - lo > 1) FAIL("range lengths %d .. %d", lo, hi);
  for (size_t i = 0; i < seen.size(); ++i)
    if (seen[i] != 1) FAIL("pair %zu covered %d times", i, (int)seen[i]);
  for (int t = 0; t < T; ++t)
    if (owners[t] != 1) FAIL("tile %d has %d owners of its last unit", t, owners[t]);
#undef FAIL
  return true;
}

int main() {
  for (int T = 1; T <= 12; ++T)
    for (int U = 1; U <= 60; ++U)
      for (int G = 1; G <= 2 * T * U; ++G)
        if (!check(T, U, G, 1)) return 1;
  // bands: fewer shapes, band counts up to more bands than units
  for (int T : {1, 2, 3, 7})
    for (int U : {1, 2, 3, 4, 5, 7, 8, 9, 13, 16, 29, 60})
      for (int B = 2; B <= U + 1 && B <= 9; ++B)
        for (int G = 1; G <= 2 * T * U; ++G)
          if (!check(T, U, G, B)) return 1;
  // the flagship geometries: conv4 (13 x 2 tiles) and conv3 as 13 x 2 of neuro3d_lite at 183
  for (int B = 1; B <= 8; ++B)
    if (!check(57, 460, 256, B) || !check(43, 500, 256, B)) return 1;
  printf("ok %ld\n", cases);
  return 0;
}
