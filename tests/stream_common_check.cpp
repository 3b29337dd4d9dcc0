// Host check of csrc/stream_common.hpp (built and run by test_stream_common_host.py): the
// magic-number divider is exact for every n < 2^31, its magics fit 32 bits, and stream_chunk is the
// loop it replaced in act.hip / pad.hip / pool.hip.  fdiv is the header's own text: outside hipcc
// its __umulhi is spelled as a 64-bit product.
#include "stream_common.hpp"

#include <cstdarg>
#include <cstdio>
#include <vector>

void e2_set_error(const char*, ...) {}

static long checked = 0, failed = 0;

static void check_div(unsigned d, long long n) {
  if (n < 0 || n > 0x7fffffffLL) return;             // the contract: n < 2^31
  const FastDiv f = mk_div(d);
  const unsigned got = fdiv((unsigned)n, f), want = (unsigned)n / d;
  ++checked;
  if (got != want && ++failed <= 10) printf("fdiv(%lld, %u) = %u, want %u\n", n, d, got, want);
}

static void check_divisor(unsigned d) {
  if (d > 1) {                                       // the magic, recomputed in 64 bits
    unsigned l = 0;
    while ((1ull << l) < d) ++l;
    const unsigned long long m = ((1ull << (31 + l)) + d - 1) / d;
    ++checked;
    if ((m >> 32) != 0 || m != mk_div(d).m) {
      if (++failed <= 10) printf("magic of %u: %llu does not fit 32 bits or is not m = %u\n", d, m, mk_div(d).m);
    }
  }
  const long long D = d, q = 0x7fffffffLL / D;
  const long long ns[] = {0, 1, D - 1, D, D + 1, 0x7ffffffeLL, 0x7fffffffLL};
  for (long long n : ns) check_div(d, n);
  const long long ks[] = {1, 2, 3, q / 2, q - 1, q};
  for (long long k : ks) {
    if (k < 1) continue;
    check_div(d, k * D - 1);
    check_div(d, k * D);
    check_div(d, k * D + 1);
  }
}

// the loop as it stood in act.hip, pad.hip and pool.hip
static unsigned chunk_loop(int num_cu, unsigned long long planes, unsigned long long items,
                           unsigned per_max, unsigned want_per_cu) {
  const unsigned long long want =
      (unsigned long long)want_per_cu * (unsigned long long)(num_cu > 0 ? num_cu : 256);
  unsigned per = per_max;
  while (per > 1 && planes * ((items + 256ull * per - 1) / (256ull * per)) < want) per >>= 1;
  return 256u * per;
}

static void check_chunk(int num_cu, unsigned long long planes, unsigned long long items,
                        unsigned per_max, unsigned want_per_cu, unsigned expect) {
  e2_ctx ctx = e2_ctx{};
  ctx.num_cu = num_cu;
  const unsigned got = stream_chunk(&ctx, planes, items, per_max, want_per_cu);
  const unsigned want = chunk_loop(num_cu, planes, items, per_max, want_per_cu);
  ++checked;
  if (got != want || (expect && got != expect)) {
    ++failed;
    printf("stream_chunk(cu %d, planes %llu, items %llu, %u, %u) = %u, loop %u, expected %u\n", num_cu,
           planes, items, per_max, want_per_cu, got, want, expect);
  }
}

int main() {
  std::vector<unsigned> ds = {1, 2, 3, 5, 7, 10, 23, 90, 185, 0x7fffffffu, 0x80000000u};
  for (int k = 1; k <= 30; ++k) {
    ds.push_back((1u << k) - 1);
    ds.push_back(1u << k);
    ds.push_back((1u << k) + 1);
  }
  for (unsigned d : ds) check_divisor(d);

  // (num_cu, planes, items, per_max, want_per_cu, chunk worked out by hand; 0 = only the loop)
  check_chunk(256, 1, 1, 8, 8, 256);                 // one item: ends at per = 1
  check_chunk(256, 2, 300000, 8, 8, 256);            // 2 * 1172 groups < 2048 even at per = 1
  check_chunk(256, 8, 300000, 8, 8, 1024);           // 8 * 147 < 2048 <= 8 * 293: per = 4
  check_chunk(256, 64, 10000000, 8, 8, 2048);        // 64 * 4883 groups: keeps per_max
  check_chunk(0, 8, 300000, 8, 8, 1024);             // num_cu = 0 behaves as 256
  check_chunk(0, 64, 10000000, 8, 8, 2048);
  check_chunk(304, 20, 23 * 90 * 23, 8, 8, 0);
  check_chunk(1, 1, 5000, 4, 2, 0);
  check_chunk(256, 65535ull * 65535ull, 0x7fffffffull, 8, 8, 2048);

  printf("%ld checks, %ld failed\n", checked, failed);
  return failed ? 1 : 0;
}
