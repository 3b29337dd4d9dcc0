// Host check of csrc/conv_host.hpp (built and run by tests/test_conv_host.py with the host
// compiler and -fsanitize=address,undefined): the tiling grammar of e2_set_tiling against a table
// written out by hand, and the builders of the conv GEMM arguments against literal members.
#include <stdio.h>
#include <string>
#include <vector>
#include "conv_host.hpp"

static int g_checks = 0;
#define CHECK(cond, ...)                                             \
  do {                                                               \
    ++g_checks;                                                      \
    if (!(cond)) {                                                   \
      printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond);       \
      printf(__VA_ARGS__);                                           \
      printf("\n");                                                  \
      return 1;                                                      \
    }                                                                \
  } while (0)

// ---- the grammar ----------------------------------------------------------------------------
// form: what a packed f32 launch makes of the list (E2_FORM_*); cb / cand / wb: the predicates of
// conv_bf16, choose_wcfg and wgrad_bf16.  A malformed string has n = 0 and nothing holds.
struct Row {
  std::string s;
  bool well_formed;
  int n;
  int v[8];
  bool igemm_ok, wgrad_ok;      // e2_set_tiling accepts it for the kind
  int form;
  bool cb, cand, wb;
};
static const int NONE = E2_FORM_NONE;
static const std::string Z55(55, '0');

static const std::vector<Row> kRows = {
    // the forms of tiling.py's docstring: kind 'igemm' ...
    {"7,2,32,1", true, 4, {7, 2, 32, 1}, true, false, E2_FORM_16x16x4, false, false, false},
    {"4,5,1,8,1,3,4,1", true, 8, {4, 5, 1, 8, 1, 3, 4, 1}, true, false, E2_FORM_4x4x1, false, false, false},
    {"1,13,1", true, 3, {1, 13, 1}, true, false, E2_FORM_POINTWISE, false, false, false},
    {"1,13,1,64,0", true, 5, {1, 13, 1, 64, 0}, true, true, E2_FORM_POINTWISE, false, true, false},
    {"32,1,2", true, 3, {32, 1, 2}, true, false, NONE, true, false, false},
    // ... and kind 'wgrad' (a five-integer list is also acceptable to the 'igemm' kind)
    {"32,2,3,1,4", true, 5, {32, 2, 3, 1, 4}, true, true, NONE, true, true, true},
    {"7,2,101,128,8", true, 5, {7, 2, 101, 128, 8}, true, true, NONE, false, true, false},
    {"13,2,9,0,4", true, 5, {13, 2, 9, 0, 4}, true, true, NONE, false, true, false},
    // the empty string clears the setting
    {"", true, 0, {}, true, true, NONE, false, false, false},
    {"1,2,2,64,0", true, 5, {1, 2, 2, 64, 0}, true, true, E2_FORM_POINTWISE, false, true, false},
    // five integers not starting with 1: set_tiling takes it, no packed launch runs it
    {"3,4,5,6,7", true, 5, {3, 4, 5, 6, 7}, true, true, NONE, false, true, false},
    // four integers starting with 32: a 16x16x4 tiling with MT = 32 to a packed launch AND the tile
    // (2, 2) to conv_bf16
    {"32,2,2,1", true, 4, {32, 2, 2, 1}, true, false, E2_FORM_16x16x4, true, false, false},
    {"32,2,2", true, 3, {32, 2, 2}, true, false, NONE, true, false, false},          // no WGRAD string
    {"7,2,9", true, 3, {7, 2, 9}, false, false, NONE, false, false, false},
    {"4,5,1,8,1,3,4", true, 7, {4, 5, 1, 8, 1, 3, 4}, false, false, NONE, false, false, false},
    {"5,5,1,8,1,3,4,1", true, 8, {5, 5, 1, 8, 1, 3, 4, 1}, false, false, NONE, false, false, false},
    {"7", true, 1, {7}, false, false, NONE, false, false, false},
    {"7,2", true, 2, {7, 2}, false, false, NONE, false, false, false},
    {"1,2,3,4,5,6", true, 6, {1, 2, 3, 4, 5, 6}, false, false, NONE, false, false, false},
    {"1,2,3,4,5,6,7,8,9", false, 0, {}, false, false, NONE, false, false, false},
    {"4,1,2,3,", false, 0, {}, false, false, NONE, false, false, false},
    {"4,1,2,x", false, 0, {}, false, false, NONE, false, false, false},
    {" 4,1,2,3", false, 0, {}, false, false, NONE, false, false, false},
    {"4, 1,2,3", false, 0, {}, false, false, NONE, false, false, false},
    {"4,1,2,3 ", false, 0, {}, false, false, NONE, false, false, false},
    {"+4,1,2,3", false, 0, {}, false, false, NONE, false, false, false},
    {"4,,1,2", false, 0, {}, false, false, NONE, false, false, false},
    {",", false, 0, {}, false, false, NONE, false, false, false},
    {"-", false, 0, {}, false, false, NONE, false, false, false},
    {"4,1,2,3x", false, 0, {}, false, false, NONE, false, false, false},
    {"1.5,2,3,4", false, 0, {}, false, false, NONE, false, false, false},
    {"--1,2,3,4", false, 0, {}, false, false, NONE, false, false, false},
    // negative numbers are integers: the launch refuses what it cannot run
    {"-1,2,3,4", true, 4, {-1, 2, 3, 4}, true, false, E2_FORM_16x16x4, false, false, false},
    {"7,-2,32,-1", true, 4, {7, -2, 32, -1}, true, false, E2_FORM_16x16x4, false, false, false},
    {"-32,1,2", true, 3, {-32, 1, 2}, false, false, NONE, false, false, false},
    {"2147483647,1,1,1", true, 4, {2147483647, 1, 1, 1}, true, false, E2_FORM_16x16x4, false, false, false},
    {"2147483648,1,1,1", false, 0, {}, false, false, NONE, false, false, false},
    // 63 characters fit the context's buffer, 64 do not
    {"7,2,32," + Z55 + "1", true, 4, {7, 2, 32, 1}, true, false, E2_FORM_16x16x4, false, false, false},
    {"7,2,32,0" + Z55 + "1", false, 0, {}, false, false, NONE, false, false, false},
};

static int check_grammar() {
  CHECK(kRows[kRows.size() - 2].s.size() == 63 && kRows.back().s.size() == 64, "lengths");
  for (const Row& r : kRows) {
    const char* s = r.s.c_str();
    E2Tiling t;
    t.n = 77;
    const bool wf = e2_parse_tiling(s, &t);
    CHECK(wf == r.well_formed, "'%s': well formed %d", s, (int)wf);
    CHECK(t.n == r.n, "'%s': n = %d", s, t.n);
    for (int i = 0; i < 8; ++i) CHECK(t.v[i] == r.v[i], "'%s': v[%d] = %d", s, i, t.v[i]);
    CHECK((wf && e2_tiling_accepted(E2_TILING_IGEMM, t)) == r.igemm_ok, "'%s' as IGEMM", s);
    CHECK((wf && e2_tiling_accepted(E2_TILING_WGRAD, t)) == r.wgrad_ok, "'%s' as WGRAD", s);
    CHECK(e2_packed_form(t) == r.form, "'%s': packed form %d", s, e2_packed_form(t));
    CHECK(e2_conv_bf16_forced(t) == r.cb, "'%s': conv_bf16", s);
    CHECK(e2_wgrad_candidate(t) == r.cand, "'%s': choose_wcfg", s);
    CHECK(e2_wgrad_bf16_forced(t) == r.wb, "'%s': wgrad_bf16", s);
    // forced / fallback / model of the two launchers with operands in memory
    CHECK(e2_memory_src(r.cb, t) == (r.cb ? E2_SRC_FORCED : (r.n ? E2_SRC_FALLBACK : E2_SRC_MODEL)), "'%s': src", s);
    CHECK(e2_memory_src(r.wb, t) == (r.wb ? E2_SRC_FORCED : (r.n ? E2_SRC_FALLBACK : E2_SRC_MODEL)), "'%s': src", s);
    // the table itself, for the Python side (test_conv_host.py compares tiling.parse with it)
    printf("row\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n", s, (int)r.well_formed, r.n, (int)r.igemm_ok,
           (int)r.wgrad_ok, r.form, (int)r.cb, (int)r.cand, (int)r.wb);
  }
  return 0;
}

// ---- the builders ---------------------------------------------------------------------------
#define IG_MEMBERS(X)                                                                             \
  X(in) X(wp) X(out) X(N) X(Cin) X(Cout) X(kd) X(kh) X(kw) X(Do) X(Ho) X(Wo) X(isN) X(isC) X(isZ) \
  X(isY) X(osN) X(osC) X(osZ) X(osY) X(ciP) X(coP) X(upz) X(upy) X(upx) X(bias) X(act) X(up_bias) \
  X(up_act) X(up_bias_done) X(gm) X(gm_src) X(gsN) X(gsC) X(gsZ) X(gm_dbias) X(gm_bias)           \
  X(gm_done) X(fill_base) X(fill_n) X(zpad) X(parts_max) X(part_stride) X(nparts)
#define WG_MEMBERS(X)                                                                             \
  X(x) X(dy) X(dw) X(N) X(Cin) X(Cout) X(kd) X(kh) X(kw) X(Do) X(Ho) X(Wo) X(xsN) X(xsC) X(xsZ)   \
  X(xsY) X(dsN) X(dsC) X(dsZ) X(dsY) X(flip) X(upR) X(accumulate) X(dy_padded)

static int same(const IgemmArgs& a, const IgemmArgs& b, const char* what) {
#define X(m) CHECK(a.m == b.m, "%s: IgemmArgs.%s", what, #m);
  IG_MEMBERS(X)
#undef X
  return 0;
}
static int same(const WgradArgs& a, const WgradArgs& b, const char* what) {
#define X(m) CHECK(a.m == b.m, "%s: WgradArgs.%s", what, #m);
  WG_MEMBERS(X)
#undef X
  return 0;
}

static int check_builders() {
  // the documented defaults: nothing set, UpConv scatter / rows off
  {
    IgemmArgs d, e{};
    e.in = nullptr; e.wp = nullptr; e.out = nullptr;
    e.N = e.Cin = e.Cout = e.kd = e.kh = e.kw = e.Do = e.Ho = e.Wo = 0;
    e.isN = e.isC = e.isZ = e.isY = e.osN = e.osC = e.osZ = e.osY = 0;
    e.ciP = e.coP = 0; e.upz = e.upy = e.upx = 1;
    e.bias = nullptr; e.act = 0; e.up_bias = nullptr; e.up_act = 0; e.up_bias_done = nullptr;
    e.gm = 0; e.gm_src = nullptr; e.gsN = e.gsC = e.gsZ = 0; e.gm_dbias = nullptr; e.gm_bias = nullptr;
    e.gm_done = nullptr; e.fill_base = nullptr; e.fill_n = 0; e.zpad = 0; e.parts_max = 0;
    e.part_stride = 0; e.nparts = nullptr;
    if (same(d, e, "default")) return 1;
    WgradArgs g, h{};
    h.x = nullptr; h.dy = nullptr; h.dw = nullptr;
    h.N = h.Cin = h.Cout = h.kd = h.kh = h.kw = h.Do = h.Ho = h.Wo = 0;
    h.xsN = h.xsC = h.xsZ = h.xsY = h.dsN = h.dsC = h.dsZ = h.dsY = 0;
    h.flip = 0; h.upR = 1; h.accumulate = 0; h.dy_padded = 0;
    if (same(g, h, "default")) return 1;
  }

  static float X[4096], Y[4096], W[64], DW[64];
  const float* wp = W;
  // forward, dense views: x (2, 3, 4, 5, 6), kernel 2 x 3 x 3, 7 output channels -> y (2, 7, 3, 3, 4)
  const e2_tensor5 xd{X, 2, 3, 4, 5, 6, 360, 120, 30, 6}, yd{Y, 2, 7, 3, 3, 4, 252, 36, 12, 4};
  // the same extents as strided views: row pitch > w, n stride not c * d * h * w, offset pointers
  const e2_tensor5 xs{X + 11, 2, 3, 4, 5, 6, 1000, 300, 60, 9}, ys{Y + 5, 2, 7, 3, 3, 4, 900, 100, 30, 7};
  {
    IgemmArgs e;
    e.in = X; e.wp = W; e.out = Y; e.N = 2; e.Cin = 3; e.Cout = 7; e.kd = 2; e.kh = 3; e.kw = 3;
    e.Do = 3; e.Ho = 3; e.Wo = 4; e.isN = 360; e.isC = 120; e.isZ = 30; e.isY = 6;
    e.osN = 252; e.osC = 36; e.osZ = 12; e.osY = 4;
    if (same(igemm_args(xd, yd, wp, 7, 2, 3, 3), e, "forward, dense")) return 1;
    e.in = X + 11; e.out = Y + 5; e.isN = 1000; e.isC = 300; e.isZ = 60; e.isY = 9;
    e.osN = 900; e.osC = 100; e.osZ = 30; e.osY = 7;
    if (same(igemm_args(xs, ys, wp, 7, 2, 3, 3), e, "forward, strided")) return 1;
  }
  // data gradient: the padded dy (2, 7, 5, 7, 8) is the input, dx (2, 3, 4, 5, 6) the output
  const e2_tensor5 pd{Y, 2, 7, 5, 7, 8, 1960, 280, 56, 8}, ps{Y + 3, 2, 7, 5, 7, 8, 2100, 290, 57, 8};
  {
    IgemmArgs e;
    e.in = Y; e.wp = W; e.out = X; e.N = 2; e.Cin = 7; e.Cout = 3; e.kd = 2; e.kh = 3; e.kw = 3;
    e.Do = 4; e.Ho = 5; e.Wo = 6; e.isN = 1960; e.isC = 280; e.isZ = 56; e.isY = 8;
    e.osN = 360; e.osC = 120; e.osZ = 30; e.osY = 6;
    if (same(igemm_args(pd, xd, wp, 3, 2, 3, 3), e, "dgrad, dense")) return 1;
    e.in = Y + 3; e.out = X + 11; e.isN = 2100; e.isC = 290; e.isZ = 57; e.isY = 8;
    e.osN = 1000; e.osC = 300; e.osZ = 60; e.osY = 9;
    if (same(igemm_args(ps, xs, wp, 3, 2, 3, 3), e, "dgrad, strided")) return 1;
  }
  // weight gradient from the padded buffer: the interior starts (kd-1, kh-1, kw-1) = (1, 2, 2) in
  {
    WgradArgs e;
    e.x = X; e.dy = Y + 1 * 56 + 2 * 8 + 2; e.dw = DW; e.N = 2; e.Cin = 3; e.Cout = 7;
    e.kd = 2; e.kh = 3; e.kw = 3; e.Do = 3; e.Ho = 3; e.Wo = 4;
    e.xsN = 360; e.xsC = 120; e.xsZ = 30; e.xsY = 6; e.dsN = 1960; e.dsC = 280; e.dsZ = 56; e.dsY = 8;
    e.flip = 1; e.upR = 1; e.accumulate = 1; e.dy_padded = 1;
    if (same(wgrad_args(xd, e2_interior(pd, 1, 2, 2), DW, 2, 3, 3, 1, 1), e, "wgrad_pad, dense")) return 1;
    e.x = X + 11; e.dy = Y + 3 + 1 * 57 + 2 * 8 + 2; e.accumulate = 0;
    e.xsN = 1000; e.xsC = 300; e.xsZ = 60; e.xsY = 9; e.dsN = 2100; e.dsC = 290; e.dsZ = 57; e.dsY = 8;
    if (same(wgrad_args(xs, e2_interior(ps, 1, 2, 2), DW, 2, 3, 3, 0, 1), e, "wgrad_pad, strided")) return 1;
    // the plain entry point: the unpadded view as it is
    e.dy = Y + 5; e.dsN = 900; e.dsC = 100; e.dsZ = 30; e.dsY = 7; e.dy_padded = 0;
    if (same(wgrad_args(xs, ys, DW, 2, 3, 3, 0, 0), e, "wgrad, strided")) return 1;
  }
  // UpConv by (1, 2, 2), R = 4: x (2, 3, 4, 5, 6) -> y (2, 5, 4, 10, 12); the space-to-depth image
  // of the backward is dense (2, 5 * 4, 4, 5, 6)
  {
    const e2_tensor5 s2d = e2_dense_view(Y, 2, 20, 4, 5, 6);
    CHECK(s2d.ptr == Y && s2d.n == 2 && s2d.c == 20 && s2d.d == 4 && s2d.h == 5 && s2d.w == 6 &&
              s2d.sn == 2400 && s2d.sc == 120 && s2d.sd == 30 && s2d.sh == 6, "dense view");
    IgemmArgs e;                                     // data gradient: s2d -> dx, a strided view
    e.in = Y; e.wp = W; e.out = X + 11; e.N = 2; e.Cin = 20; e.Cout = 3; e.kd = e.kh = e.kw = 1;
    e.Do = 4; e.Ho = 5; e.Wo = 6; e.isN = 2400; e.isC = 120; e.isZ = 30; e.isY = 6;
    e.osN = 1000; e.osC = 300; e.osZ = 60; e.osY = 9;
    if (same(igemm_args(s2d, xs, wp, 3, 1, 1, 1), e, "upconv dgrad")) return 1;
    WgradArgs g = wgrad_args(xs, s2d, DW, 1, 1, 1, 1, 1), h;
    g.flip = 0; g.upR = 4;                           // (the call site's)
    h.x = X + 11; h.dy = Y; h.dw = DW; h.N = 2; h.Cin = 3; h.Cout = 20; h.kd = h.kh = h.kw = 1;
    h.Do = 4; h.Ho = 5; h.Wo = 6; h.xsN = 1000; h.xsC = 300; h.xsZ = 60; h.xsY = 9;
    h.dsN = 2400; h.dsC = 120; h.dsZ = 30; h.dsY = 6; h.flip = 0; h.upR = 4; h.accumulate = 1; h.dy_padded = 1;
    if (same(g, h, "upconv wgrad")) return 1;
  }
  return 0;
}

int main() {
  if (check_grammar()) return 1;
  if (check_builders()) return 1;
  printf("ok %d\n", g_checks);
  return 0;
}
