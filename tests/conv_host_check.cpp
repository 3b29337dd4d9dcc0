// Host check of csrc/conv_host.hpp (built and run by tests/test_conv_host.py with the host
// compiler and -fsanitize=address,undefined): the tiling grammar of e2_set_tiling against a table
// written out by hand, the builders of the conv GEMM arguments against literal members, the route
// of a weight-gradient tiling against a table written out by hand and against the if-chain it
// replaced, and the limits of the K-contiguous weight-gradient GEMMs on literal problems.
#include <stdio.h>
#include <string.h>
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

// ---- the route of a weight-gradient tiling --------------------------------------------------
struct RouteRow {
  const char* s;
  bool padded;
  int family, MT, NT, BP;
  bool wave_split, xcd;
  int splits, bands, groups;
  bool refused;
};
static const int L = E2_WG_LDS, D = E2_WG_DIRECT, PW = E2_WG_PW, PK = E2_WG_PW_KS, KS = E2_WG_KS;
static const RouteRow kRoutes[] = {
    // WK 0 / 1 / 4: the LDS-staged kernel, BP 64 / 128; WK 1 with BP 128 / 256 only where dy is not padded
    {"1,1,0,64,2", false, L, 1, 1, 64, false, false, 2, 0, 0, false},
    {"1,1,0,128,2", true, L, 1, 1, 128, false, false, 2, 0, 0, false},     // (0: LDS-staged, forced)
    {"1,1,1,64,2", true, L, 1, 1, 64, false, false, 2, 0, 0, false},
    {"1,1,1,64,2", false, L, 1, 1, 64, false, false, 2, 0, 0, false},
    {"1,1,1,128,2", false, L, 1, 1, 128, false, false, 2, 0, 0, false},
    {"5,4,1,128,0", false, L, 5, 4, 128, false, false, 0, 0, 0, false},
    {"1,1,1,256,2", false, L, 1, 1, 256, false, false, 2, 0, 0, true},
    {"1,1,4,64,2", false, L, 1, 1, 64, true, false, 2, 0, 0, false},
    {"7,1,4,128,1", true, L, 7, 1, 128, true, false, 1, 0, 0, false},
    {"1,2,4,64,1", false, L, 1, 2, 64, false, false, 1, 0, 0, true},
    {"1,2,4,64,1", true, L, 1, 2, 64, false, false, 1, 0, 0, true},
    // WK 1 / 14 / 101 / 114 on the padded gradient, BP 128 / 256: the direct kernel
    {"1,1,1,128,2", true, D, 1, 1, 128, false, false, 2, 0, 0, false},
    {"1,1,1,256,2", true, D, 1, 1, 256, false, false, 2, 0, 0, false},
    {"1,2,14,128,2", true, D, 1, 2, 128, true, false, 2, 0, 0, false},
    {"3,4,14,256,3", true, D, 3, 4, 256, true, false, 3, 0, 0, false},
    {"7,2,101,128,8", true, D, 7, 2, 128, false, true, 8, 0, 0, false},
    {"2,2,101,256,5", true, D, 2, 2, 256, false, true, 5, 0, 0, false},
    {"3,2,114,128,7", true, D, 3, 2, 128, true, true, 7, 0, 0, false},
    {"3,2,114,256,7", true, D, 3, 2, 256, true, true, 7, 0, 0, false},
    // ... and nowhere else
    {"1,2,14,128,2", false, L, 1, 2, 128, false, false, 2, 0, 0, true},
    {"1,1,14,64,2", true, L, 1, 1, 64, false, false, 2, 0, 0, true},
    {"7,2,101,128,8", false, L, 7, 2, 128, false, false, 8, 0, 0, true},
    {"1,1,101,64,2", true, L, 1, 1, 64, false, false, 2, 0, 0, true},
    {"3,2,114,64,7", true, L, 3, 2, 64, false, false, 7, 0, 0, true},
    {"1,1,100,128,2", true, L, 1, 1, 128, false, false, 2, 0, 0, true},
    {"1,1,55,128,1", true, L, 1, 1, 128, false, false, 1, 0, 0, true},
    {"1,1,55,128,1", false, L, 1, 1, 128, false, false, 1, 0, 0, true},
    {"1,1,-1,64,2", false, L, 1, 1, 64, false, false, 2, 0, 0, true},
    {"1,1,1,0,2", true, L, 1, 1, 0, false, false, 2, 0, 0, true},
    // WK 7 / 8 / 9: the K-contiguous GEMMs, whatever the entry point; BP ignored (7) or the bands
    {"2,2,7,0,3", true, PW, 2, 2, 0, false, false, 3, 0, 0, false},
    {"2,2,7,5,3", true, PW, 2, 2, 0, false, false, 3, 0, 0, false},
    {"2,2,7,128,3", false, PW, 2, 2, 0, false, false, 3, 0, 0, false},
    {"13,2,8,0,4", true, PK, 13, 2, 0, false, false, 4, 0, 0, false},
    {"7,2,8,3,16", true, PK, 7, 2, 0, false, false, 16, 3, 16, false},
    {"7,2,8,-3,16", false, PK, 7, 2, 0, false, false, 16, 0, 0, false},
    {"13,2,9,0,4", true, KS, 13, 2, 0, false, false, 4, 0, 0, false},
    {"7,2,9,3,512", true, KS, 7, 2, 0, false, false, 512, 3, 512, false},
    {"7,2,9,128,4", true, KS, 7, 2, 0, false, false, 4, 128, 4, false},
    {"7,2,9,1,0", false, KS, 7, 2, 0, false, false, 0, 1, 0, false},
};

static int same(const E2WgradRoute& r, const RouteRow& w, const char* s, int padded) {
  CHECK(r.family == w.family, "'%s' padded %d: family %d", s, padded, r.family);
  CHECK(r.MT == w.MT && r.NT == w.NT, "'%s' padded %d: tile %d x %d", s, padded, r.MT, r.NT);
  CHECK(r.BP == w.BP, "'%s' padded %d: BP %d", s, padded, r.BP);
  CHECK(r.wave_split == w.wave_split, "'%s' padded %d: wave_split %d", s, padded, (int)r.wave_split);
  CHECK(r.xcd == w.xcd, "'%s' padded %d: xcd %d", s, padded, (int)r.xcd);
  CHECK(r.splits == w.splits, "'%s' padded %d: splits %d", s, padded, r.splits);
  CHECK(r.bands == w.bands && r.groups == w.groups, "'%s' padded %d: bands %d groups %d", s, padded, r.bands, r.groups);
  CHECK((r.refuse != nullptr) == w.refused, "'%s' padded %d: refused %d", s, padded, (int)(r.refuse != nullptr));
  return 0;
}

// The if-chain e2i_wgrad_conv had before the route (commit 6dbc609), kept here as the oracle: the
// same conditions in the same order, the launcher calls and E2_REQUIREs replaced by a record of
// which was reached with what.  `even` / S of the forms 8 and 9 read as their launchers read them
// (even > 0: `even` bands, S work-groups).
struct WCfg { int MT, NT, WK, BP, PS; };
static RouteRow old_chain(WCfg c, bool dy_padded, bool mfma_bf16, const char** fam_out) {
  {
    const bool direct = dy_padded && (c.WK == 1 || c.WK == 14 || c.WK == 101 || c.WK == 114) &&
                        (c.BP == 128 || c.BP == 256);
    const char* fam = c.WK == 7 ? "pw_wgrad" : c.WK == 8 ? "pw_wgrad_ks" : c.WK == 9 ? "wgrad_ks"
                      : direct ? (mfma_bf16 ? "wgrad_direct_bf16r" : "wgrad_direct")
                      : "wgrad_lds";
    *fam_out = fam;
  }
  auto pw = [](int MT, int NT, int S) { return RouteRow{"", false, PW, MT, NT, 0, false, false, S, 0, 0, false}; };
  auto ks = [](int fam, int MT, int NT, int S, int even) {
    return RouteRow{"", false, fam, MT, NT, 0, false, false, S, even > 0 ? even : 0, even > 0 ? S : 0, false};
  };
  auto direct = [](int MT, int NT, int BP, int PS, int WK, int xcd) {
    return RouteRow{"", false, D, MT, NT, BP, WK == 4, xcd != 0, PS, 0, 0, false};
  };
  auto refused = [&]() { return RouteRow{"", false, L, c.MT, c.NT, c.BP, false, false, c.PS, 0, 0, true}; };
  if (c.WK == 7) return pw(c.MT, c.NT, c.PS);
  if (c.WK == 8) return ks(PK, c.MT, c.NT, c.PS, c.BP);
  if (c.WK == 9) return ks(KS, c.MT, c.NT, c.PS, c.BP);
  if (dy_padded && (c.WK == 1 || c.WK == 14 || c.WK == 101 || c.WK == 114) && (c.BP == 128 || c.BP == 256))
    return direct(c.MT, c.NT, c.BP, c.PS, (c.WK % 100) == 14 ? 4 : 1, c.WK >= 100);
  if (!(c.WK != 14 && c.WK < 100)) return refused();
  if (c.WK == 0) c.WK = 1;
  if (!(c.BP == 64 || c.BP == 128)) return refused();
  if (!(c.WK == 1 || (c.WK == 4 && c.NT == 1))) return refused();
  return RouteRow{"", false, L, c.MT, c.NT, c.BP, c.WK == 4, false, c.PS, 0, 0, false};
}

static int check_routes() {
  for (const RouteRow& w : kRoutes) {
    E2Tiling t;
    CHECK(e2_parse_tiling(w.s, &t) && e2_wgrad_candidate(t), "'%s': five integers", w.s);
    const E2WgradRoute r = e2_wgrad_route(t.v, w.padded);
    if (same(r, w, w.s, w.padded)) return 1;
    // the table itself, for the Python side (test_conv_host.py compares tiling.wgrad_route with it)
    printf("route\t%s\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n", w.s, (int)w.padded,
           e2_wgrad_family_name(r, false), e2_wgrad_family_name(r, true), w.MT, w.NT, w.BP,
           (int)w.wave_split, (int)w.xcd, w.splits, w.bands, w.groups, (int)w.refused);
  }
  // the names e2_last_launch has for the families
  {
    E2WgradRoute r;
    const char* f32[] = {"wgrad_lds", "wgrad_direct", "pw_wgrad", "pw_wgrad_ks", "wgrad_ks"};
    const int fam[] = {L, D, PW, PK, KS};
    for (int i = 0; i < 5; ++i) {
      r.family = fam[i];
      CHECK(!strcmp(e2_wgrad_family_name(r, false), f32[i]), "name of family %d", fam[i]);
      CHECK(!strcmp(e2_wgrad_family_name(r, true), fam[i] == D ? "wgrad_direct_bf16r" : f32[i]), "bf16 name of family %d", fam[i]);
    }
  }
  // ... and the whole grid against the chain the route replaced
  int cells = 0, differences = 0;
  std::vector<int> WKs;
  for (int w = -1; w <= 15; ++w) WKs.push_back(w);
  for (int w = 99; w <= 115; ++w) WKs.push_back(w);
  for (int MT : {1, 7}) for (int NT : {1, 2, 4}) for (int WK : WKs)
    for (int BP : {0, 1, 3, 64, 128, 256, 512}) for (int PS : {0, 1, 8}) for (int padded = 0; padded < 2; ++padded)
      for (int bf = 0; bf < 2; ++bf) {
        const int v[5] = {MT, NT, WK, BP, PS};
        const char* fam = nullptr;
        const RouteRow w = old_chain(WCfg{MT, NT, WK, BP, PS}, padded != 0, bf != 0, &fam);
        const E2WgradRoute r = e2_wgrad_route(v, padded != 0);
        char s[64];
        snprintf(s, sizeof s, "%d,%d,%d,%d,%d", MT, NT, WK, BP, PS);
        ++cells;
        if (strcmp(fam, e2_wgrad_family_name(r, bf != 0))) { ++differences; printf("FAILED '%s' padded %d: name %s\n", s, padded, fam); }
        if (same(r, w, s, padded)) ++differences;
      }
  CHECK(cells == 2 * 3 * 34 * 7 * 3 * 2 * 2 && differences == 0, "%d differences in %d cells", differences, cells);
  printf("grid\t%d\t%d\n", cells, differences);
  return 0;
}

// ---- the limits of the K-contiguous weight-gradient GEMMs ---------------------------------------
static bool says(const char* msg, const char* word) { return msg && strstr(msg, word); }

static int check_limits() {
  static float X[16], Y[16], DW[16];
  // a dense 1x1x1 problem: (2, 5, 3, 7, 9) -> 6 channels
  const e2_tensor5 xd = e2_dense_view(X, 2, 5, 3, 7, 9), yd = e2_dense_view(Y, 2, 6, 3, 7, 9);
  const WgradArgs pw = wgrad_args(xd, yd, DW, 1, 1, 1, 0, 1);
  CHECK(e2_pw_wgrad_limit(pw, false, 0) == nullptr && e2_pw_wgrad_limit(pw, false, 128) == nullptr, "dense 1x1x1");
  CHECK(says(e2_pw_wgrad_limit(pw, true, 0), "bf16"), "1x1x1, bf16 mode");
  CHECK(says(e2_wgrad_ks_limit(pw, false, 128), "taps"), "1x1x1 is no kernel with taps");
  {
    WgradArgs a = pw;
    a.upR = 8;                                       // UpConv rows: the launcher's Cout % R, no limit here
    CHECK(e2_pw_wgrad_limit(a, false, 0) == nullptr, "1x1x1, upR = 8");
    a = pw; a.kw = 3;
    CHECK(says(e2_pw_wgrad_limit(a, false, 0), "1x1x1"), "taps");
    a = pw; a.xsZ = (7 + 3) * 9;                     // a crop that keeps the rows but not the planes
    CHECK(says(e2_pw_wgrad_limit(a, false, 0), "dense channel planes"), "x planes not dense");
    a = pw; a.xsY = 11; a.xsZ = 7 * 11;              // ... and one that keeps neither
    CHECK(says(e2_pw_wgrad_limit(a, false, 0), "dense channel planes"), "x rows not dense");
    a = pw; a.dsZ = 7 * 9 + 1;
    CHECK(says(e2_pw_wgrad_limit(a, false, 0), "dense channel planes"), "dy planes not dense");
    a = pw; a.dsY = 10;
    CHECK(says(e2_pw_wgrad_limit(a, false, 0), "dense channel planes"), "dy rows not dense");
  }
  // a kernel with taps: x (1, 2, 2, 10, 32), kernel (1, 3, 3) -> dy (1, 4, 2, 8, 30) inside its
  // padded buffer (1, 4, 2, 12, 32 + 2) at the input's row pitch 32
  const e2_tensor5 xk = e2_dense_view(X, 1, 2, 2, 10, 32);
  const e2_tensor5 yk{Y, 1, 4, 2, 8, 30, 4 * 2 * 384, 2 * 384, 384, 32};
  const WgradArgs ks = wgrad_args(xk, yk, DW, 1, 3, 3, 0, 1);
  CHECK(e2_wgrad_ks_limit(ks, false, 128) == nullptr && e2_wgrad_ks_limit(ks, false, 4096) == nullptr, "taps, padded, slack");
  CHECK(says(e2_wgrad_ks_limit(ks, false, 0), "e2_set_input_slack"), "slack 0");
  CHECK(says(e2_wgrad_ks_limit(ks, false, 127), "e2_set_input_slack"), "slack 127");
  CHECK(says(e2_wgrad_ks_limit(ks, true, 128), "bf16"), "taps, bf16 mode");
  CHECK(says(e2_pw_wgrad_limit(ks, false, 128), "1x1x1"), "taps are no 1x1x1 kernel");
  {
    WgradArgs a = ks;
    a.dy_padded = 0;
    CHECK(says(e2_wgrad_ks_limit(a, false, 128), "zero-padded"), "dy not padded");
    a = ks; a.upR = 8;
    CHECK(says(e2_wgrad_ks_limit(a, false, 128), "taps"), "upR = 8");
    a = ks; a.dsY = 34;                              // the gradient's own dense pitch
    CHECK(says(e2_wgrad_ks_limit(a, false, 128), "pitch"), "row pitch of dy and x differ");
    a = ks; a.xsZ = 10 * 32 - 1;                     // planes overlap by one float
    CHECK(says(e2_wgrad_ks_limit(a, false, 128), "overlap"), "overlapping planes");
    a = ks; a.xsC = 2 * 320 - 1;                     // ... channels
    CHECK(says(e2_wgrad_ks_limit(a, false, 128), "overlap"), "overlapping channels");
    a = ks; a.dsC = -1;
    CHECK(says(e2_wgrad_ks_limit(a, false, 128), "32-bit"), "negative channel stride");
    // (kh - 1) * pitch + kw - 1 zeros behind a plane: kernel (1, 2, 2), pitch 29 -> 30, pitch 30 -> 31
    for (int pitch = 29; pitch <= 30; ++pitch) {
      const e2_tensor5 x2 = e2_dense_view(X, 1, 2, 2, 9, pitch);
      const e2_tensor5 y2{Y, 1, 4, 2, 8, pitch - 1, 4 * 2 * 10 * pitch, 2 * 10 * pitch, 10 * pitch, pitch};
      const WgradArgs b = wgrad_args(x2, y2, DW, 1, 2, 2, 0, 1);
      CHECK((b.kh - 1) * b.xsY + b.kw - 1 == pitch + 1, "zeros");
      if (pitch == 29) CHECK(says(e2_wgrad_ks_limit(b, false, 128), "31 zeros"), "30 zeros behind a plane");
      else CHECK(e2_wgrad_ks_limit(b, false, 128) == nullptr, "31 zeros behind a plane");
    }
    // 32-bit byte offsets inside a sample: (Cout * dsC + Do * dsZ + K) * 4 + 256 just under / at 2^32
    const int64_t K = 7 * 32 + 30, rest = 2 * 384 + K;
    a = ks; a.Cout = 1; a.dsC = ((int64_t)1 << 30) - 64 - 1 - rest;
    CHECK((a.dsC + rest) * 4 + 256 == ((int64_t)1 << 32) - 4, "just under");
    CHECK(e2_wgrad_ks_limit(a, false, 128) == nullptr, "gradient sample just under the 32-bit limit");
    a.dsC += 1;
    CHECK(says(e2_wgrad_ks_limit(a, false, 128), "32-bit"), "gradient sample at the 32-bit limit");
    // ... and of x: (Cin * xsC + Din * xsZ) * 4 + 256
    a = ks; a.Cin = 1; a.xsC = ((int64_t)1 << 30) - 64 - 1 - 2 * 320;
    CHECK(e2_wgrad_ks_limit(a, false, 128) == nullptr, "input sample just under the 32-bit limit");
    a.xsC += 1;
    CHECK(says(e2_wgrad_ks_limit(a, false, 128), "32-bit"), "input sample at the 32-bit limit");
  }
  return 0;
}

int main() {
  if (check_grammar()) return 1;
  if (check_builders()) return 1;
  if (check_routes()) return 1;
  if (check_limits()) return 1;
  printf("ok %d\n", g_checks);
  return 0;
}
