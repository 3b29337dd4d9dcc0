// conv_host.hpp -- host-only part of the conv launches: the tiling grammar behind e2_set_tiling
// and the argument structs of the conv GEMM launchers with their builders.  Includes no HIP
// header, so that a host compiler builds it alone (tests/conv_host_check.cpp).
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/e2hip.h"

// ---- tiling strings -----------------------------------------------------------------------
// A tiling string is a comma-separated list of at most 8 integers (an optional '-' and decimal
// digits each, within 32 bits), nothing else -- no blanks, no '+', no trailing comma -- of at
// most 63 characters.  "" is the empty list.  (The same words: e2hip.h, tiling.py.)
constexpr int kE2TilingChars = 64;     // a string and its terminator
struct E2Tiling {
  int n = 0;          // integers in the string (0: none set, the cost model chooses)
  int v[8] = {};
};

// the one parser (e2_set_tiling); false: not such a list, *out is then the empty list
static inline bool e2_parse_tiling(const char* s, E2Tiling* out) {
  E2Tiling t;
  *out = t;
  if (!s[0]) return true;
  if (strlen(s) >= (size_t)kE2TilingChars) return false;
  for (;;) {
    if (t.n == 8) return false;
    const bool neg = *s == '-';
    if (neg) ++s;
    if (*s < '0' || *s > '9') return false;
    int64_t x = 0;
    for (; *s >= '0' && *s <= '9'; ++s) {
      x = x * 10 + (*s - '0');
      if (x > INT32_MAX) return false;
    }
    t.v[t.n++] = (int)(neg ? -x : x);
    if (!*s) break;
    if (*s++ != ',') return false;
  }
  *out = t;
  return true;
}

// what e2_set_tiling accepts per kind (the empty list always)
static inline bool e2_tiling_accepted(int kind, const E2Tiling& t) {
  if (t.n == 0) return true;
  if (kind == E2_TILING_WGRAD) return t.n == 5;
  return t.n == 4 || t.n == 5 || (t.n == 3 && (t.v[0] == 1 || t.v[0] == 32)) || (t.n == 8 && t.v[0] == 4);
}

// what each launch site reads out of the parsed list
enum { E2_FORM_NONE = -1, E2_FORM_16x16x4 = 0, E2_FORM_POINTWISE = 1, E2_FORM_4x4x1 = 4 };
static inline int e2_packed_form(const E2Tiling& t) {           // packed f32 launches (choose_cfg)
  if (t.n == 4) return E2_FORM_16x16x4;
  if ((t.n == 3 || t.n == 5) && t.v[0] == 1) return E2_FORM_POINTWISE;
  if (t.n == 8 && t.v[0] == 4) return E2_FORM_4x4x1;
  return E2_FORM_NONE;
}
static inline bool e2_conv_bf16_forced(const E2Tiling& t) { return t.n >= 3 && t.v[0] == 32; }
static inline bool e2_wgrad_candidate(const E2Tiling& t) { return t.n == 5; }    // choose_wcfg
static inline bool e2_wgrad_bf16_forced(const E2Tiling& t) { return t.n == 5 && t.v[0] == 32; }

// what decided the tiling of a launch (third word of e2_last_launch)
enum { E2_SRC_MODEL = 0, E2_SRC_FORCED = 1, E2_SRC_FALLBACK = 2 };
// the launchers with bf16 operands in memory: their form of the string was honoured; a string of
// another form was set and the default tile ran instead; none was set
static inline int e2_memory_src(bool forced, const E2Tiling& t) {
  return forced ? E2_SRC_FORCED : (t.n ? E2_SRC_FALLBACK : E2_SRC_MODEL);
}

// ---- conv GEMM arguments ------------------------------------------------------------------
// Generic strided "valid" correlation as implicit GEMM on fp32 MFMA.
//   out[n][oc][z][y][x] (+)= sum_ic sum_t Wp[dz][t][ic][oc] * in[n][ic][z+dz][y+ty][x+tx]
// Wp is the PACKED weight image produced by e2i_pack_weights (flip folded in).
struct IgemmArgs {
  const float* in = nullptr;
  const float* wp = nullptr;
  float* out = nullptr;
  int N = 0, Cin = 0, Cout = 0;
  int kd = 0, kh = 0, kw = 0;
  int Do = 0, Ho = 0, Wo = 0;          // output spatial
  int64_t isN = 0, isC = 0, isZ = 0, isY = 0;
  int64_t osN = 0, osC = 0, osZ = 0, osY = 0;
  int ciP = 0, coP = 0;            // padded channel counts of the packed image
  // upconv scatter mode: out channel oc' = co*R + r, stored at
  // out[n][co][pz*z+rz][py*y+ry][px*x+rx]; R = pz*py*px (1 = off)
  int upz = 1, upy = 1, upx = 1;
  // fused epilogue (conv forward of a layer that does not pool): out = act(conv + bias[oc]);
  // relu writes -0.0 where the pre-activation was NEGATIVE and +0.0 where it was exactly
  // zero, so that the backward can tell relu'(0) = 0.5 from 0 without the pre-activation
  const float* bias = nullptr;
  int act = 0;
  // UpConv (upz * upy * upx > 1): bias[oc' / R] + activation in the epilogue IF the chosen
  // kernel can (the pointwise GEMM, conv_pw.hip); *up_bias_done reports it, else the caller
  // runs its bias / activation pass on the output
  const float* up_bias = nullptr;
  int up_act = 0;
  int* up_bias_done = nullptr;
  // gradient-mask epilogue (data gradient fused with the activation backward of the layer
  // that produced this conv's input): out = conv * act'(gm_src), gm_dbias += column sums.
  // gm_src: that layer's activated output with dense rows (nullptr = linear activation).
  // e2i_igemm_conv reports in *gm_done whether the chosen kernel did it (else the caller
  // runs the activation backward in place on the output).
  int gm = 0;
  const float* gm_src = nullptr;
  int64_t gsN = 0, gsC = 0, gsZ = 0;
  float* gm_dbias = nullptr;
  const float* gm_bias = nullptr;   // non-null: gm_src is the PRE-activation, slope from gm_src + gm_bias[c]
  int* gm_done = nullptr;
  // split-K zero-fill of an output that is the interior of a zero-padded scratch buffer:
  // the whole buffer may be filled flat (batched by the caller), nullptr = fill the view
  float* fill_base = nullptr;
  size_t fill_n = 0;
  // data gradient: `in` is dy zero-padded by kd - 1 planes at both ends of z (the contract
  // of e2_conv3d_dgrad*): the kernels skip the tap planes that read only that border
  int zpad = 0;
  // split-K with partial-sum stores instead of atomics (e2_conv3d_*_packed_parts): up to
  // parts_max splits, split s stores to out + s * part_stride; *nparts receives the number
  // of parts written (1: `out` holds the complete result).  parts_max <= 1: off.
  int parts_max = 0;
  int64_t part_stride = 0;
  int* nparts = nullptr;
};

// The GEMM of `rows` output channels that reads the view `in` through a kd x kh x kw kernel and
// writes the view `out`, UpConv scatter off.  Everything else -- image dims, zpad, parts,
// epilogues, fill_base, UpConv factors (and then the low-resolution extents) -- is the call
// site's.
static inline IgemmArgs igemm_args(const e2_tensor5& in, const e2_tensor5& out, const float* wp,
                                   int rows, int kd, int kh, int kw) {
  IgemmArgs a;
  a.in = in.ptr; a.wp = wp; a.out = out.ptr;
  a.N = in.n; a.Cin = in.c; a.Cout = rows;
  a.kd = kd; a.kh = kh; a.kw = kw;
  a.Do = out.d; a.Ho = out.h; a.Wo = out.w;
  a.isN = in.sn; a.isC = in.sc; a.isZ = in.sd; a.isY = in.sh;
  a.osN = out.sn; a.osC = out.sc; a.osZ = out.sd; a.osY = out.sh;
  return a;
}

struct WgradArgs {
  const float* x = nullptr;     // input activations view
  const float* dy = nullptr;    // output-gradient view (unpadded dims)
  float* dw = nullptr;          // [M][Cin*T] dense, accumulated atomically (pre-zeroed)
  int N = 0, Cin = 0, Cout = 0;
  int kd = 0, kh = 0, kw = 0;
  int Do = 0, Ho = 0, Wo = 0;
  int64_t xsN = 0, xsC = 0, xsZ = 0, xsY = 0;
  int64_t dsN = 0, dsC = 0, dsZ = 0, dsY = 0;
  int flip = 0;           // store tap index reversed
  int upR = 1;            // >1: rows are (co*R + r); store dw[co][col][r] (UpConv)
  int accumulate = 0;     // 1: dw += grad (caller zeroed it); 0: dw = grad
  int dy_padded = 0;      // 1: dy is the interior of a zero-padded buffer (row gaps hold
                          //    zeros, >= 128 readable bytes follow its last element)
};

// The weight gradient of a kd x kh x kw kernel from the input view x and the gradient view dy
// (UNPADDED extents; a padded buffer's interior is passed as the view of that interior); a conv's
// tap order (flip), no UpConv rows.
static inline WgradArgs wgrad_args(const e2_tensor5& x, const e2_tensor5& dy, float* dw, int kd,
                                   int kh, int kw, int accumulate, int dy_padded) {
  WgradArgs a;
  a.x = x.ptr; a.dy = dy.ptr; a.dw = dw;
  a.N = x.n; a.Cin = x.c; a.Cout = dy.c;
  a.kd = kd; a.kh = kh; a.kw = kw;
  a.Do = dy.d; a.Ho = dy.h; a.Wo = dy.w;
  a.xsN = x.sn; a.xsC = x.sc; a.xsZ = x.sd; a.xsY = x.sh;
  a.dsN = dy.sn; a.dsC = dy.sc; a.dsZ = dy.sd; a.dsY = dy.sh;
  a.flip = 1;
  a.accumulate = accumulate; a.dy_padded = dy_padded;
  return a;
}

// ---- the route of a weight-gradient launch --------------------------------------------------
// The five integers "MT,NT,WK,BP,PS" of a weight-gradient tiling -- a forced string or the cost
// model's choice (choose_wcfg returns integers for both) -- are decoded HERE, once per launch;
// e2i_wgrad_conv switches on the family, the launchers read the named fields.  Tried in this
// order (the same words: tiling.py wgrad_route):
//   WK == 7                          the K-contiguous 1x1x1 GEMM (BP ignored)           pw_wgrad
//   WK == 8                          ... one tile per work-group, waves split positions pw_wgrad_ks
//   WK == 9                          ... for kernels with taps                          wgrad_ks
//       (8 / 9 with BP >= 1: the "even" form, PS work-groups over BP bands)
//   WK == 18 / 19                    8 / 9 with every f32 product made of six bf16
//                                    MFMA products (same families, same BP / PS)       pw_wgrad_ks / wgrad_ks
//   dy padded, WK in {1, 14, 101, 114}, BP in {128, 256}
//                                    the direct kernel; WK % 100 == 14: the waves split
//                                    the quads; WK >= 100: XCD-grouped block order      wgrad_direct
//   otherwise WK == 14 or WK >= 100  refused
//   otherwise BP not 64 or 128       refused
//   otherwise WK in {0, 1}, or WK == 4 with NT == 1 (the waves split K)
//                                    the LDS-staged kernel                              wgrad_lds
//   otherwise                        refused
// A refused route keeps the family of the LDS-staged kernel: that is the name e2_last_launch has
// for it, noted before the refusal is raised.
enum E2WgradFamily { E2_WG_LDS, E2_WG_DIRECT, E2_WG_PW, E2_WG_PW_KS, E2_WG_KS };
struct E2WgradRoute {
  int family = E2_WG_LDS;
  int MT = 0, NT = 0;
  int BP = 0;                   // LDS / DIRECT: positions per tile (else 0)
  bool wave_split = false;      // LDS: WK == 4;  DIRECT: WK % 100 == 14
  bool xcd = false;             // DIRECT: WK >= 100
  int splits = 0;               // PS: position splits (even form: the number of work-groups)
  int bands = 0, groups = 0;    // PW_KS / KS, even form: BP bands, PS work-groups (else 0)
  bool six = false;             // PW_KS / KS: WK 18 / 19, six bf16 products per f32 product
  const char* refuse = nullptr; // non-null: no kernel runs these integers, and why
};
static inline E2WgradRoute e2_wgrad_route(const int v[5], bool dy_padded) {
  E2WgradRoute r;
  const int WK = v[2], BP = v[3];
  r.MT = v[0]; r.NT = v[1]; r.splits = v[4];
  if (WK == 7) { r.family = E2_WG_PW; return r; }
  if (WK == 8 || WK == 9 || WK == 18 || WK == 19) {
    r.family = WK % 10 == 8 ? E2_WG_PW_KS : E2_WG_KS;
    r.six = WK >= 18;
    if (BP >= 1) { r.bands = BP; r.groups = v[4]; }
    return r;
  }
  r.BP = BP;
  if (dy_padded && (WK == 1 || WK == 14 || WK == 101 || WK == 114) && (BP == 128 || BP == 256)) {
    r.family = E2_WG_DIRECT; r.wave_split = WK % 100 == 14; r.xcd = WK >= 100;
    return r;
  }
  if (WK == 14 || WK >= 100) r.refuse = "wgrad: WK=14/101/114 need the padded-gradient entry point and BP 128/256";
  else if (BP != 64 && BP != 128) r.refuse = "wgrad: BP must be 64 or 128";
  else if (!(WK == 0 || WK == 1 || (WK == 4 && r.NT == 1))) r.refuse = "wgrad: WK=4 needs NT=1";
  else r.wave_split = WK == 4;
  return r;
}
static inline const char* e2_wgrad_family_name(const E2WgradRoute& r, bool bf16) {
  switch (r.family) {
    case E2_WG_PW: return "pw_wgrad";
    case E2_WG_PW_KS: return "pw_wgrad_ks";
    case E2_WG_KS: return "wgrad_ks";
    case E2_WG_DIRECT: return bf16 ? "wgrad_direct_bf16r" : "wgrad_direct";
  }
  return "wgrad_lds";
}

// ---- what the K-contiguous GEMMs (WK 7 / 8 / 9 / 18 / 19) can run ---------------------------------------
// The clause that refuses, or nullptr.  choose_wcfg asks (a forced 7 / 8 / 9 that gets a clause
// takes the cost model's choice: "fallback"), and the launchers ask again through E2_REQUIRE.  The
// clauses only the launchers have -- a forced string that meets one is an error -- stand there.
// WK 7, 8 and 18: a 1x1x1 kernel on dense channel planes, f32 mode
static inline const char* e2_pw_wgrad_limit(const WgradArgs& a, bool bf16, int /*input_slack*/) {
  if (!(a.kd == 1 && a.kh == 1 && a.kw == 1)) return "pointwise wgrad: the kernel is not 1x1x1";
  if (!(a.xsY == a.Wo && a.xsZ == (int64_t)a.Ho * a.Wo && a.dsY == a.Wo && a.dsZ == (int64_t)a.Ho * a.Wo))
    return "pointwise wgrad: x and dy need dense channel planes (row stride = W, plane stride = H * W)";
  if (bf16) return "pointwise wgrad: an f32 kernel, not offered in bf16 mode";
  return nullptr;
}
// WK 9 and 19: taps; the padded gradient at the input's row pitch with >= 31 zeros behind a plane; f32
// mode; 128 readable bytes behind x; 32-bit byte offsets inside a sample
static inline const char* e2_wgrad_ks_limit(const WgradArgs& a, bool bf16, int input_slack) {
  const int64_t Din = a.Do + a.kd - 1, Hin = a.Ho + a.kh - 1;
  const int64_t K = (int64_t)(a.Ho - 1) * a.dsY + a.Wo;       // memory span of a gradient plane
  if (!(a.kd * a.kh * a.kw > 1 && a.upR <= 1)) return "wgrad (position-split GEMM): a conv kernel with taps";
  if (!a.dy_padded) return "wgrad (position-split GEMM): dy must be the interior of its zero-padded buffer";
  if (a.dsY != a.xsY) return "wgrad (position-split GEMM): dy rows at the input's pitch";
  if ((a.kh - 1) * a.xsY + (a.kw - 1) < 31) return "wgrad (position-split GEMM): the kernel's rows leave fewer than 31 zeros behind a plane";
  if (bf16) return "wgrad (position-split GEMM): an f32 kernel, not offered in bf16 mode";
  if (!(a.xsZ >= Hin * a.xsY && a.xsC >= Din * a.xsZ)) return "wgrad (position-split GEMM): x planes / channels overlap";
  if (!(((int64_t)a.Cout * a.dsC + (int64_t)a.Do * a.dsZ + K) * 4 + 256 < ((int64_t)1 << 32) &&
        ((int64_t)a.Cin * a.xsC + Din * a.xsZ) * 4 + 256 < ((int64_t)1 << 32) && a.dsC >= 0 && a.xsC >= 0))
    return "wgrad (position-split GEMM): sample too large for 32-bit byte offsets";
  if (input_slack < 128) return "wgrad (position-split GEMM): needs e2_set_input_slack(ctx, >= 128)";
  return nullptr;
}

// views the call sites cut or make up before they call a builder
static inline e2_tensor5 e2_interior(const e2_tensor5& t, int pd, int ph, int pw) {   // of a padded buffer
  e2_tensor5 v = t;
  v.ptr = t.ptr + (int64_t)pd * t.sd + (int64_t)ph * t.sh + pw;
  v.d = t.d - 2 * pd; v.h = t.h - 2 * ph; v.w = t.w - 2 * pw;
  return v;
}
static inline e2_tensor5 e2_dense_view(float* ptr, int n, int c, int d, int h, int w) {
  const int64_t S = (int64_t)d * h * w;
  return e2_tensor5{ptr, n, c, d, h, w, c * S, S, (int64_t)h * w, (int64_t)w};
}
