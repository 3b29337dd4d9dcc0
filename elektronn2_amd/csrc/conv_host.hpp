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
