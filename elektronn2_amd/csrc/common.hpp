// Internal helpers shared by the libe2hip translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include "../../include/e2hip.h"
#include "conv_host.hpp"

struct e2_ctx {
  int device;
  hipStream_t stream;
  int num_cu;
  bool capturing;
  float* zeros;        // 1 KiB of zeros in device memory (masked-lane DMA source)
  hipEvent_t fork_ev[32];   // dependency events of e2_stream_fork / e2_stream_join
  int fork_next;
  int mfma_bf16;       // e2_set_mfma_dtype: 1 = conv GEMMs round their operands to bf16
  int skip_zero_fill;  // e2_set_skip_zero_fill: split-K outputs were zeroed by the caller
  float* last_fill_ptr;     // flat region the last conv launch zero-filled (n = 0: none)
  size_t last_fill_n;
  char tiling[2][kE2TilingChars];   // e2_set_tiling: forced tiling of the igemm / wgrad launches ("" = cost model)
  E2Tiling tiling_v[2];     // ... parsed there, once; the launches read this (the string: messages, debug log)
  int loss_sum_mode;        // e2_set_loss_grad_mode: 1 = NLL gradients are NOT divided by the labelled count
  float* loss_count_out;    // ... and the count is also written here (the slot behind the gradient arena)
  int input_slack;          // e2_set_input_slack: finite readable bytes behind the x of the launches that follow
  int image_rows;           // e2_set_image_rows: floats per k-row of the packed images the next launches read (0 = formula)
  int dgrad_zinset;         // e2_set_dgrad_zinset: z planes cut off either side of the padded gradient the next dgrad launches read
  char last_launch[160];    // e2_last_launch: "<kernel family> <tiling that ran> <forced|model|fallback>"
  unsigned tiling_fallbacks;   // launches since e2_ctx_create whose forced tiling was NOT the one that ran
};

// record the conv GEMM launch that is about to be issued (api.hip; src: E2_SRC_*, conv_host.hpp)
void e2_note_launch(e2_ctx* ctx, const char* family, int src, const char* fmt, ...);

// Debug switches (timing ablations, in-kernel stamps, verbose launch log) are compiled in
// only with -DE2_DEBUG_ENV (make DEBUG_ENV=1): the release library never reads the process
// environment -- tilings arrive through e2_set_tiling().
#ifdef E2_DEBUG_ENV
#include <stdlib.h>
static inline const char* e2_dbg_env(const char* name) { return getenv(name); }
#else
static inline const char* e2_dbg_env(const char*) { return nullptr; }
#endif
static inline int e2_dbg_env_int(const char* name) {
  const char* v = e2_dbg_env(name);
  return v ? atoi(v) : 0;
}

void e2_set_error(const char* fmt, ...);

#define E2_CHECK_HIP(expr)                                                   \
  do {                                                                       \
    hipError_t _e = (expr);                                                  \
    if (_e != hipSuccess) {                                                  \
      e2_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr,             \
                   hipGetErrorString(_e));                                   \
      return 1;                                                              \
    }                                                                        \
  } while (0)

#define E2_REQUIRE(cond, ...)                                                \
  do {                                                                       \
    if (!(cond)) {                                                           \
      e2_set_error(__VA_ARGS__);                                             \
      return 2;                                                              \
    }                                                                        \
  } while (0)

// e2_nll_weights as the loss kernels take it (softmax_nll.hip, head.hip, tail.hip): null = default
struct NllW {
  const float* cw;                  // class weights [ncls]
  const float* lab;                 // mask_class_labeled [n][ncls]
  const float* npr;                 // mask_class_not_present [n][ncls]
  const float* ew;                  // example weights (n, 1, d, h, w)
  long esN, esD, esH;
};
// One of the few floats behind an NllW pointer (class weights, masks): memory that no kernel of
// the grid writes, read at a wave-uniform index.  Through the constant address space, so that the
// read is a scalar load -- once per wave, not per lane -- also behind the kernel's own stores
// (hipcc cannot prove those do not alias a plain pointer and would issue a per-lane load).
#ifdef __HIPCC__
__device__ __forceinline__ float e2_uniform_ld(const float* p, int i) {
  return ((const __attribute__((address_space(4))) float*)p)[i];
}
#endif

static inline int e2i_nll_weights(const e2_nll_weights* w, const e2_tensor5* target,
                                  const char* who, NllW* out) {
  *out = NllW{};
  if (!w) return 0;
  out->cw = w->class_w; out->lab = w->labelled; out->npr = w->not_present;
  if (const e2_tensor5* e = w->example_w) {
    E2_REQUIRE(e->ptr && e->c == 1 && e->n == target->n && e->d == target->d &&
                   e->h == target->h && e->w == target->w,
               "%s: example_w must be (n,1,d,h,w) matching the target", who);
    out->ew = e->ptr; out->esN = e->sn; out->esD = e->sd; out->esH = e->sh;
  }
  return 0;
}

static inline int e2_cdiv(int a, int b) { return (a + b - 1) / b; }
static inline int64_t e2_cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- internal launchers (defined in the .hip files) ---------------------

// IgemmArgs / WgradArgs and their builders: conv_host.hpp
int e2i_igemm_conv(e2_ctx*, const IgemmArgs& a);
int e2i_pw_conv(e2_ctx*, const IgemmArgs& a, int MT, int NT, int KC);   // 1x1x1 GEMM with LDS-staged weights (conv_pw.hip)

// Wp[dz][t][ic(ciP)][oc(coP)] = w[(oc/Rout)*wsO + (ic/Rin)*wsI + tap + oc%Rout + ic%Rin],
// tap = (dz*kh*kw+t), reversed when flip.  Zero in the padding.  Cout/Cin are
// the GEMM's channel counts (already multiplied by Rout/Rin).  Rout/Rin > 1 fold
// UpConv's sub-position r into the out / in channel index (kd=kh=kw=1 then).
int e2i_pack_weights(e2_ctx*, const float* w, float* wp, int Cout, int Cin,
                     int kd, int kh, int kw, int64_t wsO, int64_t wsI, int flip,
                     int ciP, int coP, int Rout, int Rin);
void e2i_pack_dims(int cout, int cin, int* ciP, int* coP);

int e2i_upconv_dpre_s2d(e2_ctx*, const e2_tensor5* dout, const e2_tensor5* yout, int pz,
                        int py, int px, int act, float* s2d, float* dbias);
// the weight gradient: e2i_wgrad_conv decodes the tiling into its route (conv_host.hpp) and runs the
// LDS-staged kernel itself or hands the route to the launcher of its family
int e2i_wgrad_conv(e2_ctx*, const WgradArgs& a);
int e2i_wgrad_direct(e2_ctx*, const WgradArgs& a, const E2WgradRoute& r);   // conv_wgrad_direct.hip (needs dy_padded)
size_t e2i_wgrad_direct_buf_floats(const WgradArgs& a, int NT, int BP, int WK);
// conv_pw_wgrad.hip: the GEMMs with K-contiguous operands (1x1x1 / UpConv; with taps)
int e2i_pw_wgrad(e2_ctx*, const WgradArgs& a, const E2WgradRoute& r);
int e2i_pw_wgrad_ks(e2_ctx*, const WgradArgs& a, const E2WgradRoute& r);
int e2i_wgrad_ks(e2_ctx*, const WgradArgs& a, const E2WgradRoute& r);

// raise a kernel's dynamic-LDS limit once (*done: the flag of the launcher's template instance;
// one device per process: plan.py get_ctx)
static inline int e2i_raise_lds(const void* kernel, int bytes, bool* done) {
  if (*done) return 0;
  hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) { e2_set_error("hipFuncSetAttribute: %s", hipGetErrorString(e)); return 1; }
  *done = true;
  return 0;
}

// fill helpers (view_ops.hip, arena_ops.hip)
int e2i_fill_view(e2_ctx*, const e2_tensor5* v, float value);
int e2i_fill_flat(e2_ctx*, float* ptr, size_t n, float value);   // kernel fill (graph safe)
