/* e2hip.h -- C ABI of libe2hip.so: MI355X (gfx950) kernels for the 3-D
 * conv / pool / upconv training step behind ELEKTRONN2's neuromancer
 * Conv / Pool / UpConv nodes.
 *
 * The reference has NO FFI for this path: its seam is the Theano op calls in
 * elektronn2/neuromancer/computations.py and the one theano.function() call in
 * graphutils.py:376-387.  Each entry point below names the reference call it
 * replaces (paths relative to /root/reference/elektronn2/).
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; the message is
 *     available from e2_last_error() (thread-local).
 *   - all data pointers are DEVICE pointers owned by the caller; workspace sizes
 *     come from e2_*_workspace_bytes().  The library's only device allocation is
 *     one 1 KiB page of zeros per context, made in e2_ctx_create and released in
 *     e2_ctx_destroy (source of masked DMA lanes); a -DE2_DEBUG_ENV build may also
 *     allocate in-kernel timeline buffers when asked to through the environment.
 *   - the release library never reads the process environment: tilings arrive
 *     through e2_set_tiling().
 *   - layouts: activations (b,f,z,x,y) = NCDHW, fp32; weights
 *     (n_f, n_in, kz, kx, ky) = KCDHW, fp32  (neural.py:615-623 'dnn' order).
 *     Tensors are described by e2_tensor5: sizes + element strides, so crops,
 *     channel-concat slices and zero-padded gradient buffers are views.
 *     The innermost (y / "W") stride must be 1.
 *   - one hipStream_t per context; launches are asynchronous on it; no
 *     internal threads; nothing here synchronises the device, so every call is
 *     legal inside hipStreamBeginCapture/EndCapture (e2_graph_*).
 */
#ifndef E2HIP_H
#define E2HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct e2_ctx e2_ctx;

/* 5-D fp32 tensor view. n = batch, c = features, d/h/w = z/x/y spatial.
 * Strides in ELEMENTS; the w stride is implicitly 1. */
typedef struct e2_tensor5 {
  float*  ptr;
  int32_t n, c, d, h, w;
  int64_t sn, sc, sd, sh;
} e2_tensor5;

/* computations.py:57-134 apply_activation.  Every entry point that takes an `act` accepts LIN and
 * RELU; the values behind them are taken by e2_act_fwd / e2_act_bwd alone. */
enum { E2_ACT_LIN = 0, E2_ACT_RELU = 1, E2_ACT_TANH, E2_ACT_SIGMOID, E2_ACT_ABS,
       E2_ACT_ELU, E2_ACT_SELU, E2_ACT_SOFTPLUS };
enum { E2_MFMA_F32 = 0, E2_MFMA_BF16 = 1 };
enum { E2_TILING_IGEMM = 0, E2_TILING_WGRAD = 1 };

/* ---- context / stream / errors --------------------------------------- */
int  e2_ctx_create(int device, e2_ctx** out);
int  e2_ctx_destroy(e2_ctx* ctx);
/* stream: a hipStream_t (as void*); NULL = the default stream. */
int  e2_ctx_set_stream(e2_ctx* ctx, void* stream);
const char* e2_last_error(void);
int  e2_version(void);
/* Arithmetic of the convolution GEMMs (no reference counterpart: Theano computes in
 * float32 throughout).  E2_MFMA_F32 (default): f32 operands, exact f32
 * products and sums.  E2_MFMA_BF16: the operands of the packed-weight forward / data-
 * gradient kernels (tap rows of 1, 3, 4 or 5) and of e2_conv3d_wgrad_pad are rounded
 * to bf16 (nearest even) on their way into the matrix core; products and sums stay f32;
 * tensors in memory stay f32.  The first-layer, head, generic-width kernels and the plain
 * e2_conv3d_wgrad entry point always compute in f32 (UpConv follows the setting, and so do the
 * two GEMMs of e2_tail_fwd_bwd's 1x1x1 layer; its head stays f32).  Not to be changed while a graph is being captured. */
int  e2_set_mfma_dtype(e2_ctx* ctx, int dtype);
int  e2_get_mfma_dtype(const e2_ctx* ctx);
/* Tiling of the conv GEMM launches (no reference counterpart; stands where Theano's
 * per-op algorithm choice `dnn_conv3d(..., algo=...)` stood, computations.py:30,391).
 * A tiling string is a comma-separated list of at most 8 integers (an optional '-' and decimal
 * digits each, within 32 bits), nothing else -- no blanks, no '+', no trailing comma -- of at most
 * 63 characters.  It is parsed HERE, once (csrc/conv_host.hpp); anything else is an error of this
 * call.  With n integers v0, v1, ... this call accepts, for kind E2_TILING_IGEMM: n == 4, n == 5,
 * n == 3 with v0 == 1 or 32, n == 8 with v0 == 4; for kind E2_TILING_WGRAD: n == 5.  The
 * launches then read the list: a packed forward / dgrad / UpConv launch runs n == 4 (16x16x4),
 * n == 3 or 5 with v0 == 1 (pointwise), n == 8 with v0 == 4 (4x4x1) and refuses every other list;
 * e2_conv3d_{fwd,dgrad}_bf16* honour n >= 3 with v0 == 32 (so "32,2,2,1" is a 16x16x4 tiling to
 * the former and the tile (2, 2) to the latter); e2_conv3d_wgrad* take n == 5 as "MT,NT,WK,BP,PS";
 * e2_conv3d_wgrad_bf16* honour n == 5 with v0 == 32.  elektronn2_amd/tiling.py states the same
 * grammar for the host side.
 * kind E2_TILING_IGEMM: cfg = "MT,NT,CC,SK" for the packed forward / dgrad / UpConv
 * launches (16x16x4 MFMA kernel: 16*MT output channels x 64*NT positions per work-group,
 * CC input channels per LDS chunk, SK-way split of K), or cfg = "4,MG,NT,CC,SK,WM,WN,G"
 * (4x4x1 MFMA kernel, persistent: 4*MG channels x 64*NT positions per WAVE, WM x WN <= 12
 * compute waves per work-group along the channels / positions, G work-groups per CU
 * walking the tiles), or, for 1x1x1 kernels and UpConv, cfg = "1,MT,NT" / "1,MT,NT,KC,0" (the
 * GEMM with LDS-staged weights of conv_pw.hip: 16*MT channels x 64*NT positions per
 * work-group, KC = 32 / 64 / 128 reduction channels per pipeline chunk, 32 in the short form;
 * for UpConv its epilogue scatters depth-to-space and applies bias + activation);
 * kind E2_TILING_WGRAD: cfg = "MT,NT,WK,BP,PS" for
 * e2_conv3d_wgrad / e2_conv3d_wgrad_pad, decoded once per launch into the kernel that runs it
 * (e2_wgrad_route, csrc/conv_host.hpp: the whole table) (WK 1 / 14 direct kernel, 0 / 4 LDS-staged, 7 =
 * "MT,NT,7,0,S": 1x1x1 kernels and UpConv, the GEMM with K-contiguous operands of
 * conv_pw_wgrad.hip, 2 x 2 waves of MT x NT blocks, S position splits; 8 = "MT,NT,8,0,S": the
 * same GEMM with ONE 16 MT x 16 NT tile of dW per work-group whose four waves split the positions
 * and sum their partial tiles through LDS; 9 = "MT,NT,9,0,S": that kernel for a conv WITH taps --
 * every (input channel, tap) column of dW is a K-contiguous row of x at the tap's constant shift;
 * e2_conv3d_wgrad_pad only: needs the gradient at the input's row pitch, (kh - 1) input rows
 * + kw - 1 >= 31 zeros behind a gradient plane, f32 mode and e2_set_input_slack(ctx, >= 128);
 * 18 / 19 = the forms 8 / 9 with every f32 product made of six bf16 MFMA products
 * (v_mfma_f32_16x16x32_bf16 on exact hi + mid + lo pieces of both operands: f32-accurate sums,
 * +-inf in an operand gives NaN; an error in bf16 mode);
 * BP positions per tile, PS position splits).  The forms 7, 8 and 9 (18, 19) are exempt from the rule
 * below: where their layout requirements are not met the call takes the cost model's choice --
 * a FALLBACK, which e2_last_launch() reports as such and e2_tiling_fallbacks() counts (the tuning
 * keys hold the row pitch, not the plane pitch, so a shipped entry can meet a view it cannot
 * run; a caller that wants the error checks e2_last_launch after the call).  The setting holds for every following
 * launch of that kind on this context until changed; cfg NULL or "" returns the choice
 * to the library's cost model.  A tiling the problem cannot use (LDS, instance list)
 * makes the launch fail with an error, never silently fall back.  A launch captured
 * into a graph keeps the tiling that was set at capture time. */
int  e2_set_tiling(e2_ctx* ctx, int kind, const char* cfg);
/* Which kernel the last conv GEMM launch of this context ran (packed forward / data gradient /
 * UpConv, weight gradient, f32 and bf16 forms; same seam: Theano reports the chosen `algo` of a
 * dnn conv op in its profile, computations.py:30,391).  buf receives
 * "<kernel family> <tiling that ran> <source>", e.g. "wgrad_ks 13,2,9,0,4 forced":
 *   family: igemm | igemm_bf16r | igemm_generic | igemm4 | pw_gemm | conv_bf16 |
 *           wgrad_ks | pw_wgrad_ks | pw_wgrad | wgrad_direct | wgrad_direct_bf16r | wgrad_lds |
 *           wgrad_bf16
 *   source: "forced"   = the e2_set_tiling string was honoured,
 *           "model"    = no string was set, the library's cost model chose,
 *           "fallback" = a string was set but this launch could not run it and took the cost
 *                        model's choice (weight-gradient forms 7 / 8 / 9 only; every other
 *                        unrunnable string is an ERROR of the launch).
 * Host-side bookkeeping, legal during capture; "" before the first launch.
 * e2_tiling_fallbacks: number of "fallback" launches since e2_ctx_create. */
int  e2_last_launch(e2_ctx* ctx, char* buf, int n);
unsigned e2_tiling_fallbacks(const e2_ctx* ctx);

/* ---- conv  (computations.py:364-428 conv(), 3-D branch; F1: true
 *      convolution, kernel flipped in every spatial dim, 'valid') --------- */
/* bytes of workspace conv fwd / dgrad need for the packed weight image. */
size_t e2_conv3d_workspace_bytes(int cout, int cin, int kd, int kh, int kw);

/* y = conv_valid_flip(x, w).  y must be (n, cout, d-kd+1, h-kh+1, w-kw+1).
 * w: dense KCDHW [cout][cin][kd][kh][kw].  ws: workspace (device). */
int e2_conv3d_fwd(e2_ctx*, const e2_tensor5* x, const float* w,
                  int cout, int kd, int kh, int kw,
                  const e2_tensor5* y, void* ws, size_t ws_bytes);

/* dx = d(loss)/dx given dy (replaces Theano's GpuDnnConv3dGradI /
 * conv3d2d grad born at model.py:182).  dy_pad is dy stored in the interior
 * of a buffer zero-padded by (kd-1, kh-1, kw-1) on every side:
 * dy_pad dims = (n, cout, do+2(kd-1), ho+2(kh-1), wo+2(kw-1)); the border
 * MUST be zero.  dx dims = (n, cin, do+kd-1, ho+kh-1, wo+kw-1). */
int e2_conv3d_dgrad(e2_ctx*, const e2_tensor5* dy_pad, const float* w,
                    int cin, int kd, int kh, int kw,
                    const e2_tensor5* dx, void* ws, size_t ws_bytes);

/* Split form of the two calls above: the packed weight image depends only on
 * w, so a caller that runs many convolutions with the same weights (or wants
 * the repack off the critical path) packs once.  mode 0 = forward image,
 * mode 1 = dgrad image.  ws must hold e2_conv3d_workspace_bytes(). */
int e2_conv3d_pack(e2_ctx*, const float* w, int cout, int cin, int kd, int kh,
                   int kw, int mode, void* ws, size_t ws_bytes);
int e2_conv3d_fwd_packed(e2_ctx*, const e2_tensor5* x, const void* wp, int cout,
                         int kd, int kh, int kw, const e2_tensor5* y);
int e2_conv3d_dgrad_packed(e2_ctx*, const e2_tensor5* dy_pad, const void* wp,
                           int cin, int kd, int kh, int kw, const e2_tensor5* dx);
/* Conv layer WITHOUT pooling, fused: out = act(conv(x, w) + bias[oc]) in the GEMM's
 * epilogue (neural.py:662-712 with pool_shape all ones).  Needs dense output rows
 * and a kernel width of 1, 3, 4 or 5 (e2_conv3d_fwd_packed + e2_pool_bias_act_fwd
 * otherwise).  relu stores -0.0 where the pre-activation was negative and +0.0
 * where it was exactly 0 (equal values; the sign is what e2_bias_act_bwd_out reads
 * to reproduce Theano's relu'(0) = 0.5). */
int e2_conv3d_fwd_packed_act(e2_ctx*, const e2_tensor5* x, const void* wp, int cout,
                             int kd, int kh, int kw, const float* bias, int act,
                             const e2_tensor5* out);
/* its backward: dy = dout * act'(out) (dy may be the interior of the padded gradient
 * buffer), dbias[oc] += sum(dy) when dbias != NULL. */
int e2_bias_act_bwd_out(e2_ctx*, const e2_tensor5* dout, const e2_tensor5* out, int act,
                        const e2_tensor5* dy, float* dbias);
/* e2_conv3d_dgrad_packed FUSED with e2_bias_act_bwd_out of the layer that produced this
 * conv's input (a conv layer without pooling whose only consumer is this conv; T.grad's
 * chain ConvGradI -> relu', model.py:182):
 *   dy_prev = dgrad(dy_pad, w) * act_prev'(out_prev),  dbias_prev[c] += sum(dy_prev[c])
 * written straight into the INTERIOR of that layer's zero-padded gradient buffer
 * dy_pad_prev (n, cin, d + 2 pd, h + 2 ph, w + 2 pw), interior at (pd, ph, pw); its border
 * must be (and stays) zero.  out_prev (n, cin, d, h, w) = that layer's activated output
 * as e2_conv3d_fwd_packed_act stored it (bias_prev == NULL), or -- for a layer whose forward
 * ran as e2_conv3d_fwd_packed + e2_pool_bias_act_fwd with a (1,1,1) window -- its
 * PRE-activation conv output, the slope then being act'(out_prev + bias_prev[c]).  The mask is applied in the GEMM's epilogue (also
 * under split-K: it is linear in the partial sums; a contiguous dy_pad_prev is then
 * zero-filled whole); tilings without that epilogue run the two steps one after the other,
 * in place.  dbias_prev may be NULL. */
int e2_conv3d_dgrad_packed_actbwd(e2_ctx*, const e2_tensor5* dy_pad, const void* wp, int cin,
                                  int kd, int kh, int kw, const e2_tensor5* out_prev,
                                  int act_prev, const float* bias_prev,
                                  const e2_tensor5* dy_pad_prev, int pd, int ph, int pw,
                                  float* dbias_prev);

/* dw[cout][cin][kd][kh][kw] = d(loss)/dw (replaces GpuDnnConv3dGradW).
 * dy is the UNPADDED view (n, cout, do, ho, wo) (it may be the interior view
 * of a padded buffer).  dw is overwritten. */
int e2_conv3d_wgrad(e2_ctx*, const e2_tensor5* x, const e2_tensor5* dy,
                    float* dw, int kd, int kh, int kw);
/* same, but dw += gradient (no internal memset): for callers that zero one
 * flat gradient arena per step. */
int e2_conv3d_wgrad_acc(e2_ctx*, const e2_tensor5* x, const e2_tensor5* dy,
                        float* dw, int kd, int kh, int kw);
/* Fast path of the same gradient for the training plan: dy_pad is the ZERO-PADDED
 * gradient buffer that e2_conv3d_dgrad_packed reads, shape (n, cout, do+2(kd-1),
 * ho+2(kh-1), wo+2(kw-1)); the interior holds dy, the borders MUST be zero, and
 * at least 128 readable bytes must follow the buffer's last element (the kernel
 * fetches dy straight from memory, 16 bytes per lane, and masks what lies past a
 * plane).  accumulate: 0 = dw is overwritten, 1 = dw += gradient. */
int e2_conv3d_wgrad_pad(e2_ctx*, const e2_tensor5* x, const e2_tensor5* dy_pad,
                        float* dw, int kd, int kh, int kw, int accumulate);

/* Repack MANY weight tensors in one launch (after an optimiser step): fill one
 * record per (tensor, mode) with e2_pack_job_fill on the host, copy the records
 * (e2_pack_job_bytes() each) to the device, then call e2_conv3d_pack_multi.  It
 * rewrites the weight-carrying part of every image only: the images must have been
 * zero-filled (or packed by e2_conv3d_pack) once before the first call.  mode 0 / 1: a
 * conv's forward / data-gradient image; mode 2 / 3: an UpConv's (w [cout][cin][kd][kh][kw]
 * with the factors in place of the kernel extents; see e2_upconv3d_fwd_packed). */
size_t e2_pack_job_bytes(void);
int e2_pack_job_fill(void* rec, const float* w, void* wp, int cout, int cin,
                     int kd, int kh, int kw, int mode);
/* Row length of the packed conv weight images (default: cout rounded to 16, + 208 floats -- any M
 * tiling fits).  e2_pack_job_set_stride packs ONE image of e2_conv3d_pack_multi with rows of `rows`
 * floats (a multiple of 4, >= cout rounded to 16; modes 0 / 1 only); e2_set_image_rows announces
 * that length to the e2_conv3d_pack / e2_conv3d_{fwd,dgrad}_packed* calls that follow (0 = the
 * formula again): the launch that reads an image must be told the length it was packed with.  A
 * tiling whose tiles reach past the rows is an error of the launch, never an over-read.  Purpose:
 * once the tiling of a launch is known its image needs 224 instead of 416 floats per row for 200
 * channels -- the repack writes a third less, the weight rows lie closer (DESIGN finding 52).
 * UpConv images and e2_tail_fwd_bwd's images always use the formula. */
int e2_set_image_rows(e2_ctx* ctx, int rows);
int e2_pack_job_set_stride(void* rec, int rows);
/* optional, after e2_pack_job_fill: `rows` = how far the M tiles of the launch that reads this image
 * reach (number of M tiles x 16 MT of its tiling).  The repack rewrites the real rows + the padding
 * rows up to there instead of its default (rows rounded to 16, + 96: any tiling); rows beyond stay
 * zero from the one-time fill -- correct for every tiling, a bandwidth hint only. */
int e2_pack_job_set_rows(void* rec, int rows);
int e2_conv3d_pack_multi(e2_ctx*, const void* jobs_dev, int njobs);
/* the same with the launch's LDS tile sized for the largest kd * kh * kw among the jobs */
int e2_conv3d_pack_multi_ex(e2_ctx*, const void* jobs_dev, int njobs, int max_taps);

/* ---- first layer, fused (Conv node on a 1-channel input: conv -> pool -> +b ->
 *      act in one pass; neural.py:662-712).  Supported: kd = 1, pool z = 1 and
 *      (kh,kw,py,px) in {(4,4,2,2), (6,6,2,2)} -- the neuro3d nets' first layers --
 *      or (3,3,1,1), the U-Net stem; e2_conv1_supported() tells.  act: E2_ACT_LIN
 *      or E2_ACT_RELU, any other value is an error.  The backward RECOMPUTES the
 *      conv values instead of reading a stored conv output; dw / dbias are
 *      accumulated (zero them first). ---------------------------------------- */
int e2_conv1_supported(int cin, int kd, int kh, int kw, int pz, int py, int px);
int e2_conv1_pool_act_fwd(e2_ctx*, const e2_tensor5* x, const float* w,
                          const float* bias, int cout, int kh, int kw, int py,
                          int px, int act, const e2_tensor5* out);
/* workspace of the backward: per-tile partial sums, (n, cout, d, ho, wo) = dims of
 * the POOLED output gradient */
size_t e2_conv1_bwd_workspace_bytes(int n, int cout, int d, int ho, int wo, int kh, int kw);
int e2_conv1_pool_act_bwd(e2_ctx*, const e2_tensor5* x, const float* w,
                          const float* bias, const e2_tensor5* dout, int kh,
                          int kw, int py, int px, int act, float* dw, float* dbias,
                          void* ws, size_t ws_bytes);

/* ---- split-K without atomics: partial sums added up by the consumer ------------------
 * (No reference counterpart: inside Theano's compiled function the conv, the pooling and the
 * bias / activation that follows are separate ops, computations.py:364-428, 538-631,
 * neural.py:705-712; this is how the conv hands its result to the next op here.)
 * A small layer fills the chip only when its K range is split over several work-groups.
 * The plain entry points then ACCUMULATE with float atomics into a zero-filled output
 * (~1.3 TB/s chip-wide, and a fill launch).  The _parts forms store split s with plain
 * stores to y.ptr + s * part_stride instead (the caller provides max_parts such slabs,
 * nothing needs to be zero) and report in *nparts how many were written (1: y holds the
 * complete result -- the tiling did not split K); the pointwise kernel that consumes the
 * tensor anyway adds the parts up on its way:
 *   e2_pool_bias_act_fwd_parts   y = sum of the parts (left in part 0), out = act(pool(y) + b)
 *   e2_pool_bias_act_bwd_parts / e2_bias_act_bwd_out_parts   dout = sum of the parts
 * (at most 8 parts: a consumer requests every part of an element before it adds them up;
 * the sum is left in part 0 for the elements a pooling window reads -- where a window does
 * not divide an extent, the rows / columns / planes beyond the last window keep part 0's
 * own partial sum: no pass reads them)
 * Partial sums are added up for the pooling windows (1,1,1), (1,2,2), (2,1,1), (2,2,2). */
int e2_conv3d_fwd_packed_parts(e2_ctx*, const e2_tensor5* x, const void* wp, int cout, int kd,
                               int kh, int kw, const e2_tensor5* y, int64_t part_stride,
                               int max_parts, int* nparts);
int e2_conv3d_dgrad_packed_parts(e2_ctx*, const e2_tensor5* dy_pad, const void* wp, int cin,
                                 int kd, int kh, int kw, const e2_tensor5* dx,
                                 int64_t part_stride, int max_parts, int* nparts);
int e2_pool_bias_act_fwd_parts(e2_ctx*, const e2_tensor5* y, int64_t part_stride, int nparts,
                               const float* bias, int pz, int py, int px, int act,
                               const e2_tensor5* out);
int e2_pool_bias_act_bwd_parts(e2_ctx*, const e2_tensor5* dout, int64_t dout_part_stride,
                               int dout_parts, const e2_tensor5* y, const float* bias, int pz,
                               int py, int px, int act, const e2_tensor5* dy, float* dbias);
int e2_bias_act_bwd_out_parts(e2_ctx*, const e2_tensor5* dout, int64_t dout_part_stride,
                              int dout_parts, const e2_tensor5* out, int act,
                              const e2_tensor5* dy, float* dbias);

/* ---- pool + bias + activation  (computations.py:538-631 pooling();
 *      neural.py:705-712; computations.py:57-134 apply_activation) -------- */
/* out = act(maxpool(y, pool) + bias[c]) ; pool == stride, floor semantics. */
int e2_pool_bias_act_fwd(e2_ctx*, const e2_tensor5* y, const float* bias,
                         int pz, int py, int px, int act,
                         const e2_tensor5* out);
/* Given dout = dL/dout: dy = dL/dy (every element equal to its window max
 * receives the gradient -- Theano CPU tie rule; relu'(0) = 0.5) written to the
 * view dy (typically the interior of the zero-padded dgrad buffer), and
 * dbias[c] += sum(dL/dpre).  dbias must be zeroed by the caller. */
int e2_pool_bias_act_bwd(e2_ctx*, const e2_tensor5* dout, const e2_tensor5* y,
                         const float* bias, int pz, int py, int px, int act,
                         const e2_tensor5* dy, float* dbias);

/* stand-alone max-pool (neural.py:1520-1523 Pool node) */
int e2_maxpool3d_fwd(e2_ctx*, const e2_tensor5* x, int pz, int py, int px,
                     const e2_tensor5* out);
/* dx (+)= pool-backward(dout); accumulate != 0 adds into dx. */
int e2_maxpool3d_bwd(e2_ctx*, const e2_tensor5* dout, const e2_tensor5* x,
                     int pz, int py, int px, const e2_tensor5* dx,
                     int accumulate);

/* ---- average / sum pooling with a stride of its own (computations.py:538-649 pooling(), the
 *      dnn_pool route: modes 'average_inc_pad' / 'average_exc_pad' / 'sum', pad 0, any stride;
 *      neural.py:1409-1559 Pool node) --------------------------------------------------------
 * out = scale * (sum of x over the window (pz, py, px) at (oz sz, oy sy, ox sx)), walked in
 * ascending (z, y, x) order in f32; scale = 1 (SUM) or 1 / (pz py px) (AVG; at pad 0 inc_pad and
 * exc_pad coincide).  out sizes = floor((in - p) / s) + 1 per axis; windows may overlap (s < p) or
 * leave gaps (s > p).  The backward is a gather over the windows that hold each element of dx:
 * no atomics, the same bits every run; elements that no window holds are written as +0, or left
 * as they are with accumulate != 0 (dx += gradient, a plain read-add-write).  x is not needed.
 * All views arbitrary; nothing outside out / dx is written.  p < 1, s < 1, p > in, sizes that do
 * not match, another mode and a channel of 2^31 elements or more are errors. */
enum { E2_POOL_AVG = 1, E2_POOL_SUM = 2 };   /* 0 stays free for max */
int e2_pool3d_lin_fwd(e2_ctx*, const e2_tensor5* x, int pz, int py, int px, int sz, int sy,
                      int sx, int mode, const e2_tensor5* out);
int e2_pool3d_lin_bwd(e2_ctx*, const e2_tensor5* dout, int pz, int py, int px, int sz, int sy,
                      int sx, int mode, const e2_tensor5* dx, int accumulate);

/* ---- local response normalisation (neural.py:2043-2181 LRN node: 2113-2118 and 2148-2150 the
 *      'spatial' mean square as a 'same' conv of x^2 with an identity-over-features averaging
 *      filter, 2152-2176 the 'channel' one over the feature axis with a replicated edge,
 *      2179-2180 the division) -----------------------------------------------------------------
 * q = k + alpha * m, out = x * q^(-beta), m the mean square over a window:
 *   SPATIAL  the box (fz, fy, fx) around the element inside its (n, c); positions outside the
 *            tensor add 0 and the divisor is always fz fy fx.  The C x C x box filter of the
 *            reference is never built.
 *   CHANNEL  fz features around c at the same (n, z, y, x), indices clamped to [0, C - 1] (the
 *            edge feature counts once per offset that lands on it); divisor fz; fy = fx = 1.
 * Every extent is odd and >= 1 and may exceed its axis.  alpha, k, beta are DEVICE scalars read
 * when the kernels run.  The forward is one launch and also writes q where q != NULL (the backward
 * wants it).  Backward, with t = dout * x * q^(-beta-1) and N the divisor:
 *   dx_i (+)= dout_i * q_i^(-beta) - (2 alpha beta / N) * x_i * sum_j mult(i, j) * t_j
 * j over the same box, mult = 1 (SPATIAL); j over the features, mult(i, j) = the number of
 * offsets o with clamp(j + o) == i (CHANNEL).  Two launches: t into `tmp` (same sizes as x), then
 * a gather over the window of t -- no atomics, the same bits every run, windows walked in
 * ascending (z, y, x) / feature order in f32; accumulate != 0 adds into dx (a plain read-add-
 * write).  No gradient goes to alpha, k or beta; q <= 0 gives what powf gives.  All views
 * arbitrary with identical sizes; nothing outside out / q / tmp / dx is written.  Errors: sizes
 * that differ, an even or < 1 extent, another mode, a null pointer (q of the forward excepted),
 * out aliasing x, dx aliasing dout (the windows read neighbours), tmp aliasing any other view, a
 * channel of 2^31 elements or more. */
enum { E2_LRN_SPATIAL = 0, E2_LRN_CHANNEL = 1 };
int e2_lrn_fwd(e2_ctx*, const e2_tensor5* x, int mode, int fz, int fy, int fx,
               const float* alpha, const float* k, const float* beta, const e2_tensor5* q,
               const e2_tensor5* out);
int e2_lrn_bwd(e2_ctx*, const e2_tensor5* dout, const e2_tensor5* x, const e2_tensor5* q, int mode,
               int fz, int fy, int fx, const float* alpha, const float* beta,
               const e2_tensor5* tmp, const e2_tensor5* dx, int accumulate);

/* ---- UpConv  (neural.py:989-1072; computations.py:216-255 upconv(),
 *      749-782 unpooling_nd; F2: y[n,co,p*i+r] = sum_ci w[co,ci,r] x[n,ci,i]) */
/* (n,d,h,w) = dims of the UpConv INPUT x. */
size_t e2_upconv3d_workspace_bytes(int cout, int cin, int pz, int py, int px,
                                   int n, int d, int h, int w);
/* y = act(upconv(x, w) + bias); w [cout][cin][pz][py][px]; bias may be NULL
 * (then act must be LIN). */
int e2_upconv3d_fwd(e2_ctx*, const e2_tensor5* x, const float* w,
                    const float* bias, int cout, int pz, int py, int px,
                    int act, const e2_tensor5* y, void* ws, size_t ws_bytes);
/* dpre = dout * act'(y) is formed internally from the forward OUTPUT y
 * (relu: y > 0).  dx overwritten; dw overwritten; dbias overwritten.
 * Any of dx / dw / dbias may be NULL to skip it. */
int e2_upconv3d_bwd(e2_ctx*, const e2_tensor5* x, const float* w,
                    const e2_tensor5* y, const e2_tensor5* dout,
                    int pz, int py, int px, int act,
                    const e2_tensor5* dx, float* dw, float* dbias,
                    void* ws, size_t ws_bytes);
/* The same with the two packed weight images kept by the caller and refreshed once per step
 * by e2_conv3d_pack_multi (e2_pack_job_fill modes 2 = forward image, 3 = data-gradient image;
 * e2_upconv3d_image_bytes each) instead of a repack launch inside every call; ws of the
 * backward (e2_upconv3d_workspace_bytes) still holds the space-to-depth image.  accumulate
 * != 0: dw and dbias are ADDED to -- the caller cleared them (the training plan zeroes the
 * whole gradient arena with one launch), two fill launches less; dx is overwritten. */
size_t e2_upconv3d_image_bytes(int cout, int cin, int pz, int py, int px);
int e2_upconv3d_fwd_packed(e2_ctx*, const e2_tensor5* x, const float* wp_fwd,
                           const float* bias, int cout, int pz, int py, int px, int act,
                           const e2_tensor5* y);
int e2_upconv3d_bwd_packed(e2_ctx*, const e2_tensor5* x, const float* wp_dgrad,
                           const e2_tensor5* y, const e2_tensor5* dout, int pz, int py, int px,
                           int act, const e2_tensor5* dx, float* dw, float* dbias, void* ws,
                           size_t ws_bytes, int accumulate);

/* ---- layout / copies (computations.py:398-401,414-428 dimshuffles;
 *      neural.py:1152-1168 Crop; node_basic.py:1433-1440 Concat) ---------- */
/* dst[n][d][h][w][c] (dense NDHWC) <- src (NCDHW view) and back; staged
 * through LDS tiles so both sides are coalesced. */
int e2_transpose_ncdhw_to_ndhwc(e2_ctx*, const e2_tensor5* src, float* dst);
int e2_transpose_ndhwc_to_ncdhw(e2_ctx*, const float* src, const e2_tensor5* dst);
/* dst (+)= src, both arbitrary views of identical sizes. */
int e2_copy5(e2_ctx*, const e2_tensor5* src, const e2_tensor5* dst,
             int accumulate);
int e2_fill(e2_ctx*, float* ptr, size_t n, float value);

/* ---- constant padding (neural.py:1195-1279 Pad; computations.py:287-291,320-326: the 'same' /
 *      'full' border modes of conv() are the valid conv of the zero-framed input) ---------------
 * dst = src surrounded by a frame of `value`: pz planes, py rows and px columns on either side,
 * dst sizes = src sizes + 2 (pz, py, px); both arbitrary views.  One launch, one pass; nothing
 * outside the dst view is written.  frame_only != 0: only the frame is written, the interior of
 * dst keeps its contents and src is not read (may be NULL).  The backward of the Pad node is
 * e2_copy5 from the interior view of the output gradient. */
int e2_pad5(e2_ctx*, const e2_tensor5* src, const e2_tensor5* dst, int pz, int py, int px,
            float value, int frame_only);

/* Batching the zero-fills of a captured step (no reference counterpart).  A split-K conv
 * launch (forward / data gradient with a small output) zero-fills its output and then
 * accumulates with atomics; each such fill is a ~5 us kernel.  A caller that replays the
 * same launches every step can (1) ask after a launch which flat region it zeroed
 * (e2_conv_last_zero_fill: *n = 0 if none), (2) zero all of them with ONE
 * e2_fill_multi(ptrs, counts: device arrays of nregions 64-bit entries) at the start of
 * the step, and (3) wrap the launches in e2_set_skip_zero_fill(ctx, 1) ... (ctx, 0):
 * "the output is already zero".  Nothing else may write the region in between. */
int e2_fill_multi(e2_ctx*, const void* ptrs_dev, const void* counts_dev, int nregions,
                  float value);
int e2_set_skip_zero_fill(e2_ctx*, int on);

/* Several steps in ONE captured graph (no reference counterpart: training/trainer.py:186-194 hands
 * one batch to model.trainingstep per iteration and reads the loss back before the next).  Between
 * two graph launches the device idles for ~19 us however short the host's part is (DESIGN finding
 * 54); a graph of k steps has that gap once per k steps.  What differs between the k copies of the
 * step -- the batch and the loss -- goes through rings in device memory indexed by a launch count.
 * e2_step_prologue is the first launch of such a step; with L = its launches on `state` so far:
 *   dst[0 .. slot_floats) = ring[L % n_slots]            (ring != NULL; the producer -- data/batch.py's
 *                            sampler, or copies from the host -- fills slots ahead of their step)
 *   hist[(L - 1) % hist_slots][0 .. n_vals) = src[..]     (hist != NULL, L > 0: what the step BEFORE
 *                            this one left in src -- its loss; the newest loss is still in src)
 * state: two zeroed 64-bit words in device memory owned by the caller ([0] = L; advanced by the
 * work-group that finishes last).  ring / dst 16-byte aligned, slot_floats a multiple of 4;
 * launches on one state must be ordered (one stream). */
int e2_step_prologue(e2_ctx*, const float* ring, int n_slots, size_t slot_floats, float* dst,
                     const float* src, int n_vals, float* hist, int hist_slots, void* state);
/* the conv launches that follow may read up to `bytes` (finite, readable) bytes behind the last
 * element of their input x (0 withdraws the promise): required (>= 128) by the weight-gradient
 * tiling "MT,NT,9,0,S", csrc/conv_pw_wgrad.hip */
int e2_set_input_slack(e2_ctx*, int bytes);
int e2_conv_last_zero_fill(const e2_ctx*, void** ptr, size_t* n);
/* the e2_conv3d_dgrad_packed* launches that follow read a SUB-VIEW of a padded gradient that is
 * inset by `planes` z planes on either side (the data gradient of a 'same' / 'full' conv is wanted
 * on the interior of the framed input only, computations.py:287-291): of the kd - 1 zero planes
 * they may skip, kd - 1 - planes are left.  0 (the default) withdraws it. */
int e2_set_dgrad_zinset(e2_ctx*, int planes);

/* ---- loss (computations.py:175-176 softmax; loss.py:261-347
 *      MultinoulliNLL(target_is_sparse); loss.py:1357-1363 AggregateLoss) - */
/* ---- classifier head, fused: 1x1x1 conv to ncls <= 4 'lin' features + channel softmax
 *      + MultinoulliNLL (sparse target) and their gradients (neural.py:662-712 with a
 *      (1,1,1) kernel, computations.py:175-176, loss.py:261-347).  w is the dense
 *      (ncls, cin, 1,1,1) weight tensor.  stats = {sum of -log(p_t + 1e-5), #labelled},
 *      zero it before e2_head_fwd; loss = stats[0] / (stats[1] + 1e-5).  target NULL:
 *      probabilities only.  e2_head_bwd ACCUMULATES into dw / dbias; its workspace holds
 *      per-work-group partial sums (e2_head_bwd_workspace_bytes). --------------------- */
int e2_head_supported(int cin, int ncls);
int e2_head_fwd(e2_ctx*, const e2_tensor5* x, const float* w, const float* bias, int ncls,
                const e2_tensor5* target, const e2_tensor5* probs, float* stats);
size_t e2_head_bwd_workspace_bytes(int n, int cin, int ncls, int d, int h, int w);
int e2_head_bwd(e2_ctx*, const e2_tensor5* x, const float* w, const e2_tensor5* probs,
                const e2_tensor5* target, const float* stats, const e2_tensor5* dx,
                int accumulate_dx, float* dw, float* dbias, float* loss_out, void* ws,
                size_t ws_bytes);

/* ---- the TAIL of the neuro3d nets, forward AND backward in one launch (csrc/tail.hip):
 *      x -> [1x1x1 conv to c2 channels + bias + relu] -> [classifier head as above], i.e. the
 *      last two Conv nodes of examples/neuro3d.py:61-63 / neuro3d_lite.py:57-59 under
 *      Softmax + MultinoulliNLL, and T.grad of that chain (model.py:182).  Replaces
 *      e2_conv3d_fwd_packed_act + e2_head_fwd + e2_head_bwd + e2_bias_act_bwd_out +
 *      e2_conv3d_dgrad_packed of the two layers: both convs have ONE tap, so a work-group runs
 *      the whole chain for its tile of positions out of LDS.
 *      x: (n, c1, d, h, w) with dense (z, y, x) planes, c1, c2 <= 208; wp_fwd / wp_dgrad: the
 *      1x1x1 layer's packed images (e2_conv3d_pack modes 0 / 1; wp_dgrad only with dx);
 *      w_head: dense (ncls, c2), ncls <= 4; target (n, 1, d, h, w) float class ids (< 0:
 *      unlabelled).  Writes probs (n, ncls, ...), dpre = d loss / d (pre-activation of the
 *      1x1x1 layer) (n, c2, ...) -- the operand of that layer's weight gradient --, dx
 *      (optional) = d loss / d x, stats[1] = #labelled, and one slot of partial sums per
 *      work-group to ws (e2_tail_workspace_bytes; *n_slots slots).
 *      e2_tail_reduce ADDS the slots into dw_head (ncls * c2), db_head (ncls), db1 (c2) --
 *      zero those first -- and writes stats[0] = sum of -log(p_t + 1e-5) and loss_out =
 *      stats[0] / (stats[1] + 1e-5).  f32 mode only. ------------------------------------ */
int e2_tail_supported(int c1, int c2, int ncls);
size_t e2_tail_workspace_bytes(int n, int c1, int c2, int ncls, int d, int h, int w);
/* gm_mode != 0: dx is written THROUGH the activation backward of the layer that produced x
 * (e2_bias_act_bwd_out / e2_pool_bias_act_bwd with a (1,1,1) window): dx *= act'(.), and that
 * layer's bias gradient (the row sums) joins the slots (e2_tail_reduce: c1_gm = c1, db_parent);
 * dx may then be the interior of that layer's zero-padded gradient buffer (any row / plane
 * pitch).  1: relu slope read off gm_src = its activated output (signed zeros, as
 * e2_conv3d_fwd_packed_act stores them), 2: off gm_src = its pre-activation + gm_bias[c],
 * 3: linear activation. */
int e2_tail_fwd_bwd(e2_ctx*, const e2_tensor5* x, const float* wp_fwd, const float* wp_dgrad,
                    const float* bias1, int c2, const float* w_head, const float* b_head,
                    int ncls, const e2_tensor5* target, const e2_tensor5* probs,
                    const e2_tensor5* dpre, const e2_tensor5* dx, int gm_mode,
                    const e2_tensor5* gm_src, const float* gm_bias, float* stats, void* ws,
                    size_t ws_bytes, int* n_slots);
int e2_tail_reduce(e2_ctx*, const void* ws, int n_slots, int c2, int ncls, float* dw_head,
                   float* db_head, float* db1, float* stats, float* loss_out, int c1_gm,
                   float* db_parent);

/* probs = softmax_c(logits); loss_sum += sum_pos -log(p[target]+1e-5);
 * n_lab += #labelled (target in [0,C)).  stats = {loss_sum, n_lab} must be
 * zeroed by the caller.  target: (n,1,d,h,w) float class ids. */
int e2_softmax_nll_fwd(e2_ctx*, const e2_tensor5* logits,
                       const e2_tensor5* target, const e2_tensor5* probs,
                       float* stats);
/* dlogits = d(loss)/d(logits) with loss = loss_sum/(n_lab+1e-5);
 * also writes loss_out[0] = loss (device scalar). */
int e2_softmax_nll_bwd(e2_ctx*, const e2_tensor5* probs,
                       const e2_tensor5* target, const float* stats,
                       const e2_tensor5* dlogits, float* loss_out);

/* ---- MultinoulliNLL over E = n_indep independent softmaxes (Softmax(parent, n_indep = E),
 *      loss.py:82-92; sparse targets, loss.py:275-285; one normaliser, loss.py:338-346), one
 *      launch per direction for all groups and batch items.  logits / probs / dlogits are
 *      (n, E*k, d, h, w): group g owns features g*k .. g*k+k-1 and has a softmax of its own;
 *      target is (n, E, d, h, w), float class ids of group g in feature g.  With
 *        T[n,g,v] = 1 if target[n,g,v] == c for an integer c in [0,k), else 0 (negative, >= k
 *                   and non-integer ids are unlabelled)
 *      the forward writes probs and ADDS to stats = {loss_sum, n_lab} (zeroed by the caller):
 *        loss_sum = sum_{T = 1} -log(p[n, g*k + target, v] + 1e-5),   n_lab = sum T over ALL groups
 *        loss     = loss_sum / (n_lab + 1e-5)
 *      (the pred.size / n_indep / n_class factors of loss.py:342-346 cancel under AggregateLoss's
 *      mean, as for n_indep = 1) and the backward writes
 *        dlogits[n, g*k+c, v] = T * (-1/(n_lab + 1e-5) * p_t/(p_t + 1e-5)) * ([c == target] - p_c)
 *      with the probabilities of the same group, and loss_out[0] = loss.  A group without a
 *      labelled voxel gets zeros; nothing labelled: loss 0, gradient exactly 0.  target == NULL in
 *      the forward: probabilities only, stats is not touched (and may be NULL).  The backward
 *      honours e2_set_loss_grad_mode like e2_softmax_nll_bwd (sum_mode: unnormalised gradient,
 *      count_out[0] = n_lab).  All views may be strided (channel slices of wider buffers);
 *      dlogits may alias probs.  Errors, nothing launched: n_indep < 1, logits.c % n_indep != 0,
 *      target.c != n_indep, batch or spatial extents that disagree. ----------------------------- */
int e2_softmax_nll_grouped_fwd(e2_ctx*, const e2_tensor5* logits, const e2_tensor5* target,
                               const e2_tensor5* probs, int n_indep, float* stats);
int e2_softmax_nll_grouped_bwd(e2_ctx*, const e2_tensor5* probs, const e2_tensor5* target,
                               int n_indep, const float* stats, const e2_tensor5* dlogits,
                               float* loss_out);

/* ---- K MultinoulliNLL terms under one AggregateLoss ("multi-target training": one trunk, K
 *      softmax heads, loss.py:261-347 per term, 1357-1363 for the mix), 1 <= K <=
 *      E2_MAX_LOSS_TERMS.  Term j has c_j classes, n_indep = 1, logits / probs / dlogits
 *      (n, c_j, spatial_j) and a sparse target (n, 1, spatial_j) of float class ids; the terms
 *      share the batch size and may differ in class count and spatial size.  With
 *        T = 1 where the id equals an integer in [0, c_j), else 0 (negative, >= c_j and
 *            non-integer ids are unlabelled)
 *        S_j = sum_{T=1} -log(p_target + 1e-5)    N_j = sum T    L_j = S_j / (N_j + 1e-5)
 *        total  = (1/K) sum_j w_j L_j             (w = mixing_w)
 *        coef_j = w_j / (K (N_j + 1e-5))
 *        dlogits_j[c] = T coef_j (-p_t / (p_t + 1e-5)) ([c == target] - p_c)
 *      Every term has its OWN normaliser (the groups of e2_softmax_nll_grouped_* share one).  A
 *      term with nothing labelled has L_j = 0 and a gradient of exact zeros and still counts in K;
 *      nothing labelled anywhere: total 0, every gradient 0.
 *      e2_nll_multi_fwd: ONE launch for all terms; writes probs_j and ADDS to stats = 2K device
 *      floats {S_0, N_0, S_1, N_1, ...} (zeroed by the caller).  targets NULL, or all its entries
 *      NULL: probabilities only, stats is untouched and may be NULL.  The probabilities are bit-
 *      equal to e2_softmax_nll_fwd's.
 *      e2_nll_mix: one small launch; writes coef[j], term_loss[j] = L_j, count[j] = N_j (K floats
 *      each) and loss_out[0] = total.  mixing_w is DEVICE memory read when the kernel runs: a
 *      captured launch follows its contents.
 *      e2_nll_multi_bwd: ONE launch; dlogits_j may alias probs_j.
 *      logits / targets / probs / dlogits are HOST arrays of K view pointers (the views go by value
 *      into the kernel arguments); every view may be strided (channel slices of wider buffers),
 *      nothing outside the output views is written.  Errors, nothing launched: K out of range,
 *      NULL arguments, some but not all targets NULL, class / batch / spatial extents that
 *      disagree, and every call while e2_set_loss_grad_mode has sum mode on (its one count slot
 *      cannot hold K counts). ------------------------------------------------------------------ */
int e2_nll_multi_fwd(e2_ctx*, int k, const e2_tensor5* const* logits,
                     const e2_tensor5* const* targets, const e2_tensor5* const* probs,
                     float* stats);
int e2_nll_mix(e2_ctx*, int k, const float* stats, const float* mixing_w, float* coef,
               float* term_loss, float* count, float* loss_out);
int e2_nll_multi_bwd(e2_ctx*, int k, const e2_tensor5* const* probs,
                     const e2_tensor5* const* targets, const float* coef,
                     const e2_tensor5* const* dlogits);

/* ---- the same K terms where every softmax sits on a 1x1x1 'lin' conv of ONE trunk x
 *      (n, cin, d, h, w): K classifier heads fused (csrc/multihead.hip).  Head j: w_j the dense
 *      (ncls_j, cin) weights and bias_j[ncls_j] of its own parameter, probs_j (n, ncls_j, d, h, w),
 *      target_j (n, 1, d, h, w).  Supported: 2 <= k <= 8, every ncls_j >= 2, sum ncls_j <= 16,
 *      1 <= cin <= 512.
 *      e2_multihead_fwd: one launch; every element of x is read once, all sum ncls logits
 *      z_j = W_j x + b_j are formed, one softmax per head goes to probs_j, and with targets
 *      stats[2j] += S_j, stats[2j+1] += N_j as e2_nll_multi_fwd (zero stats first).  targets
 *      NULL, or all its entries NULL: probabilities only, stats untouched (may be NULL).
 *      e2_multihead_bwd: with dlogits_j as above from probs_j, target_j and coef[j] (device, from
 *      e2_nll_mix): dx = sum_j W_j^T dlogits_j written once (accumulate_dx != 0: added; dx NULL:
 *      not wanted), dw_j[ncls_j*cin] and dbias_j[ncls_j] ACCUMULATED (zero them first) through
 *      per-work-group partial sums in ws and a reduce launch.  ws:
 *      e2_multihead_bwd_workspace_bytes(n, cin, sum ncls, d, h, w) bytes.
 *      w / bias / ncls / targets / probs / dw / dbias are HOST arrays of k entries; all views may
 *      be strided (x a channel slice, probs_j slices of one concat buffer, targets channels of one
 *      buffer).  f32 arithmetic in either mfma mode.  Errors, nothing launched: an unsupported
 *      case, NULL arguments, some but not all targets NULL, class / batch / spatial mismatches, a
 *      short workspace, and every call while e2_set_loss_grad_mode has sum mode on. ------------ */
int e2_multihead_supported(int cin, int k, const int* ncls);
int e2_multihead_fwd(e2_ctx*, const e2_tensor5* x, int k, const float* const* w,
                     const float* const* bias, const int* ncls,
                     const e2_tensor5* const* targets, const e2_tensor5* const* probs,
                     float* stats);
size_t e2_multihead_bwd_workspace_bytes(int n, int cin, int sum_ncls, int d, int h, int w);
int e2_multihead_bwd(e2_ctx*, const e2_tensor5* x, int k, const float* const* w,
                     const e2_tensor5* const* probs, const e2_tensor5* const* targets,
                     const float* coef, const e2_tensor5* dx, int accumulate_dx,
                     float* const* dw, float* const* dbias, void* ws, size_t ws_bytes);

/* ---- weighted MultinoulliNLL: class / example weights and the lazy-labelling masks
 *      (loss.py:172-212 arguments, loss.py:261-347 computation; n_indep = 1, sparse targets,
 *      weakness = 0).  With t = target class id (< 0: unlabelled), w = class_w, e = example_w,
 *      L = labelled (mask_class_labeled), M = not_present (mask_class_not_present), S = positions
 *      per batch item:
 *        T[b,c,v] = [t[b,v] == c] * L[b,c]
 *        stats[0] = - sum T w e log(p + 1e-5)  -  sum_{ALL voxels} M w e log((1 - p) + 1e-5)
 *        stats[1] = sum T + S * sum M           (a count: the weights do not enter it)
 *        loss     = stats[0] / (stats[1] + 1e-5)
 *        dloss/dp = (-T w e / (p + 1e-5) + M w e / ((1 - p) + 1e-5)) / (stats[1] + 1e-5)
 *      1 - p_c is formed as the sum of the OTHER classes' terms, never by subtraction (f32
 *      loses every digit of it where a not-present class saturates).  NULL members take their
 *      default; all members NULL, or a NULL descriptor, is the unweighted loss.  The arrays are
 *      device memory, read at launch time (a captured graph follows their contents).  The _w
 *      entry points take the arguments of their unweighted siblings and honour
 *      e2_set_loss_grad_mode the same way (count_out = stats[1]).  e2_tail_fwd_bwd_w is f32
 *      only: in bf16 mode (e2_set_mfma_dtype) it is an error -- use the head / conv entry points. ----------------------- */
typedef struct e2_nll_weights {
  const float*      class_w;      /* [ncls]                                  NULL: 1 */
  const e2_tensor5* example_w;    /* (n, 1, d, h, w), spatial = the target's NULL: 1 */
  const float*      labelled;     /* [n][ncls]  mask_class_labeled           NULL: 1 */
  const float*      not_present;  /* [n][ncls]  mask_class_not_present       NULL: 0 */
} e2_nll_weights;
int e2_softmax_nll_fwd_w(e2_ctx*, const e2_tensor5* logits, const e2_tensor5* target,
                         const e2_tensor5* probs, float* stats, const e2_nll_weights* wts);
/* (dlogits must not alias probs: the weighted backward keeps partial sums in dlogits while it
 * still reads the probabilities -- the unweighted one has no such restriction) */
int e2_softmax_nll_bwd_w(e2_ctx*, const e2_tensor5* probs, const e2_tensor5* target,
                         const float* stats, const e2_tensor5* dlogits, float* loss_out,
                         const e2_nll_weights* wts);
int e2_head_fwd_w(e2_ctx*, const e2_tensor5* x, const float* w, const float* bias, int ncls,
                  const e2_tensor5* target, const e2_tensor5* probs, float* stats,
                  const e2_nll_weights* wts);
int e2_head_bwd_w(e2_ctx*, const e2_tensor5* x, const float* w, const e2_tensor5* probs,
                  const e2_tensor5* target, const float* stats, const e2_tensor5* dx,
                  int accumulate_dx, float* dw, float* dbias, float* loss_out, void* ws,
                  size_t ws_bytes, const e2_nll_weights* wts);
int e2_tail_fwd_bwd_w(e2_ctx*, const e2_tensor5* x, const float* wp_fwd, const float* wp_dgrad,
                      const float* bias1, int c2, const float* w_head, const float* b_head,
                      int ncls, const e2_tensor5* target, const e2_tensor5* probs,
                      const e2_tensor5* dpre, const e2_tensor5* dx, int gm_mode,
                      const e2_tensor5* gm_src, const float* gm_bias, float* stats, void* ws,
                      size_t ws_bytes, int* n_slots, const e2_nll_weights* wts);

/* MALIS NLL (neuromancer/loss.py:560-690 MalisNLL; malis/malisop.py:19-123): probs is
 * (1, 2E, d, h, w) -- E independent 2-class softmaxes, channel 2e = "disconnected",
 * 2e+1 = affinity of edge e; pos / neg: dense (E, d, h, w) float MALIS counts (from
 * e2_malis_loss_weights, constants for the gradient); norm[0] = 1/(n_tot + 1e-5) on
 * the device.  loss_sum[0] += -sum(pos*log(p_aff+1e-5) + neg*log(p_dis+1e-5))*norm[0]
 * (terms with a zero count contribute 0: xlogy0, loss.py:26-28); dlogits (nullable):
 * d(loss)/d(logits) through the pair softmax, same shape as probs. */
int e2_malis_nll(e2_ctx*, const e2_tensor5* probs, const float* pos, const float* neg,
                 const float* norm, const e2_tensor5* dlogits, float* loss_sum);

/* ---- optimiser (optimiser.py:273-334 Adam; 135-165 SGD) on one flat
 *      parameter arena.  wd_mult[i] = weight-decay multiplier per element
 *      segment is given by seg tables: for segment s, elements
 *      [seg_off[s], seg_off[s+1]) use decay multiplier seg_reg[s]. --------- */
/* hyper: 8 device floats {lr, mom, beta2, wd, t, factor, -, arrival counter}.  The
 * kernel reads t, steps with t + 1 (bias factor sqrt(1-beta2^t)/(1-mom^t)) and stores
 * the new t for the next call; hyper[7] must be zero before the first call; all four
 * arenas 16-byte aligned, n_seg <= 1024. */
int e2_adam_step(e2_ctx*, float* p, const float* g, float* m, float* s,
                 size_t n, const int64_t* seg_off, const float* seg_reg,
                 int n_seg, const float* hyper /* device: lr,mom,beta2,wd,t,.. */);
int e2_sgd_step(e2_ctx*, float* p, const float* g, float* d, size_t n,
                const int64_t* seg_off, const float* seg_reg, int n_seg,
                const float* hyper /* device: lr,mom,_,wd,_ */);

/* Data-parallel normalisation: the reference divides the NLL by the labelled voxels of the
 * WHOLE batch (loss.py:342-344).  With sum_mode != 0 the NLL backward launches that follow
 * (e2_tail_fwd_bwd, e2_head_bwd, e2_softmax_nll_bwd) leave the gradient UNNORMALISED -- loss
 * values are unaffected -- and e2_tail_reduce / e2_head_bwd / e2_softmax_nll_bwd also write this
 * rank's labelled count to count_out (a slot behind the gradient arena, so that it rides in
 * the same all-reduce); sum-all-reduce + e2_adam_step_ex(gdiv = the summed count) then IS the
 * whole-batch gradient, with no elementwise launch around the collective.  (0, NULL) restores
 * the per-rank normalisation. */
int e2_set_loss_grad_mode(e2_ctx*, int sum_mode, float* count_out);

/* the same with the gradient scaled on the way in and the arena cleared on the way out:
 * the update sees g * gmul / (gdiv ? gdiv[0] + 1e-5 : 1); zero_g != 0 leaves g ZERO for the
 * next backward pass (no fill launch).  gdiv: device scalar -- the data-parallel step sums
 * unnormalised gradients (and the labelled-voxel counts, in a slot behind the arena) over the
 * ranks and divides here, which is the reference's whole-batch normalisation
 * (loss.py:342-344) without elementwise launches around the collective. */
int e2_adam_step_ex(e2_ctx*, float* p, float* g, float* m, float* s, size_t n,
                    const int64_t* seg_off, const float* seg_reg, int n_seg,
                    const float* hyper, const float* gdiv, float gmul, int zero_g);
int e2_sgd_step_ex(e2_ctx*, float* p, float* g, float* d, size_t n, const int64_t* seg_off,
                   const float* seg_reg, int n_seg, const float* hyper, const float* gdiv,
                   float gmul, int zero_g);

/* AdaGrad (optimiser.py:168-214) and AdaDelta (optimiser.py:222-264) on the same arena, segment
 * tables, hyper array ({lr, mom, -, wd, t, -, -, arrival counter}) and gdiv / gmul / zero_g as
 * the two above; all arithmetic float32, g' = the scaled gradient.
 *   AdaGrad:  c = (t == 0) ? 2 : 1;  h' = h + c g'^2;  p' = p - lr / sqrt(h') (g' + wd r p);
 *     t' = t + 1.  c: the reference's first call runs init_func (h += g^2 from one gradient
 *     evaluation of the same batch) and then the step, which adds g^2 again (optimiser.py:
 *     200-214); with the same batch and parameters both gradients are the same, so the first
 *     step sees h = 2 g^2 -- one launch here, no second forward / backward pass.  (With dropout
 *     the reference draws different gates in its two evaluations; here the step's own gradient
 *     counts twice.)  r = 1 where the segment's multiplier is not 0, else 0: optimiser.py:187-189
 *     has no apply_reg > 1 branch, so a multiplier of 3 decays like 1 under AdaGrad.  t lives in
 *     hyper[4] as Adam's does; hyper[7] must be zero before the first call; hyper[5] is left
 *     alone.  THE ONE DEPARTURE from the reference: where h' == 0 -- every gradient of the
 *     element exactly zero since the start: a dead unit, a feature that never fired -- the
 *     reference divides by sqrt(0) and writes NaN or +-inf into the parameter; here the element
 *     is left unchanged and h stays 0.
 *   AdaDelta: eps = 1e-5;  s' = mom s + (1 - mom) g'^2;  dir = g' sqrt(d + eps) / sqrt(s + eps)
 *     with the OLD s and the OLD d, as the reference has it (optimiser.py:243-245);
 *     d' = mom d + (1 - mom) dir^2;  p' = p - lr (dir + wd mult p), mult = the segment's
 *     multiplier as in SGD.  No step counter: hyper is only read.
 * Refusals as above (a NULL argument, n_seg outside 1..1024, an arena off its 16-byte
 * boundary): nothing is written. */
int e2_adagrad_step_ex(e2_ctx*, float* p, float* g, float* h, size_t n, const int64_t* seg_off,
                       const float* seg_reg, int n_seg, const float* hyper,
                       const float* gdiv, float gmul, int zero_g);
int e2_adadelta_step_ex(e2_ctx*, float* p, float* g, float* s, float* d, size_t n,
                        const int64_t* seg_off, const float* seg_reg, int n_seg,
                        const float* hyper, const float* gdiv, float gmul, int zero_g);

/* The Adam update of optimiser.py:301-329 that also WRITES the packed weight images of every
 * conv (what e2_conv3d_pack_multi does at the head of a step): a work-group owns a tile of one
 * weight tensor -- 32 output channels x IC input channels x the taps of one kernel plane --,
 * updates it (arithmetic and order of e2_adam_step_ex: bit-identical p / m / s), and writes the
 * new values from LDS as the tile of the forward image and of the data-gradient image, each along
 * its contiguous axis, zeros in the fetched padding exactly where e2_conv3d_pack_multi writes them.
 * One launch instead of two, the weights read once (csrc/update_pack.hip).
 *   e2_upd_job_fill: one record per conv weight tensor w[cout][cin][kd][kh][kw] at element offset
 *     `off` of the arenas; wp_f / wp_d = its e2_conv3d_pack images of mode 0 / 1 (either may be
 *     NULL); reg = weight-decay multiplier (0 = none); tile0 = tiles of the records before it;
 *     *ntiles = this record's tiles, *lds_bytes = LDS a launch holding it needs.
 *   e2_upd_rest_fill: a run of `n` elements at `off` without images (biases, first layer, head,
 *     UpConv): the plain update.
 *   e2_adam_pack_step: jobs_dev / rest_dev = device arrays of those records; every trainable
 *     element must be covered exactly once by the two lists (caller's contract); lds_bytes = the
 *     largest *lds_bytes; hyper / gdiv / gmul / zero_g as e2_adam_step_ex, except that hyper
 *     holds 24 floats here ([8..23]: arrival counters, zero before the first launch). */
size_t e2_upd_job_bytes(void);
size_t e2_upd_rest_bytes(void);
int e2_upd_job_fill(void* rec, long off, void* wp_f, void* wp_d, int cout, int cin, int kd, int kh,
                    int kw, float reg, int tile0, int* ntiles, size_t* lds_bytes);
int e2_upd_rest_fill(void* rec, long off, long n, float reg);
int e2_adam_pack_step(e2_ctx*, float* p, float* g, float* m, float* s, const void* jobs_dev,
                      int njobs, int ntiles, const void* rest_dev, int nrest, float* hyper,
                      const float* gdiv, float gmul, int zero_g, size_t lds_bytes);

/* ---- step capture (replaces theano.function, graphutils.py:376-387) ---- */
typedef struct e2_graph e2_graph;
int e2_graph_begin(e2_ctx*);                 /* hipStreamBeginCapture      */
int e2_graph_end(e2_ctx*, e2_graph** out);   /* EndCapture + Instantiate   */
int e2_graph_launch(e2_ctx*, e2_graph*);     /* hipGraphLaunch on the stream*/
int e2_graph_destroy(e2_graph*);
/* the captured graph as a GraphViz file (hipGraphDebugDotPrint; verbose: with the kernels' names) --
 * how the fork / join structure of a plan with a side stream was looked at (DESIGN finding 54) */
int e2_graph_debug_dot(e2_graph*, const char* path, int verbose);

/* ---- timing helpers (HIP events on the context's stream) -------------- */
/* ---- patch extraction with warp + grey augmentation on the device (SURVEY 8f-1;
 *      data/transformations.py:337-492, :42-76; data/cnndata.py:42-60).
 *      dst[f][z][x][y] = interp(src[f], Minv . (z + dest_off[0], x + dest_off[1],
 *      y + dest_off[2], 1) - src_off): trilinear, or nearest (np.round) for the
 *      channels whose bit is set in nearest_mask.  src: (1, F <= 32, Z, X, Y) view of
 *      the resident volume; dst: dense (1, F, pz, px, py); Minv, dest_off (3 ints),
 *      src_off (3 floats) in HOST memory (NULL offsets = 0).  The caller checks the
 *      patch corners against the volume first (WarpingOOBError on the host side). */
int e2_warp_slice(e2_ctx*, const e2_tensor5* src, const float* minv, int perspective,
                  unsigned nearest_mask, const int* dest_off, const float* src_off,
                  const e2_tensor5* dst);
/* d = clip(d * alpha + c, 0, 1) ** gamma on one dense channel of n floats, in place */
int e2_grey_augment(e2_ctx*, float* d, size_t n, float alpha, float c, float gamma);

/* ---- target forms of the batch creator, on the device (targets.hip; data/cnndata.py:319-396,
 *      data/image.py:80-102, :138-220).  t = full-resolution target patches (n, C, D, H, W);
 *      stride = (sz, sx, sy) >= 1 and nhood = E x 3 displacements (E <= 64) in HOST memory;
 *      ts[n,c,z,x,y] = t[n,c,z sz,x sx,y sy] with extents ceil(D/sz), ...; all views arbitrary
 *      (unit w stride), nothing outside them is read or written; one launch each.
 * e2_target_stride:   dst (n, C, d, h, w) = ts, NaN -> -666.
 * e2_target_nhood:    dst (n, E + C - 1, d, h, w): channel e < E = t[n, 0, p s - nhood[e]], -1 where
 *                     that lies outside (D, H, W) (the shift acts on the full-resolution patch, then
 *                     the stride); channels E.. = ts[:, 1:]; NaN -> -666.  |nhood[e][k]| must be
 *                     smaller than the extent of axis k.
 * e2_target_affinity: dst (n, E, d, h, w) = 1 where p + nhood[e] lies inside (d, h, w) and
 *                     a = rint(ts[n,0,p]), b = rint(ts[n,0,p + nhood[e]]) are equal and both > 0,
 *                     else 0 (NaN, zero and negative ids connect to nothing):
 *                     malis.seg_to_affgraph of the rounded strided ids.
 * e2_count_negative:  count[0] += #{t < 0} over the view (NaN is not negative); count: one
 *                     unsigned in DEVICE memory that the caller zeroes; integer atomics.
 * e2_ids2barriers:    ids, dst (1, 1, D, H, W): the 0 / 1 (/ 2) barrier volume of ids2barriers with
 *                     smoothen=False -- the reference's forward pass and its pass over the reversed
 *                     volume, edge behaviour included -- written as a gather (no atomics, bit-
 *                     reproducible).  dilute / connectivity: 3 ints each in HOST memory; ecs_mode:
 *                     0 none, 1 max(ids == 0, barriers), 2 'new_class' (ids == 0 and no barrier -> 2). */
int e2_target_stride(e2_ctx*, const e2_tensor5* t, const int* stride, const e2_tensor5* dst);
int e2_target_nhood(e2_ctx*, const e2_tensor5* t, const int* nhood, int E, const int* stride,
                    const e2_tensor5* dst);
int e2_target_affinity(e2_ctx*, const e2_tensor5* t, const int* nhood, int E, const int* stride,
                       const e2_tensor5* dst);
int e2_count_negative(e2_ctx*, const e2_tensor5* t, unsigned* count);
int e2_ids2barriers(e2_ctx*, const e2_tensor5* ids, const int* dilute, const int* connectivity,
                    int ecs_mode, const e2_tensor5* dst);

/* ---- MALIS (host code, no GPU involved; malis/_malis_lib.cpp:38-167 via
 *      malis/_malis.pyx:42-123).  e2_malis_loss_weights: counts[e] = number of voxel
 *      pairs whose maximin edge in the affinity graph is e and whose ground-truth ids are
 *      equal (pos != 0) or different (pos == 0); seg ids 0 = unlabelled; node indices out
 *      of [0, n_vert) mark absent edges.  e2_malis_connected_components: seg[v] = 1 +
 *      representative under edges with |weight| > 1e-5, components of <= size_thresh
 *      voxels -> 0.  Return 0 on success, 2 on bad arguments. ------------------------- */
int e2_malis_loss_weights(int n_vert, const int32_t* seg, int n_edge, const int32_t* node1,
                          const int32_t* node2, const float* edge_weight, int pos,
                          uint64_t* counts);
int e2_malis_connected_components(int n_vert, int n_edge, const int32_t* node1,
                                  const int32_t* node2, const float* edge_weight,
                                  int size_thresh, int32_t* seg);

typedef struct e2_event e2_event;
int e2_event_create(e2_event** out);
int e2_event_record(e2_ctx*, e2_event*);
int e2_event_elapsed_ms(e2_event* start, e2_event* stop, float* ms); /* syncs stop */
int e2_event_destroy(e2_event*);
int e2_stream_synchronize(e2_ctx*);
/* Second stream for independent work (wgrad of a layer next to the dgrad chain):
 * fork = `side` waits for everything issued on the context's stream so far;
 * join = the context's stream waits for everything issued on `side`.  Both work
 * while the context's stream is being captured (the side stream becomes a parallel
 * branch of the graph; join it before e2_graph_end).  Launch on the side stream by
 * pointing the context at it with e2_ctx_set_stream and back. */
int e2_stream_fork(e2_ctx*, void* side_stream);
int e2_stream_join(e2_ctx*, void* side_stream);

/* ---- conv forward / data gradient with bf16 operands in memory ----------
 * Same arithmetic as E2_MFMA_BF16 (operands rounded to bf16, nearest even; f32 products and
 * sums; f32 tensors in and out) on a kernel built for v_mfma_f32_32x32x16_bf16: the call
 * converts its input to bf16 planes of 16-byte pixels (8 channels each) and the canonical
 * weights w (n_f, n_in, kd, kh, kw) to bf16 filter rows in the caller's workspace
 * (e2_conv3d_bf16_workspace_bytes for the layer: covers both directions); the GEMM stages a
 * work-group's input window in LDS once per kernel plane (LDS-DMA) and reads every tap from
 * it at a shifted pixel, filter rows come from L2.  fwd: optional fused bias + activation
 * (bias NULL: plain conv), out any strided view.  dgrad: dy_pad zero-padded as for
 * e2_conv3d_dgrad.  All reduction channels of one kernel plane must fit LDS (an error says
 * so; the operand-rounding form of E2_MFMA_BF16 has no such limit).  Tiling:
 * e2_set_tiling(E2_TILING_IGEMM, "32,MB,NB") = MB x NB blocks of 32 channels x 32 positions
 * per wave (default 2 x 2).  No reference counterpart (the reference is f32). */
size_t e2_conv3d_bf16_workspace_bytes(int n, int cin, int d, int h, int w, int cout, int kd,
                                      int kh, int kw);
int e2_conv3d_fwd_bf16(e2_ctx*, const e2_tensor5* x, const float* w, int cout, int kd, int kh,
                       int kw, const float* bias, int act, const e2_tensor5* out, void* ws,
                       size_t ws_bytes);
int e2_conv3d_dgrad_bf16(e2_ctx*, const e2_tensor5* dy_pad, const float* w, int cin, int kd,
                         int kh, int kw, const e2_tensor5* dx, void* ws, size_t ws_bytes);
/* The weight gradient in the same arithmetic (operands rounded to bf16, f32 sums), K = the
 * positions: dy (the UNPADDED gradient view, any strides) is converted to bf16 channel-major
 * planes at the input's row pitch, x to bf16 channels-last pixels, both staged in LDS per
 * 64 positions; dy rows are read with ds_read_b128, the shifted input windows with the
 * transposed LDS read ds_read_b64_tr_b16; the tile is flushed into dw with f32 atomics
 * (accumulate 0: dw is zeroed first).  Tiling: e2_set_tiling(E2_TILING_WGRAD,
 * "32,MB,NB,R,S"): MB (1..2) blocks of 32 out channels x NB (1..4) taps of a kernel row per
 * wave; R = 0: the work-group spans 128 input channels of one kernel row, R = 1: 32 input
 * channels of four kernel rows; S position splits (0 = one work-group per CU). */
size_t e2_conv3d_wgrad_bf16_workspace_bytes(int n, int cin, int d, int h, int w, int cout,
                                            int kd, int kh, int kw);
int e2_conv3d_wgrad_bf16(e2_ctx*, const e2_tensor5* x, const e2_tensor5* dy, float* dw, int kd,
                         int kh, int kw, int accumulate, void* ws, size_t ws_bytes);
/* One conversion less per layer and step: e2_conv3d_fwd_bf16_keep writes the bf16
 * channels-last copy of its input into a buffer of the caller's (e2_conv3d_bf16_xkeep_bytes,
 * zero-filled ONCE by the caller: the pixels behind the last plane stay zero) instead of the
 * shared workspace, and e2_conv3d_wgrad_bf16_xcl reads that copy (kg_per_plane = channel
 * groups of 8 per plane in it = ceil(cin / 16) * 2; x_shape: the input's extents, its
 * pointer and strides are not used) instead of converting x again. */
size_t e2_conv3d_bf16_xkeep_bytes(int n, int cin, int d, int h, int w, int kh, int kw);
int e2_conv3d_fwd_bf16_keep(e2_ctx*, const e2_tensor5* x, const float* w, int cout, int kd,
                            int kh, int kw, const float* bias, int act, const e2_tensor5* out,
                            void* ws, size_t ws_bytes, void* xkeep, size_t xkeep_bytes);
int e2_conv3d_wgrad_bf16_xcl(e2_ctx*, const e2_tensor5* x_shape, const void* xcl,
                             int kg_per_plane, const e2_tensor5* dy, float* dw, int kd, int kh,
                             int kw, int accumulate, void* ws, size_t ws_bytes);

/* ---- the producers' epilogues ---------------------------------------------
 * No conversion pass at all: the bf16 operand images of a GEMM are written by the kernel that
 * produces the tensor, the filter rows of every layer by ONE launch at the start of the step,
 * and the GEMM entry points take them ready-made.  Reference seam unchanged: the tensors are
 * those of neural.py:662-712 (conv -> pool -> bias -> activation) and of T.grad of that chain
 * (model.py:182); only WHERE their bf16 copies are made moves.
 *
 * e2_bf16_dst: where a producer puts the bf16 copies of the tensor it writes.
 *   cl  channels-last image [n][cl_d][cl_kg][cl_h][cl_w][8] (16-byte pixel pieces of 8 channels,
 *       cl_kg * 8 >= channels; the layout conv_bf16 / wgrad_bf16 read); element (z, y, x) of the
 *       tensor lands at (z + cl_oz, y + cl_oy, x + cl_ox) -- the interior of a zero-padded
 *       gradient image.  Everything the producer does not write (border, padding channel
 *       groups, slack) must be zero from a one-time fill.
 *   pl  channel-major planes [n][c][d][pl_plane] with row pitch pl_pitch (the dy operand of
 *       e2_conv3d_wgrad_bf16_ex: pl_pitch = the layer INPUT's row length, pl_plane from
 *       e2_conv3d_wgrad_bf16_geometry); gaps stay zero from a one-time fill.
 * Either may be NULL. */
typedef struct e2_bf16_dst {
  void* cl;
  int cl_kg, cl_d, cl_h, cl_w;
  int cl_oz, cl_oy, cl_ox;
  void* pl;
  int64_t pl_plane;
  int pl_pitch;
} e2_bf16_dst;
/* e2_pool_bias_act_bwd (bias != NULL: src = the conv output y, slope from max + bias) and
 * e2_bias_act_bwd_out (bias == NULL, window (1,1,1): src = the activated output, slope from its
 * signed zeros) with dout as `parts` partial sums part_stride apart; writes dy (f32; dy == NULL
 * or dy->ptr == NULL: not written), dbias += row sums (NULL: skipped) and the bf16 copies named
 * by dst.  relu / lin; windows (1,1,1), (1,2,2), (2,1,1), (2,2,2). */
int e2_pool_bias_act_bwd_bf16(e2_ctx*, const e2_tensor5* dout, int64_t part_stride, int parts,
                              const e2_tensor5* src, const float* bias, int pz, int py, int px,
                              int act, const e2_tensor5* dy, float* dbias, const e2_bf16_dst* dst);
/* e2_pool_bias_act_fwd_parts writing out (f32; out->ptr == NULL: not written) and the
 * channels-last bf16 copy of out (dst->cl: the NEXT conv layer's kept input copy). */
int e2_pool_bias_act_fwd_bf16(e2_ctx*, const e2_tensor5* y, int64_t part_stride, int parts,
                              const float* bias, int pz, int py, int px, int act,
                              const e2_tensor5* out, const e2_bf16_dst* dst);
/* e2_conv1_pool_act_fwd writing also the channels-last bf16 copy of out (cout <= 32) */
int e2_conv1_pool_act_fwd_bf16(e2_ctx*, const e2_tensor5* x, const float* w, const float* bias,
                               int cout, int kh, int kw, int py, int px, int act,
                               const e2_tensor5* out, void* next_xb, int next_kg);
/* The filter rows of a launch, packed ahead of it for the tile "32,mb,nb" (mode 0: forward
 * image of w (nf, nin, kd, kh, kw), rows = nf; mode 1: data-gradient image, rows = nin); in_w /
 * out_w: the row lengths of the GEMM's input and output (forward: x and y; data gradient: the
 * padded dy and dx).  Jobs are plain records (e2_bf16_wjob_bytes each) filled on the host,
 * copied to the device by the caller and run by ONE launch. */
size_t e2_conv3d_bf16_wb_bytes(int rows, int kk, int kd, int kh, int kw, int in_w, int out_w,
                               int mb, int nb);
size_t e2_bf16_wjob_bytes(void);
int e2_bf16_wjob_fill(void* rec, const float* w, int nf, int nin, int kd, int kh, int kw, int mode,
                      int in_w, int out_w, int mb, int nb, void* wb, size_t wb_bytes);
int e2_conv3d_bf16_pack_w_multi(e2_ctx*, const void* jobs_dev, int njobs);
/* e2_conv3d_fwd_bf16_keep / e2_conv3d_dgrad_bf16 with ready-made operands: x_ready != 0: xkeep
 * already holds this step's copy of x (x->ptr may be NULL); wb != NULL: the packed filter rows
 * (w may be NULL; the forced tile must be the one they were packed for); next_xb != NULL
 * (forward): the channels-last bf16 copy of out, [n][d][next_kg][h * w][8] with next_kg =
 * ceil(cout / 16) * 2, is written by the epilogue (padding channels as zeros).  dy_cl: the
 * channels-last image of the padded gradient (dy_pad gives the shape).  With every operand
 * ready ws may be NULL. */
int e2_conv3d_fwd_bf16_ex(e2_ctx*, const e2_tensor5* x, const float* w, int cout, int kd, int kh,
                          int kw, const float* bias, int act, const e2_tensor5* out, void* ws,
                          size_t ws_bytes, void* xkeep, size_t xkeep_bytes, int x_ready,
                          const void* wb, void* next_xb, int next_kg);
int e2_conv3d_dgrad_bf16_ex(e2_ctx*, const e2_tensor5* dy_pad, const float* w, int cin, int kd,
                            int kh, int kw, const e2_tensor5* dx, void* ws, size_t ws_bytes,
                            const void* dy_cl, const void* wb);
/* e2_conv3d_wgrad_bf16_xcl with dy as ready-made planes (dyc: e2_bf16_dst.pl of the kernel that
 * produced dy; dy gives the shape) and the f32 sums in a buffer of the caller's (sums:
 * sums_bytes of e2_conv3d_wgrad_bf16_geometry, zero-filled ONCE -- the call leaves it zero);
 * xcl, dyc, sums may each be NULL (then made / held in ws as before). */
int e2_conv3d_wgrad_bf16_geometry(int n, int cin, int d, int h, int w, int cout, int kd, int kh,
                                  int kw, int64_t* plane_d, size_t* dyc_bytes, size_t* sums_bytes);
int e2_conv3d_wgrad_bf16_ex(e2_ctx*, const e2_tensor5* x_shape, const void* xcl, int kg_per_plane,
                            const e2_tensor5* dy, const void* dyc, float* sums, float* dw, int kd,
                            int kh, int kw, int accumulate, void* ws, size_t ws_bytes);

/* ---- BASELINE config 1 (examples/mnist.py:29-56): Perceptron and batch normalisation ----
 * Correctness-first kernels for the reference's CPU-runnable plumbing case.
 *
 * Perceptron (neural.py:258-410, computations.py:179-213 `dot`): plain row-major matrices,
 *   y (n x m) = x (n x k) . w (k x m)              w has the reference's (n_in, n_f) layout
 *   dx (n x k) (+)= dy (n x m) . w^T               accumulate: 0 overwrite, 1 add
 *   dw (k x m) (+)= x^T . dy
 * bias / activation of a Perceptron without batch norm: e2_pool_bias_act_fwd / _bwd with a
 * (1,1,1) window on the (n, m, 1, 1, 1) view. */
int e2_dense_fwd(e2_ctx*, const float* x, const float* w, float* y, int n, int k, int m);
int e2_dense_dgrad(e2_ctx*, const float* dy, const float* w, float* dx, int n, int k, int m,
                   int accumulate);
int e2_dense_wgrad(e2_ctx*, const float* x, const float* dy, float* dw, int n, int k, int m,
                   int accumulate);
/* Batch normalisation + bias + activation (neural.py:352-378 Perceptron, 681-711 Conv; applied
 * to the pooled conv output / the dot product):
 *   train != 0: mean, std = statistics of x over every axis but the channel (population std,
 *               + 1e-6); update_running != 0 additionally performs the training function's
 *               extra updates  run_mean <- 0.9995 run_mean + 0.0005 mean  (same for run_std)
 *   train == 0: mean, std = run_mean, run_std ('predict' mode)
 *   out = act((gamma / std) * x + bias - gamma * mean / std)
 * save (2 * c floats, may be NULL in forward-only use) receives the mean and std used.
 * Backward: dx (may be NULL), dgamma += , dbias += (either may be NULL); in train mode the
 * gradient flows through the batch statistics (as T.grad does), in predict mode they are
 * constants.  relu'(0) = 0.5. */
int e2_batchnorm_act_fwd(e2_ctx*, const e2_tensor5* x, const float* gamma, const float* bias,
                         float* run_mean, float* run_std, int train, int update_running,
                         int act, const e2_tensor5* out, float* save);
int e2_batchnorm_act_bwd(e2_ctx*, const e2_tensor5* dout, const e2_tensor5* x,
                         const float* gamma, const float* bias, const float* save, int train,
                         int act, const e2_tensor5* dx, float* dgamma, float* dbias);

/* ---- dropout (neural.py:246-249 the rate parameter; 391-397 Perceptron: one gate per output
 *      feature; 714-720 Conv and 1064-1070 UpConv: one gate per output element; the last thing a
 *      node does to its output) ---------------------------------------------------
 * The reference draws Bernoulli(1 - rate) gates from Theano's MRG stream, seeded with the wall
 * clock, multiplies the activated output by gate / (1 - rate) and lets T.grad send the output
 * gradient through the same product.  Here the gate is a pure function of (seed, counter, stream,
 * element index) -- Philox4x32-10 (Salmon et al. 2011: multipliers 0xD2511F53 / 0xCD9E8D57, key
 * increments 0x9E3779B9 / 0xBB67AE85) -- so that the backward pass REGENERATES it; no mask is
 * ever stored.  The contract (tests restate it in NumPy):
 *
 *   j     = gate index of the element (64-bit): its row-major index in the LOGICAL dense shape
 *           (n, c, d, h, w) of the view in element mode; its feature index c in feature mode
 *   word  = philox4x32_10(ctr = (lo32(j >> 2), hi32(j >> 2), stream, counter),
 *                         key = (lo32(seed), hi32(seed)))[j & 3]
 *   T     = rate >= 1 ? 0xffffffff : (uint32)(rate * 4294967296.0f)        (exact: a power of two)
 *   keep  = word >= T ;  scale = 1.0f / (1.0f - rate) ;  out = keep ? x * scale : 0
 *
 * j depends on the logical shape alone: never on strides, tiling or launch geometry.  rate = 0
 * gives T = 0, scale = 1: a bit-exact copy.
 *   rate   one float in DEVICE memory, read when the kernel runs (a captured launch follows later
 *          changes of the rate)
 *   state  four 32-bit words in DEVICE memory, 16-byte aligned, owned by the caller:
 *          [0] lo32(seed), [1] hi32(seed), [2] counter, [3] unused; read when the kernel runs
 *   stream a launch argument: tells the dropout nodes of one model (and the ranks of a
 *          data-parallel group) apart
 * e2_dropout_fwd: out = gate(x); e2_dropout_bwd: dx = gate(dout), the same gate for the same
 * (state, stream).  The two views of a call have identical sizes and may be the same (in place);
 * otherwise they must not overlap.  One thread makes one Philox block = four consecutive j and
 * moves them with one 16-byte access where they lie in one 16-byte aligned row piece.
 * e2_dropout_tick: state[2] += 1 (one tiny launch).  A step issues it once, in front of all its
 * dropout launches, which then read the counter it left: every replay of a captured step draws
 * new gates, forward and backward of one step draw the same. */
int e2_dropout_fwd(e2_ctx*, const e2_tensor5* x, const e2_tensor5* out, int feature_mode,
                   const float* rate, const void* state, uint32_t stream);
int e2_dropout_bwd(e2_ctx*, const e2_tensor5* dout, const e2_tensor5* dx, int feature_mode,
                   const float* rate, const void* state, uint32_t stream);
int e2_dropout_tick(e2_ctx*, void* state);

/* ---- bias + activation as an op of its own (computations.py:57-134 apply_activation, called
 *      from neural.py:389 Perceptron, :712 Conv, :1062 UpConv) -------------------------------
 * All eight E2_ACT_* values, on strided views of identical sizes; v = pre + bias[c]:
 *
 *   act       f(v)                                  f'(v)
 *   LIN       v                                     1
 *   RELU      max(v, 0)                             v > 0 ? 1 : (v == 0 ? 0.5 : 0)
 *   TANH      tanh v                                1 - tanh^2 v
 *   SIGMOID   1 / (1 + e^-v)                        f (1 - f)
 *   ABS       |v|                                   sgn v, 0 at v = 0
 *   ELU       v > 0 ? v : expm1 v                   v > 0 ? 1 : e^v
 *   SELU      s (v > 0 ? v : a expm1 v)             v > 0 ? s : s a e^v
 *             a = 1.6732632423543772..., s = 1.0507009873554804... (computations.py:96-98)
 *   SOFTPLUS  log(1 + e^v)                          sigmoid v
 *
 * The slopes at v = 0 follow the reading of Theano that gives relu'(0) = 0.5 (T.nnet.relu =
 * 0.5 (v + |v|), sgn 0 = 0): abs'(0) = 0; switch(v > 0, ..) takes its second branch at 0, so
 * elu'(0) = 1 and selu'(0) = s a.  f32 arithmetic in forms that are finite for every finite v.
 * Nodes with relu / lin do not use this pair (their activation is fused into the pooling
 * kernels and GEMM epilogues); both values are accepted so that the op is complete. */
/* out = f(pre + bias[c]);  bias may be NULL;  out may alias pre (computations.py:57-134) */
int e2_act_fwd(e2_ctx*, const e2_tensor5* pre, const float* bias, int act, const e2_tensor5* out);
/* dpre = dout * f'(pre + bias[c]);  dbias[c] += sum over n,z,y,x of dpre (NULL: not wanted; the
 * caller zeroes it);  dpre may alias dout (T.grad of computations.py:57-134) */
int e2_act_bwd(e2_ctx*, const e2_tensor5* dout, const e2_tensor5* pre, const float* bias, int act,
               const e2_tensor5* dpre, float* dbias);

/* ---- element-wise losses and their mix (loss.py:829-887 GaussianNLL, 953-1011 BinaryNLL,
 *      1014-1101 SquaredLoss, 1215-1276 AbsLoss, 1346-1363 AggregateLoss) -------------------------
 * p prediction, t target of the same sizes, d = t - p, EPS = 1e-5, n_tot = elements of p.
 * masked = |t + 666| <= 1e-8 + 666e-5 (T.isclose(t, -666.0) with Theano's rtol = 1e-5, atol = 1e-8;
 * NaN is not masked); n_lab = unmasked elements.  The reference multiplies an element-wise array
 * by n_tot / (n_lab + 1) and AggregateLoss takes its mean: n_tot cancels, the array is never made.
 *
 *   kind        element loss l (unmasked elements)                 term value L
 *   SQUARED     0.5 d^2 g c,  g = [|d| >= margin] (1 without),     S1 / (n_lab + 1) - margin S2 / n_tot
 *               c = sc / (|t| + sc) (1 without)                    S1 = sum l, S2 = sum c; second part
 *   ABS         |d| g c,      c = sc |t| + 1                       only with a margin (loss.py:1084-1085)
 *   BINARY_NLL  -xlogy0(t, p + EPS) - xlogy0(1 - t, 1 - p + EPS)   S1 / (n_lab + 1)
 *               [- xlogy0(t, t + EPS) - xlogy0(1 - t, 1 - t + EPS) with subtract_label_entropy]
 *               xlogy0(x, y) = 0 where x == 0, else x log y
 *   GAUSS_NLL   0.5 log(2 pi) + log s + 0.5 ((t - mu) / s)^2       S1 / n_tot  (no mask)
 *               s = exp(sig), log s = sig with sig_is_log
 *
 *   dL/dp: SQUARED -d g c / (n_lab + 1);  ABS -sgn(d) g c / (n_lab + 1), sgn 0 = 0;
 *          BINARY_NLL (-t / (p + EPS) + (1 - t) / (1 - p + EPS)) / (n_lab + 1);  0 where masked;
 *          GAUSS_NLL dmu = -(t - mu) / s^2 / n_tot, dsig = (1 / s - (t - mu)^2 / s^3) / n_tot, or
 *          (1 - (t - mu)^2 / s^2) / n_tot with sig_is_log.
 *   total = (1 / K) sum_k w_k L_k over the K terms of a mix (loss.py:1357-1363).
 *
 * margin / scale_correction / the mixing weights / coef are DEVICE scalars read when the kernels
 * run: a captured launch follows later changes.  All arithmetic is f32 (sums of the mix: double). */
enum { E2_LOSS_SQUARED = 0, E2_LOSS_ABS, E2_LOSS_BINARY_NLL, E2_LOSS_GAUSS_NLL };
#define E2_MAX_LOSS_TERMS 8
typedef struct e2_loss_term {
  int kind;
  const float* margin;            /* device scalar; NULL: none   (SQUARED / ABS)        */
  const float* scale_correction;  /* device scalar; NULL: none   (SQUARED / ABS)        */
  int subtract_label_entropy;     /* BINARY_NLL */
  int sig_is_log;                 /* GAUSS_NLL  */
} e2_loss_term;
/* rows of 4 floats that e2_loss_fwd writes for a prediction of these sizes (one per work-group,
 * at most 1024); depends on the sizes alone.  0: empty / null view */
size_t e2_loss_partials(e2_ctx*, const e2_tensor5* pred);
/* forward sums of one term: partials[row] = (S1, n_lab, S2, 0) of the row's work-group, every row
 * written by a plain store (no zero fill needed, no atomics); partials 16-byte aligned.  sig: the
 * GAUSS_NLL sigma view, NULL otherwise.  (loss.py:877-885, 994-1009, 1075-1094, 1256-1273) */
int e2_loss_fwd(e2_ctx*, const e2_loss_term*, const e2_tensor5* pred, const e2_tensor5* sig,
                const e2_tensor5* target, float* partials);
/* one small launch for k <= E2_MAX_LOSS_TERMS terms: sums each slab in a fixed order (bit-
 * reproducible) and writes term_loss[j] = L_j, count[j] = n_lab_j (n_tot_j for GAUSS_NLL),
 * coef[j] = mix[j] / (k (n_lab_j + 1)) (GAUSS_NLL: mix[j] / (k n_tot_j)) and loss_out[0] = total.
 * terms / partials / rows / n_tot are HOST arrays of k entries; mix, coef, term_loss, count
 * (k floats each) and loss_out are device memory.  (loss.py:1357-1363) */
int e2_loss_mix(e2_ctx*, int k, const e2_loss_term* terms, float* const* partials,
                const size_t* rows, const int64_t* n_tot, const float* mix, float* coef,
                float* term_loss, float* count, float* loss_out);
/* gradient of the mixed total wrt pred (and sig): dpred (=|+=) coef[0] * d(sum l)/dp, accumulate
 * != 0 adds to what the view holds.  coef: the DEVICE scalar e2_loss_mix wrote for this term.
 * dpred or dsig may be NULL (not wanted), not both; dsig is for GAUSS_NLL alone.  Nothing outside
 * the views is written.  (T.grad of the lines above) */
int e2_loss_bwd(e2_ctx*, const e2_loss_term*, const e2_tensor5* pred, const e2_tensor5* sig,
                const e2_tensor5* target, const float* coef, const e2_tensor5* dpred,
                const e2_tensor5* dsig, int accumulate);

/* ---- losses over the feature axis and the mean of a loss map (csrc/loss_map.hip; loss.py:
 *      1104-1151 EuclideanDistance, 1154-1212 RampLoss, 1346-1363 AggregateLoss) -----------------
 * All operands are strided views of the same n, d, h, w; the maps have ONE feature.
 *
 *   op      forward (a map, one feature)                        backward (dm: the map's gradient)
 *   fdist   m = sqrt(sum_f (t - p)^2), a NaN m is stored as 0   dp = -(t - p) / m * dm,  dt = -dp
 *   ramp    m = (1/F) sum_f r,  r = d_low - d_big + margin,     dd_low = dm / F where r >= 0 and r is
 *           r < 0 -> 0, then NaN -> 0                           not NaN, else 0;  dd_big = -dd_low
 *   mean    rows (sum x, elements summed, 0, 0)                 dx = coef[0] in every element
 *
 * The reference masks r < 0 only: the slope of the ramp AT r == 0 is 1.
 * Two departures from the reference's gradient of fdist: where m == 0 (p == t over all features)
 * T.grad gives 0/0 = NaN, here EVERY feature receives an exact 0; where the forward replaced a NaN
 * by 0, likewise an exact 0 in every feature.
 * The mean of a map is a term of e2_loss_mix, which is unchanged by it: e2_mean_fwd writes the slab
 * rows of e2_loss_fwd -- (S1, n, S2, 0) per work-group, plain 16-byte stores, no atomics,
 * e2_loss_partials(x) rows -- and the term is normalised by n_tot (a plain mean, no -666 mask),
 * which is the GAUSS_NLL row of the mix: L = S1 / n_tot, coef = mix / (K n_tot).  The caller hands
 * e2_loss_mix a GAUSS_NLL-kind descriptor for such a term.
 * margin and coef are DEVICE scalars read when the kernels run.  A gradient view may be NULL (not
 * wanted), not both; each has its own accumulate flag (!= 0 adds to what the view holds): in a
 * siamese net both parents are network branches and either may hold another consumer's gradient.
 * Nothing outside a view is read or written.  All arithmetic is f32. */
int e2_fdist_fwd(e2_ctx*, const e2_tensor5* pred, const e2_tensor5* target, const e2_tensor5* out);
int e2_fdist_bwd(e2_ctx*, const e2_tensor5* pred, const e2_tensor5* target, const e2_tensor5* out,
                 const e2_tensor5* dout, const e2_tensor5* dpred, const e2_tensor5* dtarget,
                 int acc_pred, int acc_target);
int e2_ramp_fwd(e2_ctx*, const e2_tensor5* d_low, const e2_tensor5* d_big, const float* margin,
                const e2_tensor5* out);
int e2_ramp_bwd(e2_ctx*, const e2_tensor5* d_low, const e2_tensor5* d_big, const float* margin,
                const e2_tensor5* dout, const e2_tensor5* dd_low, const e2_tensor5* dd_big,
                int acc_low, int acc_big);
/* partials: e2_loss_partials(x) rows of 4 floats, 16-byte aligned, every row written.  The second
 * column (elements summed, which the mix reports as count) is informational: the GAUSS_NLL row
 * normalises by the host's n_tot, and as a float sum the column is exact only below 2^24 elements
 * per row's work-group and 2^53 in the mix's double sum of rows. */
int e2_mean_fwd(e2_ctx*, const e2_tensor5* x, float* partials);
int e2_mean_bwd(e2_ctx*, const float* coef, const e2_tensor5* dx, int accumulate);
/* OneHot (loss.py:96-138): out[n,k,z,y,x] = (target[n,0,z,y,x] == k) ? 1 : 0 as float for k <
 * n_class = the features of out.  The equality is exact: a negative, fractional or NaN id, or
 * one >= n_class, gives a column of zeros.  No gradient. */
int e2_onehot(e2_ctx*, const e2_tensor5* target, int n_class, const e2_tensor5* out);

/* ---- BetaNLL (csrc/loss_elem.hip; loss.py:890-950) ---------------------------------------------
 * m mode, c concentration, x target in [0, 1], all of one size; EPS = 1e-5;
 * a = m (c - 2) + 1, b = (1 - m)(c - 2) + 1:
 *   l = -[lgamma(a + b) - lgamma(a) - lgamma(b) + (a - 1) log(x + EPS) + (b - 1) log(1 - x + EPS)]
 *       + softplus(-c),                     no mask,   L = S1 / n_tot
 *   dl/dm = (c - 2) [psi(a) - psi(b) - log(x + EPS) + log(1 - x + EPS)]
 *   dl/dc = -psi(a + b) + m psi(a) + (1 - m) psi(b) - m log(x + EPS) - (1 - m) log(1 - x + EPS)
 *           - sigmoid(-c)
 * psi (digamma) is an f32 device function of the library: the recurrence up to an argument >= 6,
 * then the asymptotic series.  Domain: c > 2 and 0 < m < 1, so a, b > 1; outside it the kernels
 * follow the formula as far as lgammaf does and guard nothing.
 * The forward writes the slab rows of e2_loss_fwd (e2_loss_partials(mode) rows); the term goes
 * into e2_loss_mix under a GAUSS_NLL-kind descriptor (the same plain mean over n_tot), and the
 * backward reads the coef the mix wrote.  dmode or dconc may be NULL, not both. */
int e2_beta_nll_fwd(e2_ctx*, const e2_tensor5* mode, const e2_tensor5* conc,
                    const e2_tensor5* target, float* partials);
int e2_beta_nll_bwd(e2_ctx*, const e2_tensor5* mode, const e2_tensor5* conc,
                    const e2_tensor5* target, const float* coef, const e2_tensor5* dmode,
                    const e2_tensor5* dconc, int accumulate);

#ifdef __cplusplus
}
#endif
#endif /* E2HIP_H */
