// loss_sobel.hip -- SobelizedLoss (loss.py:1373-1439) as a stencil: the separable Sobel filters of
// the prediction and of the target and the AbsLoss element between them in ONE launch each way
// (e2_sobel_abs_fwd / e2_sobel_abs_bwd).  The reference builds two Conv nodes with a constant,
// block-diagonal (dim F, F, 3, 3, 3) weight; here neither pred_sobel nor target_sobel is ever
// written to memory, and no matrix instruction runs: every output feature reads ONE input feature
// through one of three fixed filters, an implicit GEMM would spend F - 1 of every F products on
// zeros.
//
//   p prediction, t target, (N, F, D, H, W); dim = 3, or 2 with a unit D.  For a component k < dim
//   S_k is [1, 0, -1] along axis k (out(x) = v(x - 1) - v(x + 1)) times [0.3, 0.4, 0.3] along each
//   other spatial axis, over the zero-framed feature map ('same', zero bias):
//     ps = S_k p,  ts = S_k t,  d = ts - ps;  n_tot = dim N F D H W elements
//     l = |d| g c,  g = [|d| >= margin],  c = sc |ts| + 1,  masked where |ts + 666| <= 1e-8 + 666e-5
//   slab rows (S1, n_lab, S2, 0) as e2_loss_fwd's; the term is an ABS row of e2_loss_mix.
//     dp = -coef sum_k S_k^T s_k,  s_k = sgn(d) g c  (sgn 0 = 0, 0 where masked)
//   s_k exists at positions INSIDE the tensor only and is ZERO outside it: what the zero frame
//   would give at a position outside (t and p are 0 there, but their filtered values are not) must
//   never reach dp.  S_k is antisymmetric along its own axis and symmetric along the others, so
//   S_k^T = -S_k and dp = coef sum_k S_k s_k: the backward applies the forward's filter to s_k.
//
// Geometry.  A work-group of 256 threads owns one tile of TD x 8 x 32 positions (TD = 4; 1 for
// dim = 2) of one (n, f) map and walks the tiles grid-stride.  It stages the p and t tiles with their
// halo in LDS -- rows of 40 floats, the 32 interior columns at float 4, so that an interior quad is
// one 16-byte LDS store; 16-byte global loads where the quad is whole and aligned in the view,
// element by element otherwise; zeros (selects, never products) outside the tensor.  Thread
// (x = tid % 32, y = tid / 32) owns the z column of its position.  Per staged plane it reads the
// 3 x 3 neighbourhood and forms the in-plane parts separably -- along W: N_w v, D_w v; along H:
// A = N_h N_w v, B = N_h D_w v, C = D_h N_w v -- and a three-plane window in registers finishes them
// along D: (N_d B, N_d C, D_d A).  Nine multiply-adds per component set, not 3 x 27 taps.
//   forward:  halo 1 (6 x 10 x 34 of each operand, 19.2 KB LDS), the ABS element, one slab row per
//             work-group by a plain 16-byte store: no atomics, no zero fill.
//   backward: halo 2 (8 x 12 x 36, 30.7 KB).  s_k on the tile plus a halo of 1 (6 x 10 x 34 columns:
//             340 columns over 256 threads in two passes) stays in registers until every thread
//             has read its p / t, then takes their place in LDS; the same column code filters it.
//             A gather: no atomics; dpred = or += inside the view only.
// Nothing outside a view is read or written.  coef, margin and scale_correction are device scalars
// read when the kernel runs.  All arithmetic is f32, no contraction.
#include "stream_common.hpp"

namespace {

#define E2_SOBEL_MASK_TOL (1e-8f + 666e-5f)
#define E2_SOBEL_CAP 1024u         /* work-groups of a launch = slab rows of the forward */

typedef float sob_f4 __attribute__((ext_vector_type(4)));

constexpr int TH = 8, TW = 32;     // tile rows, columns (one thread each)
constexpr int RS = 40;             // floats per LDS row
constexpr int XC = 4;              // LDS column of the tile's first x
constexpr float K3 = 0.3f, K4 = 0.4f;

struct SView {
  long sn, sc, sd, sh;
};

struct SobP {
  const float* pred;
  const float* tgt;
  float* dpred;
  SView vp, vt, vd;
  int F, D, H, W;
  unsigned tiles;                  // N F tz ty tx  (< 2^31)
  unsigned tz, ty, tx;             // tiles along z, y, x
  FastDiv dx, dy, dz, df;
  const float* margin;             // device scalars, read when the kernel runs
  const float* sc;
  const float* coef;
  float* partials;                 // fwd: [gridDim.x][4]
};

struct Tile {
  int n, f, z0, y0, x0;
};
template <int TD>
__device__ __forceinline__ Tile locate(const SobP& p, unsigned t) {
  Tile q;
  unsigned r = fdiv(t, p.dx);
  q.x0 = (int)(t - r * p.tx) * TW;
  unsigned r2 = fdiv(r, p.dy);
  q.y0 = (int)(r - r2 * p.ty) * TH;
  r = fdiv(r2, p.dz);
  q.z0 = (int)(r2 - r * p.tz) * TD;
  q.n = (int)fdiv(r, p.df);
  q.f = (int)(r - (unsigned)q.n * (unsigned)p.F);
  return q;
}
__device__ __forceinline__ long map_off(const SView& v, const Tile& q) {
  return (long)q.n * v.sn + (long)q.f * v.sc;
}

// up to four consecutive floats, nv of them inside the row (nv <= 0: none); the rest zeros
__device__ __forceinline__ sob_f4 ld_quad(const float* g, int nv) {
  sob_f4 v = {0.f, 0.f, 0.f, 0.f};
  if (nv >= 4 && (((uintptr_t)g) & 15) == 0) {
    v = *reinterpret_cast<const sob_f4*>(g);
  } else {
    if (nv > 0) v[0] = g[0];
    if (nv > 1) v[1] = g[1];
    if (nv > 2) v[2] = g[2];
    if (nv > 3) v[3] = g[3];
  }
  return v;
}

// stage PZ x PY rows of both operands around the tile: HH halo columns / rows, HZ halo planes.
// An item is one interior quad (q < 8) or the 2 HH halo columns (q == 8) of one row.
template <int PZ, int PY, int HH, int HZ>
__device__ __forceinline__ void stage(const SobP& p, const Tile& q, float* sp, float* st) {
  const long bp = map_off(p.vp, q), bt = map_off(p.vt, q);
  for (int i = threadIdx.x; i < PZ * PY * 9; i += 256) {
    const int r = i / 9, k = i - r * 9;
    const int pz = r / PY, py = r - pz * PY;
    const int z = q.z0 - HZ + pz, y = q.y0 - HH + py;
    const bool row = z >= 0 && z < p.D && y >= 0 && y < p.H;
    const float* gp = p.pred + (bp + (long)z * p.vp.sd + (long)y * p.vp.sh);
    const float* gt = p.tgt + (bt + (long)z * p.vt.sd + (long)y * p.vt.sh);
    float* lp = sp + r * RS + XC;
    float* lt = st + r * RS + XC;
    if (k < 8) {
      const int x = q.x0 + 4 * k;
      const int nv = row ? p.W - x : 0;
      *reinterpret_cast<sob_f4*>(lp + 4 * k) = ld_quad(gp + x, nv);
      *reinterpret_cast<sob_f4*>(lt + 4 * k) = ld_quad(gt + x, nv);
    } else {
#pragma unroll
      for (int e = 0; e < HH; ++e) {
        const int xl = q.x0 - HH + e, xr = q.x0 + TW + e;
        const bool okl = row && xl >= 0, okr = row && xr < p.W;
        lp[e - HH] = okl ? gp[xl] : 0.f;
        lt[e - HH] = okl ? gt[xl] : 0.f;
        lp[TW + e] = okr ? gp[xr] : 0.f;
        lt[TW + e] = okr ? gt[xr] : 0.f;
      }
    }
  }
}

// the in-plane parts at one LDS position c: along W first, then along H
//   A = N_h N_w v   B = N_h D_w v   C = D_h N_w v      N = [0.3, 0.4, 0.3], D v (x) = v(x-1) - v(x+1)
struct Parts {
  float A, B, C;
};
__device__ __forceinline__ Parts plane_parts(const float* c) {
  float nw[3], dw[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float* r = c + (j - 1) * RS;
    const float a = r[-1], b = r[0], e = r[1];
    nw[j] = (K3 * a + K4 * b) + K3 * e;
    dw[j] = a - e;
  }
  Parts o;
  o.A = (K3 * nw[0] + K4 * nw[1]) + K3 * nw[2];
  o.B = (K3 * dw[0] + K4 * dw[1]) + K3 * dw[2];
  o.C = nw[0] - nw[2];
  return o;
}
// ... and along D over three consecutive planes: component 0 (x), 1 (y), 2 (z)
__device__ __forceinline__ float smooth3(float a, float b, float c) { return (K3 * a + K4 * b) + K3 * c; }

// The filtered values of one z column: NZ output planes from NZ + 2 LDS planes (DIM 3), or from
// the one plane there is (DIM 2: no z factor, no z component).  c: the column's position in the
// first LDS plane it reads; zs: floats between planes.  out[j][k]: plane j, component k.
template <int DIM, int NZ>
__device__ __forceinline__ void column(const float* c, int zs, float (&out)[NZ][DIM]) {
  if constexpr (DIM == 2) {
    const Parts o = plane_parts(c);
    out[0][0] = o.B;
    out[0][1] = o.C;
  } else {
    Parts w[3];
#pragma unroll
    for (int pz = 0; pz < NZ + 2; ++pz) {
      w[pz % 3] = plane_parts(c + pz * zs);
      if (pz >= 2) {
        const Parts &lo = w[(pz - 2) % 3], &mid = w[(pz - 1) % 3], &hi = w[pz % 3];
        out[pz - 2][0] = smooth3(lo.B, mid.B, hi.B);
        out[pz - 2][1] = smooth3(lo.C, mid.C, hi.C);
        out[pz - 2][2] = lo.A - hi.A;
      }
    }
  }
}

__device__ __forceinline__ bool masked(float t) { return fabsf(t + 666.0f) <= E2_SOBEL_MASK_TOL; }

// the ABS element of the table in include/e2hip.h on (ps, ts)
template <bool MARGIN, bool SC>
__device__ __forceinline__ void fwd_elem(float ps, float ts, float m, float sc, float& s1, float& nl,
                                         float& s2) {
  if (masked(ts)) return;
  nl += 1.f;
  const float ad = fabsf(ts - ps);
  const float c = SC ? sc * fabsf(ts) + 1.f : 1.f;
  float l = ad;
  if (MARGIN) {
    l = ad >= m ? l : 0.f;
    s2 += c;
  }
  s1 += l * c;
}
// s = sgn(d) g c, 0 where masked
template <bool MARGIN, bool SC>
__device__ __forceinline__ float sign_elem(float ps, float ts, float m, float sc) {
  if (masked(ts)) return 0.f;
  const float d = ts - ps;
  const float c = SC ? sc * fabsf(ts) + 1.f : 1.f;
  float g = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
  if (MARGIN) g = fabsf(d) >= m ? g : 0.f;
  return g * c;
}

template <int DIM, bool MARGIN, bool SC>
__global__ __launch_bounds__(256) void e2map_sobel_fwd_kernel(SobP p) {
  constexpr int TD = DIM == 3 ? 4 : 1, HZ = DIM == 3 ? 1 : 0;
  constexpr int PZ = TD + 2 * HZ, PY = TH + 2;
  __shared__ __attribute__((aligned(16))) float sp[PZ * PY * RS];
  __shared__ __attribute__((aligned(16))) float st[PZ * PY * RS];
  __shared__ float red[4][3];
  const float m = MARGIN ? e2_uniform_ld(p.margin, 0) : 0.f;
  const float sc = SC ? e2_uniform_ld(p.sc, 0) : 0.f;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int col = (ty + 1) * RS + XC + tx;
  float s1 = 0.f, nl = 0.f, s2 = 0.f;
  for (unsigned t = blockIdx.x; t < p.tiles; t += gridDim.x) {
    const Tile q = locate<TD>(p, t);
    stage<PZ, PY, 1, HZ>(p, q, sp, st);
    __syncthreads();
    float ps[TD][DIM], ts[TD][DIM];
    column<DIM, TD>(sp + col, PY * RS, ps);
    column<DIM, TD>(st + col, PY * RS, ts);
    if (q.y0 + ty < p.H && q.x0 + tx < p.W) {
#pragma unroll
      for (int j = 0; j < TD; ++j)
        if (q.z0 + j < p.D) {
#pragma unroll
          for (int k = 0; k < DIM; ++k) fwd_elem<MARGIN, SC>(ps[j][k], ts[j][k], m, sc, s1, nl, s2);
        }
    }
    __syncthreads();               // (the next tile's staging overwrites what was just read)
  }
  s1 = wave_sum(s1);
  nl = wave_sum(nl);
  s2 = wave_sum(s2);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[wave][0] = s1; red[wave][1] = nl; red[wave][2] = s2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    sob_f4 r;
    r[0] = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
    r[1] = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
    r[2] = (red[0][2] + red[1][2]) + (red[2][2] + red[3][2]);
    r[3] = 0.f;
    *reinterpret_cast<sob_f4*>(p.partials + 4l * blockIdx.x) = r;
  }
}

template <int DIM, bool MARGIN, bool SC, bool ACC>
__global__ __launch_bounds__(256) void e2map_sobel_bwd_kernel(SobP p) {
  constexpr int TD = DIM == 3 ? 4 : 1, HZ = DIM == 3 ? 1 : 0;
  constexpr int PZ = TD + 4 * HZ, PY = TH + 4;         // p / t: halo 2
  constexpr int QZ = TD + 2 * HZ, QY = TH + 2, QX = TW + 2;   // s_k: halo 1
  constexpr int OPER = PZ * PY * RS, COMP = QZ * QY * RS;
  static_assert(DIM * COMP <= 2 * OPER, "the s_k planes take the place of the staged operands");
  __shared__ __attribute__((aligned(16))) float lds[2 * OPER];
  float* const sp = lds;
  float* const st = lds + OPER;
  const float m = MARGIN ? e2_uniform_ld(p.margin, 0) : 0.f;
  const float sc = SC ? e2_uniform_ld(p.sc, 0) : 0.f;
  const float co = e2_uniform_ld(p.coef, 0);
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (unsigned t = blockIdx.x; t < p.tiles; t += gridDim.x) {
    const Tile q = locate<TD>(p, t);
    stage<PZ, PY, 2, 2 * HZ>(p, q, sp, st);
    __syncthreads();
    // s_k of the columns (qy, qx) of the tile plus its halo of 1; column c of pass a is tid + 256 a
    float s[2][QZ][DIM];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int c = (int)threadIdx.x + 256 * a;
      if (c < QY * QX) {
        const int qy = c / QX, qx = c - qy * QX;
        const int y = q.y0 - 1 + qy, x = q.x0 - 1 + qx;
        const bool in_xy = y >= 0 && y < p.H && x >= 0 && x < p.W;
        const int at = (qy + 1) * RS + XC - 1 + qx;
        float ps[QZ][DIM], ts[QZ][DIM];
        column<DIM, QZ>(sp + at, PY * RS, ps);
        column<DIM, QZ>(st + at, PY * RS, ts);
#pragma unroll
        for (int j = 0; j < QZ; ++j) {
          const int z = q.z0 - HZ + j;
          const bool in = in_xy && z >= 0 && z < p.D;  // ZERO outside the tensor
#pragma unroll
          for (int k = 0; k < DIM; ++k)
            s[a][j][k] = in ? sign_elem<MARGIN, SC>(ps[j][k], ts[j][k], m, sc) : 0.f;
        }
      }
    }
    __syncthreads();               // (every thread has read its p / t)
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int c = (int)threadIdx.x + 256 * a;
      if (c < QY * QX) {
        const int qy = c / QX, qx = c - qy * QX;
#pragma unroll
        for (int j = 0; j < QZ; ++j)
#pragma unroll
          for (int k = 0; k < DIM; ++k) lds[k * COMP + (j * QY + qy) * RS + XC - 1 + qx] = s[a][j][k];
      }
    }
    __syncthreads();
    // dp = coef sum_k S_k s_k: component k of the column code run on the plane set of s_k
    const int at = (ty + 1) * RS + XC + tx;
    float g[DIM][TD][DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k) column<DIM, TD>(lds + k * COMP + at, QY * RS, g[k]);
    if (q.y0 + ty < p.H && q.x0 + tx < p.W) {
      float* dp = p.dpred + (map_off(p.vd, q) + (long)(q.y0 + ty) * p.vd.sh + (long)(q.x0 + tx));
#pragma unroll
      for (int j = 0; j < TD; ++j)
        if (q.z0 + j < p.D) {
          float v = g[0][j][0] + g[1][j][1];
          if (DIM == 3) v += g[2][j][2];
          v *= co;
          float* o = dp + (long)(q.z0 + j) * p.vd.sd;
          *o = ACC ? *o + v : v;
        }
    }
    __syncthreads();               // (the next tile's staging overwrites s_k)
  }
}

unsigned cdiv_u(int a, int b) { return (unsigned)((a + b - 1) / b); }

// sizes, tiles and views of a launch; dpred may be null (forward)
int sobel_setup(const char* who, const e2_loss_term* term, int dim, const e2_tensor5* pred,
                const e2_tensor5* target, const e2_tensor5* dpred, SobP& p) {
  E2_REQUIRE(term->kind == E2_LOSS_ABS, "%s: the term must be of kind ABS, got %d", who, term->kind);
  E2_REQUIRE(dim == 2 || dim == 3, "%s: dim = %d, 2 or 3 are supported", who, dim);
  E2_REQUIRE(pred->n > 0 && pred->c > 0 && pred->d > 0 && pred->h > 0 && pred->w > 0,
             "%s: empty tensor (%d,%d,%d,%d,%d)", who, pred->n, pred->c, pred->d, pred->h, pred->w);
  E2_REQUIRE(dim == 3 || pred->d == 1, "%s: dim = 2 needs a unit z axis, got %d", who, pred->d);
  E2_REQUIRE(same_size(pred, target) && (!dpred || same_size(pred, dpred)), "%s: size mismatch", who);
  p.tz = cdiv_u(pred->d, dim == 3 ? 4 : 1);
  p.ty = cdiv_u(pred->h, TH);
  p.tx = cdiv_u(pred->w, TW);
  const unsigned long long tiles =
      (unsigned long long)pred->n * pred->c * p.tz * p.ty * (unsigned long long)p.tx;
  E2_REQUIRE(tiles < (1ull << 31), "%s: tensor too large", who);
  p.tiles = (unsigned)tiles;
  p.dx = mk_div(p.tx); p.dy = mk_div(p.ty); p.dz = mk_div(p.tz); p.df = mk_div((unsigned)pred->c);
  p.F = pred->c; p.D = pred->d; p.H = pred->h; p.W = pred->w;
  p.pred = pred->ptr; p.tgt = target->ptr;
  p.vp = SView{(long)pred->sn, (long)pred->sc, (long)pred->sd, (long)pred->sh};
  p.vt = SView{(long)target->sn, (long)target->sc, (long)target->sd, (long)target->sh};
  if (dpred) {
    p.dpred = dpred->ptr;
    p.vd = SView{(long)dpred->sn, (long)dpred->sc, (long)dpred->sd, (long)dpred->sh};
  }
  p.margin = term->margin; p.sc = term->scale_correction;
  return 0;
}

unsigned sobel_wgs(const SobP& p) { return p.tiles < E2_SOBEL_CAP ? p.tiles : E2_SOBEL_CAP; }

template <int DIM, bool MARGIN, bool SC>
void launch_bwd(e2_ctx* ctx, const SobP& p, bool acc) {
  const dim3 g(sobel_wgs(p)), b(256);
  if (acc) hipLaunchKernelGGL((e2map_sobel_bwd_kernel<DIM, MARGIN, SC, true>), g, b, 0, ctx->stream, p);
  else hipLaunchKernelGGL((e2map_sobel_bwd_kernel<DIM, MARGIN, SC, false>), g, b, 0, ctx->stream, p);
}
template <int DIM>
void launch_fwd_ms(e2_ctx* ctx, const SobP& p, bool m, bool s) {
  const dim3 g(sobel_wgs(p)), b(256);
  if (m && s) hipLaunchKernelGGL((e2map_sobel_fwd_kernel<DIM, true, true>), g, b, 0, ctx->stream, p);
  else if (m) hipLaunchKernelGGL((e2map_sobel_fwd_kernel<DIM, true, false>), g, b, 0, ctx->stream, p);
  else if (s) hipLaunchKernelGGL((e2map_sobel_fwd_kernel<DIM, false, true>), g, b, 0, ctx->stream, p);
  else hipLaunchKernelGGL((e2map_sobel_fwd_kernel<DIM, false, false>), g, b, 0, ctx->stream, p);
}
template <int DIM>
void launch_bwd_ms(e2_ctx* ctx, const SobP& p, bool m, bool s, bool acc) {
  if (m && s) launch_bwd<DIM, true, true>(ctx, p, acc);
  else if (m) launch_bwd<DIM, true, false>(ctx, p, acc);
  else if (s) launch_bwd<DIM, false, true>(ctx, p, acc);
  else launch_bwd<DIM, false, false>(ctx, p, acc);
}

}  // namespace

extern "C" size_t e2_sobel_abs_partials(e2_ctx*, const e2_tensor5* pred) {
  if (!pred || pred->n <= 0 || pred->c <= 0 || pred->d <= 0 || pred->h <= 0 || pred->w <= 0)
    return 0;
  // (a unit z axis is one tile deep under either dim: the count depends on the sizes alone)
  const unsigned long long tiles = (unsigned long long)pred->n * pred->c * cdiv_u(pred->d, 4) *
                                   cdiv_u(pred->h, TH) * (unsigned long long)cdiv_u(pred->w, TW);
  return (size_t)(tiles < E2_SOBEL_CAP ? tiles : E2_SOBEL_CAP);
}

extern "C" int e2_sobel_abs_fwd(e2_ctx* ctx, const e2_loss_term* term, int dim,
                                const e2_tensor5* pred, const e2_tensor5* target, float* partials) {
  E2_REQUIRE(ctx && term && pred && target && partials && pred->ptr && target->ptr,
             "e2_sobel_abs_fwd: null argument");
  E2_REQUIRE((((uintptr_t)partials) & 15) == 0, "e2_sobel_abs_fwd: partials must be 16-byte aligned");
  SobP p = SobP{};
  if (int rc = sobel_setup("e2_sobel_abs_fwd", term, dim, pred, target, nullptr, p)) return rc;
  p.partials = partials;
  const bool m = term->margin != nullptr, s = term->scale_correction != nullptr;
  if (dim == 3) launch_fwd_ms<3>(ctx, p, m, s);
  else launch_fwd_ms<2>(ctx, p, m, s);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_sobel_abs_bwd(e2_ctx* ctx, const e2_loss_term* term, int dim,
                                const e2_tensor5* pred, const e2_tensor5* target, const float* coef,
                                const e2_tensor5* dpred, int accumulate) {
  E2_REQUIRE(ctx && term && pred && target && coef && dpred && pred->ptr && target->ptr &&
                 dpred->ptr, "e2_sobel_abs_bwd: null argument");
  SobP p = SobP{};
  if (int rc = sobel_setup("e2_sobel_abs_bwd", term, dim, pred, target, dpred, p)) return rc;
  p.coef = coef;
  const bool m = term->margin != nullptr, s = term->scale_correction != nullptr;
  if (dim == 3) launch_bwd_ms<3>(ctx, p, m, s, accumulate != 0);
  else launch_bwd_ms<2>(ctx, p, m, s, accumulate != 0);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}
