// dense_gemm.hip -- the Perceptron's three dot products on the matrix cores.
//
//   Perceptron   neural.py:258-410   lin = dot(x.flatten(2), W), W of shape (n_in, n_f)
//                computations.py:179-213 `dot`; the two gradients are what T.grad makes of it
//
// One GEMM core, C[M x N] (+)= sum_K A * B on v_mfma_f32_16x16x4_f32 (f32 operands, f32 sums, also
// in bf16 mode), instantiated for the three operand orientations (n = batch, k = n_in, m = n_f,
// every matrix row-major):
//
//   op                       M x N   K   A                     B
//   fwd    y = x w           n x m   k   x,  K-contiguous      w,      N-contiguous
//   dgrad  dx (+)= dy w^T    n x k   m   dy, K-contiguous      w rows, K-contiguous
//   wgrad  dw (+)= x^T dy    k x m   n   x,  M-contiguous      dy,     N-contiguous
//
// A work-group of four waves owns one BM x BN tile of C and walks its K range in chunks of 32.
// Both operand panels of a chunk stand in LDS K-major -- As[kk][row], Bs[kk][col] -- which is the
// order the MFMA lanes read: lane (l15, qd) of step s takes As[4 s + qd][.. + l15] and
// Bs[4 s + qd][.. + l15].  The pitch of a panel is 16 * (an odd number) floats, so the four qd
// rows of one ds_read_b32 start 16 banks apart and their 16 consecutive floats never overlap: no
// bank conflict, for 32 banks and for 64.
//   An operand that is contiguous along M / N is copied as it lies (16-byte global load, 16-byte
// LDS write).  A K-contiguous operand is fetched by 16-byte loads along K and transposed on the way
// in: a lane holds four k of ONE row and writes them to four LDS rows; adjacent lanes hold adjacent
// rows, so each of the four ds_write_b32 covers consecutive banks.
//   The loads of chunk c + 1 are issued into registers before the MFMAs of chunk c and written to
// LDS behind them (one LDS buffer, two barriers per chunk).  The accumulators stay in registers for
// the whole K range.  The MFMA takes the B fragment in its first slot and the A fragment in its
// second, i.e. computes the transposed block: a lane then owns C[row l15][4 qd .. 4 qd + 3], four
// consecutive floats of one row, one 16-byte store.
//   Tile edges and the last chunk are masked in the kernel: a 16-byte piece that is whole and
// aligned (base pointer and pitch multiples of 16 bytes) goes as one load / store, any other piece
// element by element, elements outside the matrix read as 0 and are not written.
//
// Split-K without atomics: split s of S takes the k-steps (4 k each) [s per, (s + 1) per) and
// stores its partial tile into slab s of the caller's workspace (S dense M x N slabs); one small
// launch adds slab 0, 1, .. S-1 in that order and adds the base when `accumulate` is set.  With
// S = 1 the GEMM's epilogue writes (or adds onto) C itself.  Nothing depends on the order the
// work-groups run in: results are bit-reproducible for every form and split count.
#include "common.hpp"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

enum { OP_FWD = 0, OP_DGRAD = 1, OP_WGRAD = 2 };
constexpr int KC = 32;                  // k per chunk (8 MFMA steps)
constexpr int kMaxSplits = 1024;
// the split rule aims at one work-group per CU of an MI355X (a constant, not the device's count:
// the workspace size is asked for without a context, and results do not depend on the device)
constexpr int kTargetWGs = 256;
constexpr int kAutoMaxSplits = 64;

struct DenseP {
  const float* A;
  const float* B;
  float* C;               // the output, or the first slab
  int64_t lda, ldb, ldc;     // pitches (floats) of A, B, C / the slabs
  long slab;              // floats between slabs (splits > 1), else 0
  int M, N, K;
  int tm, tn;             // tiles along M, N
  int per;                // k-steps per split
  int accumulate;         // splits == 1: add onto C
  int avec, bvec, cvec;   // 16-byte pieces of A / B / C are aligned
};

// ---- the shape rule, the split rule (the ONLY place either is stated) ---------------------------
struct Choice {
  int M, N, K;
  int bm, bn;             // tile shape
  int tiles, splits, per; // output tiles; splits and k-steps (of 4 k) per split
  int limit;              // most splits the caller may ask for
};
static void op_dims(int op, int n, int k, int m, int* M, int* N, int* K) {
  *M = op == OP_WGRAD ? k : n;
  *N = op == OP_DGRAD ? k : m;
  *K = op == OP_FWD ? k : (op == OP_DGRAD ? m : n);
}
// Shape rule: up to 32 rows of C (a batch-sized M: fwd and dgrad at n <= 32) run the 16 x 128 tile,
// four waves side by side; everything else the 64 x 64 tile, 2 x 2 waves of 32 x 32.
// Split rule (splits == 0): no split once the tiles fill a quarter of the card; else as many splits
// as bring the grid to kTargetWGs work-groups, each keeping at least two whole chunks, at most
// kAutoMaxSplits; the K range is dealt out in whole chunks.  splits >= 1: honoured up to `limit`
// = min(k-steps, kMaxSplits), the K range dealt out in k-steps.
static Choice dense_choose(int op, int n, int k, int m, int splits) {
  Choice c;
  op_dims(op, n, k, m, &c.M, &c.N, &c.K);
  const bool skinny = c.M <= 32;
  c.bm = skinny ? 16 : 64;
  c.bn = skinny ? 128 : 64;
  c.tiles = e2_cdiv(c.M, c.bm) * e2_cdiv(c.N, c.bn);
  const int ksteps = e2_cdiv(c.K, 4), chunks = e2_cdiv(c.K, KC);
  c.limit = ksteps < kMaxSplits ? ksteps : kMaxSplits;
  if (splits >= 1) {
    c.splits = splits < c.limit ? splits : c.limit;
    c.per = e2_cdiv(ksteps, c.splits);
    return c;
  }
  int want = 4 * c.tiles > kTargetWGs ? 1 : kTargetWGs / c.tiles;
  if (want > chunks / 2) want = chunks / 2;
  if (want > kAutoMaxSplits) want = kAutoMaxSplits;
  if (want < 1) want = 1;
  const int per_chunks = e2_cdiv(chunks, want);
  c.splits = e2_cdiv(chunks, per_chunks);
  c.per = per_chunks * (KC / 4);
  return c;
}
static size_t choice_ws_bytes(const Choice& c) {
  return c.splits > 1 ? (size_t)c.splits * (size_t)c.M * (size_t)c.N * sizeof(float) : 0;
}

// ---- staging --------------------------------------------------------------------------------
// One operand panel of a chunk: R rows (M or N of the tile) x KC k.  KCONT: element (row, k) lies
// at base[row * ld + k] (K-contiguous), else at base[k * ld + row].  A thread fetches CNT 16-byte
// pieces into registers (fetch) and writes them K-major into LDS (put), pitch P.
template <int R>
struct Panel {
  static constexpr int PIECES = R * KC / 4;
  static constexpr int CNT = (PIECES + 255) / 256;
  static constexpr int P = R + ((R / 16) % 2 == 0 ? 16 : 0);    // 16 * odd
  f32x4 v[CNT];
};

template <int R, bool KCONT>
__device__ __forceinline__ void panel_fetch(Panel<R>& pn, const float* __restrict__ base, int64_t ld,
                                            int r0, int rlim, int k0, int kend, int vec, int tid) {
#pragma unroll
  for (int i = 0; i < Panel<R>::CNT; ++i) {
    const int e = tid + 256 * i;
    f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (Panel<R>::PIECES % 256 == 0 || e < Panel<R>::PIECES) {
      if constexpr (KCONT) {
        const int row = r0 + e % R, kk = k0 + 4 * (e / R);        // adjacent lanes: adjacent rows
        if (row < rlim && kk < kend) {
          const float* src = base + (long)row * ld + kk;
          if (vec && kk + 3 < kend) {
            v = *reinterpret_cast<const f32x4*>(src);
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (kk + j < kend) v[j] = src[j];
          }
        }
      } else {
        const int row = r0 + 4 * (e % (R / 4)), kk = k0 + e / (R / 4);
        if (row < rlim && kk < kend) {
          const float* src = base + (long)kk * ld + row;
          if (vec && row + 3 < rlim) {
            v = *reinterpret_cast<const f32x4*>(src);
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (row + j < rlim) v[j] = src[j];
          }
        }
      }
    }
    pn.v[i] = v;
  }
}

template <int R, bool KCONT>
__device__ __forceinline__ void panel_put(const Panel<R>& pn, float* __restrict__ lds, int tid) {
  constexpr int P = Panel<R>::P;
#pragma unroll
  for (int i = 0; i < Panel<R>::CNT; ++i) {
    const int e = tid + 256 * i;
    if (Panel<R>::PIECES % 256 == 0 || e < Panel<R>::PIECES) {
      if constexpr (KCONT) {
        float* dst = lds + (4 * (e / R)) * P + e % R;
#pragma unroll
        for (int j = 0; j < 4; ++j) dst[j * P] = pn.v[i][j];
      } else {
        *reinterpret_cast<f32x4*>(lds + (e / (R / 4)) * P + 4 * (e % (R / 4))) = pn.v[i];
      }
    }
  }
}

// ---- the kernel -------------------------------------------------------------------------------
// BM x BN tile, WM x WN waves (WM * WN == 4), each wave MT x NT blocks of 16 x 16.
template <int BM, int BN, int WM, int WN, bool AK, bool BK>
__global__ __launch_bounds__(256) void dense_gemm_kernel(DenseP p) {
  static_assert(WM * WN == 4, "four waves");
  constexpr int MT = BM / (16 * WM), NT = BN / (16 * WN);
  constexpr int PA = Panel<BM>::P, PB = Panel<BN>::P;
  __shared__ __attribute__((aligned(16))) float As[KC * PA];
  __shared__ __attribute__((aligned(16))) float Bs[KC * PB];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave - wm * WN;
  const int l15 = lane & 15, qd = lane >> 4;

  int bid = blockIdx.x;
  const int mt = bid % p.tm; bid /= p.tm;
  const int nt = bid % p.tn;
  const int ks = bid / p.tn;
  const int m0 = mt * BM, n0 = nt * BN;
  const int kbeg = ks * p.per * 4;
  const int kend = min(p.K, kbeg + p.per * 4);     // (kbeg >= kend: an empty split stores zeros)

  f32x4 acc[MT][NT];
#pragma unroll
  for (int mb = 0; mb < MT; ++mb)
#pragma unroll
    for (int nb = 0; nb < NT; ++nb) acc[mb][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};

  Panel<BM> pa;
  Panel<BN> pb;
  if (kbeg < kend) {
    panel_fetch<BM, AK>(pa, p.A, p.lda, m0, p.M, kbeg, kend, p.avec, tid);
    panel_fetch<BN, BK>(pb, p.B, p.ldb, n0, p.N, kbeg, kend, p.bvec, tid);
  }
  const float* ar = As + qd * PA + wm * (16 * MT) + l15;
  const float* br = Bs + qd * PB + wn * (16 * NT) + l15;
  for (int k0 = kbeg; k0 < kend; k0 += KC) {
    __syncthreads();                               // the MFMAs of the chunk before have read LDS
    panel_put<BM, AK>(pa, As, tid);
    panel_put<BN, BK>(pb, Bs, tid);
    __syncthreads();
    if (k0 + KC < kend) {                          // next chunk: in flight under the MFMAs below
      panel_fetch<BM, AK>(pa, p.A, p.lda, m0, p.M, k0 + KC, kend, p.avec, tid);
      panel_fetch<BN, BK>(pb, p.B, p.ldb, n0, p.N, k0 + KC, kend, p.bvec, tid);
    }
    const int nks = min(KC / 4, (kend - k0 + 3) >> 2);
    auto step = [&](int s) {
      float a[MT], b[NT];
#pragma unroll
      for (int mb = 0; mb < MT; ++mb) a[mb] = ar[4 * s * PA + 16 * mb];
#pragma unroll
      for (int nb = 0; nb < NT; ++nb) b[nb] = br[4 * s * PB + 16 * nb];
#pragma unroll
      for (int mb = 0; mb < MT; ++mb)
#pragma unroll
        for (int nb = 0; nb < NT; ++nb)
          acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[nb], a[mb], acc[mb][nb], 0, 0, 0);
    };
    if (nks == KC / 4) {
#pragma unroll
      for (int s = 0; s < KC / 4; ++s) step(s);
    } else {
      for (int s = 0; s < nks; ++s) step(s);
    }
  }

  // ---- epilogue: lane (l15, qd) owns C[row l15][4 qd .. 4 qd + 3] of each block ---------------
  float* out = p.C + (long)ks * p.slab;
#pragma unroll
  for (int mb = 0; mb < MT; ++mb) {
    const int row = m0 + wm * (16 * MT) + 16 * mb + l15;
    if (row >= p.M) continue;
#pragma unroll
    for (int nb = 0; nb < NT; ++nb) {
      const int col = n0 + wn * (16 * NT) + 16 * nb + 4 * qd;
      if (col >= p.N) continue;
      float* dst = out + (long)row * p.ldc + col;
      f32x4 v = acc[mb][nb];
      if (p.cvec && col + 3 < p.N) {
        if (p.accumulate) {
          const f32x4 o = *reinterpret_cast<const f32x4*>(dst);
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = o[j] + v[j];
        }
        *reinterpret_cast<f32x4*>(dst) = v;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (col + j < p.N) dst[j] = p.accumulate ? dst[j] + v[j] : v[j];
      }
    }
  }
}

// C[i][j] (+)= slab 0 + slab 1 + ... in that order; one thread per element
__global__ __launch_bounds__(256) void dense_gemm_reduce_kernel(const float* __restrict__ ws,
                                                                int splits, int M, int N,
                                                                float* __restrict__ C, long ldc,
                                                                int accumulate) {
  const long idx = blockIdx.x * 256L + threadIdx.x;
  const long tot = (long)M * N;
  if (idx >= tot) return;
  float v = ws[idx];
  for (int s = 1; s < splits; ++s) v += ws[(long)s * tot + idx];
  const long i = idx / N;
  float* dst = C + i * ldc + (idx - i * N);
  *dst = accumulate ? *dst + v : v;
}

static bool al16(const void* ptr, long ld) { return ((uintptr_t)ptr & 15) == 0 && (ld & 3) == 0; }

template <bool AK, bool BK>
static int dense_gemm_run(e2_ctx* ctx, const char* who, const Choice& c, const float* A, long lda,
                          const float* B, long ldb, float* C, long ldc, int accumulate, void* ws,
                          size_t ws_bytes) {
  const size_t need = choice_ws_bytes(c);
  E2_REQUIRE(need == 0 || (ws && ws_bytes >= need),
             "%s: %d splits of the %d x %d output need a workspace of %zu bytes, got %zu", who,
             c.splits, c.M, c.N, need, ws ? ws_bytes : (size_t)0);
  DenseP p;
  p.A = A; p.B = B; p.lda = lda; p.ldb = ldb;
  p.M = c.M; p.N = c.N; p.K = c.K;
  p.tm = e2_cdiv(c.M, c.bm); p.tn = e2_cdiv(c.N, c.bn);
  p.per = c.per;
  p.avec = al16(A, lda); p.bvec = al16(B, ldb);
  if (c.splits > 1) {
    p.C = (float*)ws; p.ldc = c.N; p.slab = (long)c.M * c.N; p.accumulate = 0;
  } else {
    p.C = C; p.ldc = ldc; p.slab = 0; p.accumulate = accumulate;
  }
  p.cvec = al16(p.C, p.ldc) && (p.slab & 3) == 0;
  const long grid = (long)c.tiles * c.splits;
  E2_REQUIRE(grid < (1L << 31), "%s: %ld work-groups", who, grid);
  if (c.bm == 16)
    hipLaunchKernelGGL((dense_gemm_kernel<16, 128, 1, 4, AK, BK>), dim3((unsigned)grid), dim3(256),
                       0, ctx->stream, p);
  else
    hipLaunchKernelGGL((dense_gemm_kernel<64, 64, 2, 2, AK, BK>), dim3((unsigned)grid), dim3(256),
                       0, ctx->stream, p);
  E2_CHECK_HIP(hipGetLastError());
  if (c.splits > 1) {
    const long tot = (long)c.M * c.N;
    hipLaunchKernelGGL(dense_gemm_reduce_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0,
                       ctx->stream, (const float*)ws, c.splits, c.M, c.N, C, ldc, accumulate);
    E2_CHECK_HIP(hipGetLastError());
  }
  return 0;
}

static int dense_args_ok(const char* who, const void* ctx, const void* a, const void* b,
                         const void* c, int n, int k, int m, int splits, int op, Choice* out) {
  E2_REQUIRE(ctx && a && b && c, "%s: null argument", who);
  E2_REQUIRE(n > 0 && k > 0 && m > 0, "%s: sizes must be positive, got n=%d k=%d m=%d", who, n, k, m);
  E2_REQUIRE(splits >= 0, "%s: splits must be 0 (the library chooses) or positive, got %d", who, splits);
  *out = dense_choose(op, n, k, m, splits);
  E2_REQUIRE(splits <= out->limit, "%s: %d splits asked for, a reduction of length %d allows at most %d",
             who, splits, out->K, out->limit);
  return 0;
}

}  // namespace

extern "C" int e2_dense_gemm_choice(int op, int n, int k, int m, int splits, int* out6) {
  E2_REQUIRE(op >= OP_FWD && op <= OP_WGRAD && out6, "dense_gemm_choice: bad argument");
  Choice c;
  if (int rc = dense_args_ok("dense_gemm_choice", out6, out6, out6, out6, n, k, m, splits, op, &c))
    return rc;
  out6[0] = c.bm; out6[1] = c.bn; out6[2] = c.tiles; out6[3] = c.splits; out6[4] = c.per;
  out6[5] = c.limit;
  return 0;
}

extern "C" size_t e2_dense_gemm_workspace_bytes(int n, int k, int m, int splits) {
  if (n <= 0 || k <= 0 || m <= 0 || splits < 0) return 0;
  size_t most = 0;
  for (int op = OP_FWD; op <= OP_WGRAD; ++op) {      // (splits beyond an op's limit: its limit)
    const size_t b = choice_ws_bytes(dense_choose(op, n, k, m, splits));
    most = b > most ? b : most;
  }
  return most;
}

extern "C" int e2_dense_gemm_fwd(e2_ctx* ctx, const float* x, int64_t ldx, const float* w, float* y,
                                 int64_t ldy, int n, int k, int m, int splits, void* ws,
                                 size_t ws_bytes) {
  Choice c;
  if (int rc = dense_args_ok("dense_gemm_fwd", ctx, x, w, y, n, k, m, splits, OP_FWD, &c)) return rc;
  E2_REQUIRE(ldx >= k && ldy >= m, "dense_gemm_fwd: pitch below the row length (ldx %ld < %d or ldy %ld < %d)",
             ldx, k, ldy, m);
  return dense_gemm_run<true, false>(ctx, "dense_gemm_fwd", c, x, ldx, w, m, y, ldy, 0, ws, ws_bytes);
}

extern "C" int e2_dense_gemm_dgrad(e2_ctx* ctx, const float* dy, int64_t lddy, const float* w,
                                   float* dx, int64_t lddx, int n, int k, int m, int accumulate,
                                   int splits, void* ws, size_t ws_bytes) {
  Choice c;
  if (int rc = dense_args_ok("dense_gemm_dgrad", ctx, dy, w, dx, n, k, m, splits, OP_DGRAD, &c)) return rc;
  E2_REQUIRE(lddy >= m && lddx >= k,
             "dense_gemm_dgrad: pitch below the row length (lddy %ld < %d or lddx %ld < %d)", lddy, m, lddx, k);
  return dense_gemm_run<true, true>(ctx, "dense_gemm_dgrad", c, dy, lddy, w, m, dx, lddx,
                                    accumulate ? 1 : 0, ws, ws_bytes);
}

extern "C" int e2_dense_gemm_wgrad(e2_ctx* ctx, const float* x, int64_t ldx, const float* dy,
                                   int64_t lddy, float* dw, int n, int k, int m, int accumulate,
                                   int splits, void* ws, size_t ws_bytes) {
  Choice c;
  if (int rc = dense_args_ok("dense_gemm_wgrad", ctx, x, dy, dw, n, k, m, splits, OP_WGRAD, &c)) return rc;
  E2_REQUIRE(ldx >= k && lddy >= m,
             "dense_gemm_wgrad: pitch below the row length (ldx %ld < %d or lddy %ld < %d)", ldx, k, lddy, m);
  return dense_gemm_run<false, false>(ctx, "dense_gemm_wgrad", c, x, ldx, dy, lddy, dw, m,
                                      accumulate ? 1 : 0, ws, ws_bytes);
}
