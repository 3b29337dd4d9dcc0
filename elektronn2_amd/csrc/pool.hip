// pool.hip -- average / sum pooling with a stride of its own (e2_pool3d_lin_fwd / _bwd): the device
// side of the Pool node's linear modes (neural.py:1409-1559; computations.py:538-649, where they
// exist on the dnn_pool route only, pad 0, any stride).
//
//   out[n, c, oz, oy, ox] = scale * sum_{dz < pz} sum_{dy < py} sum_{dx < px}
//                                   x[n, c, oz sz + dz, oy sy + dy, ox sx + dx]
//   scale = 1 (sum), 1 / (pz py px) (average);  out extent = floor((in - p) / s) + 1 per axis
//
// The window is walked in ascending (z, y, x) order and added up in f32.  The backward is a GATHER:
// the thread that owns an element of dx adds up dout over the windows that hold it -- per axis the
// outputs o with max(0, ceil((i - p + 1) / s)) <= o <= min(O - 1, floor(i / s)) -- in ascending
// order and scales once.  Overlapping windows (s < p) need no atomics, elements in the gaps between
// windows (s > p) and behind the last window come out as +0, or keep their bits with `accumulate`
// (a plain read-add-write); two runs give the same bits.  x is not read in the backward.
//
// Geometry of act.hip / pad.hip: a work-group stays inside one (n, c), a thread owns FOUR
// consecutive x of one destination row (out in the forward, dx in the backward).  The quads are cut
// where the DESTINATION row is 16-byte aligned, so every whole quad is one 16-byte store.  The span
// of the source row a quad needs (its windows in the forward, the outputs that cover it in the
// backward) is walked in pieces cut where the SOURCE row is 16-byte aligned: a piece inside the row
// is one 16-byte load, the pieces at row ends are fetched element by element.  Each fetched element
// is added to the accumulators of the quad elements whose range holds it.  Nothing outside the
// destination view is written, nothing outside the source view is read.  Pure stream: no LDS, no
// workspace; window and stride are runtime values, the mode is a template parameter.
#include "stream_common.hpp"

namespace {

// s: the tensor that is read (x / dout), o: the tensor that is written (out / dx)
struct PoolP {
  const float* s;
  float* o;
  long sn, sc, sd, sh;          // strides of the tensor read: batch, feature, d, h
  long on, oc, od, oh;          // strides of the tensor written
  unsigned W, H, D;             // extents of the tensor written
  unsigned sW, sH, sD;          // extents of the tensor read
  unsigned pz, py, px;          // window
  unsigned tz, ty, tx;          // stride
  unsigned quads;               // quads provided per destination row: (W + 3) / 4 + 1
  unsigned items;               // D * H * quads  (< 2^31)
  unsigned chunk;               // items per work-group, a multiple of 256
  FastDiv dq, dh;
  FastDiv dtz, dty, dtx;        // division by the stride (backward: the covering outputs)
  float scale;
  int accumulate;
};

typedef float pool_f4 __attribute__((ext_vector_type(4)));

// -0 is the identity of the f32 addition (-0 + v == v for every v, -0 included), so a window of
// one element hands its bits through
#define E2_POOL_ZERO (-0.0f)

// FZ > 0: the window is (FZ, FY, 2) and the stride equals it (the poolings of the U-Nets).  A whole
// quad then reads 8 consecutive floats of each of FZ * FY rows; where all of them start on a 16-byte
// boundary the loads are issued together, ahead of the first add.  The adds run in the order of the
// generic path, which takes every other quad: the bits do not depend on the path.
template <int MODE, int FZ, int FY>
__global__ __launch_bounds__(256) void e2pool_lin_fwd_kernel(PoolP p) {
  const unsigned s0 = blockIdx.x * p.chunk;
  const unsigned s1 = min(s0 + p.chunk, p.items);
  const unsigned c = blockIdx.y, n = blockIdx.z;
  const float* sbase = p.s + (long)n * p.sn + (long)c * p.sc;
  float* obase = p.o + (long)n * p.on + (long)c * p.oc;
  for (unsigned s = s0 + threadIdx.x; s < s1; s += 256) {
    const unsigned row = fdiv(s, p.dq);
    const unsigned q = s - row * p.quads;
    const unsigned z = fdiv(row, p.dh);
    const unsigned y = row - z * p.H;
    float* drow = obase + (long)z * p.od + (long)y * p.oh;
    // elements by which the row starts behind a 16-byte boundary; quad q covers the row's
    // x in [4 q - m, 4 q - m + 4), cut to [0, W)
    const unsigned m = (unsigned)((((uintptr_t)drow) >> 2) & 3);
    const int xa = (int)(q << 2) - (int)m;
    const unsigned x0 = xa < 0 ? 0u : (unsigned)xa;
    const unsigned x1 = min((unsigned)(xa + 4), p.W);
    if (xa + 4 <= 0 || x0 >= x1) continue;         // (the spare quad of an aligned row)
    // the source columns this quad's windows span: [u0, u1), inside [0, sW)
    const int u0 = (int)(x0 * p.tx), u1 = (int)((x1 - 1) * p.tx + p.px);
    // element e of the quad owns columns [w0 + e tx, w0 + e tx + px)  (e with x outside [x0, x1)
    // gather values that are not stored)
    const int w0 = xa * (int)p.tx;
    float acc[4] = {E2_POOL_ZERO, E2_POOL_ZERO, E2_POOL_ZERO, E2_POOL_ZERO};
    const float* srow0 = sbase + (long)(z * p.tz) * p.sd + (long)(y * p.ty) * p.sh;
    bool fast = false;
    if (FZ > 0) {
      constexpr int R = FZ > 0 ? FZ * FY : 1;
      const float* a[R];
      fast = (x1 - x0) == 4u;
#pragma unroll
      for (int k = 0; k < R; ++k) {
        a[k] = srow0 + (long)(k / FY) * p.sd + (long)(k % FY) * p.sh + u0;
        fast = fast && ((((uintptr_t)a[k]) & 15) == 0);
      }
      if (fast) {
        pool_f4 r[R][2];
#pragma unroll
        for (int k = 0; k < R; ++k) {
          r[k][0] = *reinterpret_cast<const pool_f4*>(a[k]);
          r[k][1] = *reinterpret_cast<const pool_f4*>(a[k] + 4);
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            acc[e] += r[k][e >> 1][(e & 1) * 2];
            acc[e] += r[k][e >> 1][(e & 1) * 2 + 1];
          }
        }
      }
    }
    for (unsigned dz = 0; !fast && dz < p.pz; ++dz) {
      for (unsigned dy = 0; dy < p.py; ++dy) {
        const float* srow = srow0 + (long)dz * p.sd + (long)dy * p.sh;
        const int ms = (int)((((uintptr_t)srow) >> 2) & 3);
        for (int ua = u0 - ((ms + u0) & 3); ua < u1; ua += 4) {
          pool_f4 r;
          if (ua >= 0 && ua + 4 <= (int)p.sW) {
            r = *reinterpret_cast<const pool_f4*>(srow + ua);
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int u = ua + j;
              r[j] = (u >= u0 && u < u1) ? srow[u] : 0.f;
            }
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int u = ua + j;
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if ((unsigned)(u - w0 - e * (int)p.tx) < p.px) acc[e] += r[j];
          }
        }
      }
    }
    if (MODE == E2_POOL_AVG) {
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] *= p.scale;
    }
    if ((x1 - x0) == 4u) {
      pool_f4 r;
      r[0] = acc[0]; r[1] = acc[1]; r[2] = acc[2]; r[3] = acc[3];
      *reinterpret_cast<pool_f4*>(drow + x0) = r;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int x = xa + e;
        if (x >= (int)x0 && x < (int)x1) drow[x] = acc[e];
      }
    }
  }
}

// the outputs whose window holds input coordinate i: [lo, hi] (empty: lo > hi)
__device__ __forceinline__ void cover(unsigned i, unsigned p, unsigned t, unsigned O,
                                      const FastDiv& dt, int* lo, int* hi) {
  *lo = (i + 1 > p) ? (int)fdiv(i - p + t, dt) : 0;              // ceil((i - p + 1) / t)
  *hi = (int)min(O - 1, fdiv(i, dt));
}

// (the many wave-uniform values of the two cover ranges: held to the scalar registers of 8 waves
// per SIMD, which the grid is sized for)
// TILED: the stride equals the window, so every element of dx lies in at most one window and the
// gather is one load: dx[z, y, x] = scale * dout[z / pz, y / py, x / px].
template <int MODE, bool TILED>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8)))
void e2pool_lin_bwd_kernel(PoolP p) {
  const unsigned s0 = blockIdx.x * p.chunk;
  const unsigned s1 = min(s0 + p.chunk, p.items);
  const unsigned c = blockIdx.y, n = blockIdx.z;
  const float* sbase = p.s + (long)n * p.sn + (long)c * p.sc;    // dout
  float* obase = p.o + (long)n * p.on + (long)c * p.oc;          // dx
  for (unsigned s = s0 + threadIdx.x; s < s1; s += 256) {
    const unsigned row = fdiv(s, p.dq);
    const unsigned q = s - row * p.quads;
    const unsigned z = fdiv(row, p.dh);
    const unsigned y = row - z * p.H;
    float* drow = obase + (long)z * p.od + (long)y * p.oh;
    const unsigned m = (unsigned)((((uintptr_t)drow) >> 2) & 3);
    const int xa = (int)(q << 2) - (int)m;
    const unsigned x0 = xa < 0 ? 0u : (unsigned)xa;
    const unsigned x1 = min((unsigned)(xa + 4), p.W);
    if (xa + 4 <= 0 || x0 >= x1) continue;
    float acc[4] = {E2_POOL_ZERO, E2_POOL_ZERO, E2_POOL_ZERO, E2_POOL_ZERO};
    bool cov[4];
    if (TILED) {
      const unsigned oz = fdiv(z, p.dtz), oy = fdiv(y, p.dty);
      const bool rows = oz < p.sD && oy < p.sH;
      const float* srow = sbase + (long)oz * p.sd + (long)oy * p.sh;   // (read only if ``rows``)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int x = xa + e;
        const bool valid = x >= (int)x0 && x < (int)x1;
        const unsigned ox = valid ? fdiv((unsigned)x, p.dtx) : 0u;
        cov[e] = valid && rows && ox < p.sW;
        if (cov[e]) acc[e] += srow[ox];
      }
    } else {
    int zlo, zhi, ylo, yhi;
    cover(z, p.pz, p.tz, p.sD, p.dtz, &zlo, &zhi);
    cover(y, p.py, p.ty, p.sH, p.dty, &ylo, &yhi);
    int lo[4], hi[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int x = xa + e;
      if (x >= (int)x0 && x < (int)x1) cover((unsigned)x, p.px, p.tx, p.sW, p.dtx, &lo[e], &hi[e]);
      else { lo[e] = 1; hi[e] = 0; }
    }
    const bool rows = zlo <= zhi && ylo <= yhi;
    // the dout columns the quad gathers from: [u0, u1) (lo and hi do not fall along the row)
    int u0 = 0x7fffffff, u1 = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (lo[e] <= hi[e]) { u0 = min(u0, lo[e]); u1 = max(u1, hi[e] + 1); }
    if (rows && u0 < u1) {
      for (int oz = zlo; oz <= zhi; ++oz) {
        for (int oy = ylo; oy <= yhi; ++oy) {
          const float* srow = sbase + (long)oz * p.sd + (long)oy * p.sh;
          const int ms = (int)((((uintptr_t)srow) >> 2) & 3);
          for (int ua = u0 - ((ms + u0) & 3); ua < u1; ua += 4) {
            pool_f4 r;
            if (ua >= 0 && ua + 4 <= (int)p.sW) {
              r = *reinterpret_cast<const pool_f4*>(srow + ua);
            } else {
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const int u = ua + j;
                r[j] = (u >= u0 && u < u1) ? srow[u] : 0.f;
              }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int u = ua + j;
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (u >= lo[e] && u <= hi[e]) acc[e] += r[j];
            }
          }
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) cov[e] = rows && lo[e] <= hi[e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (MODE == E2_POOL_AVG) acc[e] *= p.scale;
      if (!cov[e]) acc[e] = 0.f;
    }
    if (p.accumulate) {
      // elements no window covers keep their bits
      if (!(cov[0] || cov[1] || cov[2] || cov[3])) continue;
      if ((x1 - x0) == 4u) {
        pool_f4 r = *reinterpret_cast<const pool_f4*>(drow + x0);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (cov[e]) r[e] += acc[e];
        *reinterpret_cast<pool_f4*>(drow + x0) = r;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (cov[e]) drow[xa + e] += acc[e];
      }
    } else if ((x1 - x0) == 4u) {
      pool_f4 r;
      r[0] = acc[0]; r[1] = acc[1]; r[2] = acc[2]; r[3] = acc[3];
      *reinterpret_cast<pool_f4*>(drow + x0) = r;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int x = xa + e;
        if (x >= (int)x0 && x < (int)x1) drow[x] = acc[e];
      }
    }
  }
}

// big: the unpooled tensor (x / dx), small: the pooled one (out / dout)
int geometry_ok(const char* who, const e2_tensor5* big, const e2_tensor5* small, int pz, int py,
                int px, int sz, int sy, int sx, int mode) {
  E2_REQUIRE(mode == E2_POOL_AVG || mode == E2_POOL_SUM, "%s: bad mode %d (1 average, 2 sum)", who,
             mode);
  E2_REQUIRE(pz >= 1 && py >= 1 && px >= 1 && sz >= 1 && sy >= 1 && sx >= 1,
             "%s: window %d,%d,%d / stride %d,%d,%d below 1", who, pz, py, px, sz, sy, sx);
  E2_REQUIRE(pz <= big->d && py <= big->h && px <= big->w,
             "%s: window %d,%d,%d exceeds the extents %d,%d,%d", who, pz, py, px, big->d, big->h,
             big->w);
  E2_REQUIRE(small->n == big->n && small->c == big->c && small->d == (big->d - pz) / sz + 1 &&
                 small->h == (big->h - py) / sy + 1 && small->w == (big->w - px) / sx + 1,
             "%s: (%d,%d,%d,%d,%d) pooled by %d,%d,%d stride %d,%d,%d is not (%d,%d,%d,%d,%d)", who,
             big->n, big->c, big->d, big->h, big->w, pz, py, px, sz, sy, sx, small->n, small->c,
             small->d, small->h, small->w);
  E2_REQUIRE((unsigned long long)big->d * big->h * big->w < (1ull << 31),
             "%s: a channel of (%d,%d,%d,%d,%d) holds 2^31 elements or more", who, big->n, big->c,
             big->d, big->h, big->w);
  // (32-bit index math: 5 * extent stays below 2^31)
  E2_REQUIRE(big->d < (1 << 28) && big->h < (1 << 28) && big->w < (1 << 28),
             "%s: feature map too large", who);
  return 0;
}

// src is read, dst is written
PoolP mk_params(e2_ctx* ctx, const e2_tensor5* src, const e2_tensor5* dst, int pz, int py, int px,
                int sz, int sy, int sx, int mode, dim3* grid) {
  PoolP p = PoolP{};
  p.s = src->ptr; p.o = dst->ptr;
  p.sn = (long)src->sn; p.sc = (long)src->sc; p.sd = (long)src->sd; p.sh = (long)src->sh;
  p.on = (long)dst->sn; p.oc = (long)dst->sc; p.od = (long)dst->sd; p.oh = (long)dst->sh;
  p.W = (unsigned)dst->w; p.H = (unsigned)dst->h; p.D = (unsigned)dst->d;
  p.sW = (unsigned)src->w; p.sH = (unsigned)src->h; p.sD = (unsigned)src->d;
  p.pz = (unsigned)pz; p.py = (unsigned)py; p.px = (unsigned)px;
  // a stride beyond the unpooled extent leaves one output, as the extent itself does
  p.tz = (unsigned)min(sz, max(src->d, dst->d));
  p.ty = (unsigned)min(sy, max(src->h, dst->h));
  p.tx = (unsigned)min(sx, max(src->w, dst->w));
  p.quads = (p.W + 3) / 4 + 1;
  const unsigned long long items = (unsigned long long)p.D * p.H * p.quads;
  p.items = (unsigned)items;
  p.dq = mk_div(p.quads); p.dh = mk_div(p.H);
  p.dtz = mk_div(p.tz); p.dty = mk_div(p.ty); p.dtx = mk_div(p.tx);
  p.scale = mode == E2_POOL_AVG ? 1.0f / (float)((long)pz * py * px) : 1.0f;
  p.chunk = stream_chunk(ctx, (unsigned long long)dst->n * dst->c, items, 8, 8);
  *grid = dim3((unsigned)((items + p.chunk - 1) / p.chunk), (unsigned)dst->c, (unsigned)dst->n);
  return p;
}

}  // namespace

extern "C" int e2_pool3d_lin_fwd(e2_ctx* ctx, const e2_tensor5* x, int pz, int py, int px, int sz,
                                 int sy, int sx, int mode, const e2_tensor5* out) {
  const char* who = "e2_pool3d_lin_fwd";
  E2_REQUIRE(ctx, "%s: null ctx", who);
  if (int rc = check_view(x, "e2_pool3d_lin_fwd x")) return rc;
  if (int rc = check_view(out, "e2_pool3d_lin_fwd out")) return rc;
  if (int rc = geometry_ok(who, x, out, pz, py, px, sz, sy, sx, mode)) return rc;
  E2_REQUIRE(((unsigned long long)out->d * out->h) * ((unsigned long long)(out->w + 3) / 4 + 1) <
                 (1ull << 31), "%s: feature map too large", who);
  dim3 grid;
  const PoolP p = mk_params(ctx, x, out, pz, py, px, sz, sy, sx, mode, &grid);
  // the fixed-window instantiations: (2,2,2) and (1,2,2) with the stride of the window
  const bool tiled = pz == sz && py == sy && px == sx;
  const int fixed = (tiled && px == 2 && py == 2 && pz <= 2) ? pz : 0;
#define E2_POOL_FWD(M, FZ, FY) \
  hipLaunchKernelGGL((e2pool_lin_fwd_kernel<M, FZ, FY>), grid, dim3(256), 0, ctx->stream, p)
  if (mode == E2_POOL_AVG) {
    if (fixed == 2) E2_POOL_FWD(E2_POOL_AVG, 2, 2);
    else if (fixed == 1) E2_POOL_FWD(E2_POOL_AVG, 1, 2);
    else E2_POOL_FWD(E2_POOL_AVG, 0, 0);
  } else {
    if (fixed == 2) E2_POOL_FWD(E2_POOL_SUM, 2, 2);
    else if (fixed == 1) E2_POOL_FWD(E2_POOL_SUM, 1, 2);
    else E2_POOL_FWD(E2_POOL_SUM, 0, 0);
  }
#undef E2_POOL_FWD
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int e2_pool3d_lin_bwd(e2_ctx* ctx, const e2_tensor5* dout, int pz, int py, int px,
                                 int sz, int sy, int sx, int mode, const e2_tensor5* dx,
                                 int accumulate) {
  const char* who = "e2_pool3d_lin_bwd";
  E2_REQUIRE(ctx, "%s: null ctx", who);
  if (int rc = check_view(dout, "e2_pool3d_lin_bwd dout")) return rc;
  if (int rc = check_view(dx, "e2_pool3d_lin_bwd dx")) return rc;
  if (int rc = geometry_ok(who, dx, dout, pz, py, px, sz, sy, sx, mode)) return rc;
  E2_REQUIRE(((unsigned long long)dx->d * dx->h) * ((unsigned long long)(dx->w + 3) / 4 + 1) <
                 (1ull << 31), "%s: feature map too large", who);
  dim3 grid;
  PoolP p = mk_params(ctx, dout, dx, pz, py, px, sz, sy, sx, mode, &grid);
  p.accumulate = accumulate ? 1 : 0;
  const bool tiled = pz == sz && py == sy && px == sx;
#define E2_POOL_BWD(M, T) \
  hipLaunchKernelGGL((e2pool_lin_bwd_kernel<M, T>), grid, dim3(256), 0, ctx->stream, p)
  if (mode == E2_POOL_AVG) {
    if (tiled) E2_POOL_BWD(E2_POOL_AVG, true); else E2_POOL_BWD(E2_POOL_AVG, false);
  } else {
    if (tiled) E2_POOL_BWD(E2_POOL_SUM, true); else E2_POOL_BWD(E2_POOL_SUM, false);
  }
#undef E2_POOL_BWD
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}
