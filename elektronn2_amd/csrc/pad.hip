// pad.hip -- constant padding of a strided 5-D view (e2_pad5): the device side of the Pad node
// (neural.py:1195-1279) and of the zero frame the 'same' / 'full' conv modes put around their
// input (computations.py:287-291,320-326; the valid conv kernels then run on the framed image).
//
//   dst[n, c, z, y, x] = src[n, c, z - pz, y - py, x - px]   inside the interior
//                      = value                                 in the frame
//
// dst sizes = src sizes + 2 (pz, py, px) on (d, h, w).  One launch, one pass over dst; the
// frame-only form writes the frame and leaves the interior (and src, which may be NULL) alone.
//
// Geometry of act.hip / loss_elem.hip: a work-group stays inside one (n, c), a thread owns FOUR
// consecutive x of one dst row.  The quads are cut where the DESTINATION row is 16-byte aligned
// (a row that starts m elements behind a 16-byte boundary gets a short first quad of 4 - m), so
// every whole quad is one 16-byte store; the source row is shifted by px elements against it and
// is fetched as one 16-byte load only where it happens to be aligned too, element by element
// otherwise and at row ends.  Spatial axes that carry no x padding and are dense in both views
// are collapsed on the host: rows of w with (py, 0) padding become one row of h * w with
// py * w padding elements at either end.  Nothing outside the dst view is written, nothing
// outside the src view is read.  Pure stream: no LDS, no workspace.
#include "stream_common.hpp"

namespace {

// the (d, h, w) block of one (n, c) of dst after the host's collapse
struct PadP {
  const float* s;
  float* o;
  long sn, sc, sd, sh;          // src strides: batch, feature, d, h
  long on, oc, od, oh;          // dst strides
  unsigned W, H, D;             // dst extents
  unsigned px, py, pz;          // frame widths
  unsigned quads;               // quads provided per dst row: (W + 3) / 4 + 1
  unsigned items;               // D * H * quads  (< 2^31)
  unsigned chunk;               // items per work-group, a multiple of 256
  FastDiv dq, dh;
  float value;
};

typedef float pad_f4 __attribute__((ext_vector_type(4)));

template <bool FRAME_ONLY>
__global__ __launch_bounds__(256) void e2pad_kernel(PadP p) {
  const unsigned s0 = blockIdx.x * p.chunk;
  const unsigned s1 = min(s0 + p.chunk, p.items);
  const unsigned c = blockIdx.y, n = blockIdx.z;
  const float* sbase = FRAME_ONLY ? nullptr : p.s + (long)n * p.sn + (long)c * p.sc;
  float* obase = p.o + (long)n * p.on + (long)c * p.oc;
  const unsigned xi1 = p.W - p.px;                  // interior: px <= x < xi1
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
    const bool row_in = z >= p.pz && z < p.D - p.pz && y >= p.py && y < p.H - p.py;
    const bool whole = (x1 - x0) == 4u;
    const bool all_in = row_in && x0 >= p.px && x1 <= xi1;
    if (FRAME_ONLY) {
      if (all_in) continue;
      if (whole && !(row_in && x1 > p.px && x0 < xi1)) {     // a quad of frame alone
        pad_f4 r;
        r[0] = r[1] = r[2] = r[3] = p.value;
        *reinterpret_cast<pad_f4*>(drow + x0) = r;
      } else {
        for (unsigned x = x0; x < x1; ++x)
          if (!(row_in && x >= p.px && x < xi1)) drow[x] = p.value;
      }
      continue;
    }
    // the source row, addressed with dst's x: the pointer itself lies px elements in front of the
    // row (and is a dummy for frame rows) -- it is only dereferenced at interior coordinates,
    // px <= x < W - px of an interior row, which are inside the source view
    const float* srow = row_in ? sbase + (long)(z - p.pz) * p.sd + (long)(y - p.py) * p.sh - (long)p.px
                               : sbase;
    if (whole) {
      pad_f4 r;
      if (all_in && ((((uintptr_t)(srow + x0)) & 15) == 0)) {
        r = *reinterpret_cast<const pad_f4*>(srow + x0);
      } else {
#pragma unroll
        for (unsigned e = 0; e < 4; ++e) {
          const unsigned x = x0 + e;
          r[e] = (row_in && x >= p.px && x < xi1) ? srow[x] : p.value;
        }
      }
      *reinterpret_cast<pad_f4*>(drow + x0) = r;
    } else {
      for (unsigned x = x0; x < x1; ++x)
        drow[x] = (row_in && x >= p.px && x < xi1) ? srow[x] : p.value;
    }
  }
}

}  // namespace

extern "C" int e2_pad5(e2_ctx* ctx, const e2_tensor5* src, const e2_tensor5* dst, int pz, int py,
                       int px, float value, int frame_only) {
  E2_REQUIRE(ctx && dst && dst->ptr, "e2_pad5: null argument");
  E2_REQUIRE(frame_only || (src && src->ptr), "e2_pad5: null source");
  E2_REQUIRE(pz >= 0 && py >= 0 && px >= 0, "e2_pad5: negative padding %d,%d,%d", pz, py, px);
  E2_REQUIRE(dst->n > 0 && dst->c > 0 && dst->d > 2 * pz && dst->h > 2 * py && dst->w > 2 * px,
             "e2_pad5: destination (%d,%d,%d,%d,%d) has no interior for padding %d,%d,%d", dst->n,
             dst->c, dst->d, dst->h, dst->w, pz, py, px);
  if (src)
    E2_REQUIRE(src->n == dst->n && src->c == dst->c && src->d + 2 * pz == dst->d &&
                   src->h + 2 * py == dst->h && src->w + 2 * px == dst->w,
               "e2_pad5: sizes (%d,%d,%d,%d,%d) + 2 * (%d,%d,%d) != (%d,%d,%d,%d,%d)", src->n, src->c,
               src->d, src->h, src->w, pz, py, px, dst->n, dst->c, dst->d, dst->h, dst->w);
  E2_REQUIRE(dst->c <= 65535 && dst->n <= 65535, "e2_pad5: more than 65535 features / batch entries");
  unsigned long long W = (unsigned long long)dst->w, H = (unsigned long long)dst->h,
                     D = (unsigned long long)dst->d;
  unsigned long long qx = (unsigned long long)px, qy = (unsigned long long)py,
                     qz = (unsigned long long)pz;
  long ssd = src ? (long)src->sd : 0, ssh = src ? (long)src->sh : 0;
  long osd = (long)dst->sd, osh = (long)dst->sh;
  // a row axis joins x where x carries no padding and the rows follow each other without a gap in
  // both views: its padding becomes whole rows' worth of x padding
  for (int pass = 0; pass < 2; ++pass) {
    const bool dense = (H == 1 || (osh == (long)W && (!src || ssh == (long)W)));
    if (!(qx == 0 && dense && W * H < (1ull << 30))) break;
    qx = qy * W; W *= H;
    H = D; qy = qz; D = 1; qz = 0;
    osh = osd; ssh = ssd; osd = 0; ssd = 0;
  }
  const unsigned long long quads = (W + 3) / 4 + 1, items = D * H * quads;
  E2_REQUIRE(W < (1ull << 30) && items < (1ull << 31), "e2_pad5: feature map too large");
  PadP p = PadP{};
  p.s = src ? src->ptr : nullptr; p.o = dst->ptr;
  p.sn = src ? (long)src->sn : 0; p.sc = src ? (long)src->sc : 0; p.sd = ssd; p.sh = ssh;
  p.on = (long)dst->sn; p.oc = (long)dst->sc; p.od = osd; p.oh = osh;
  p.W = (unsigned)W; p.H = (unsigned)H; p.D = (unsigned)D;
  p.px = (unsigned)qx; p.py = (unsigned)qy; p.pz = (unsigned)qz;
  p.quads = (unsigned)quads; p.items = (unsigned)items;
  p.dq = mk_div(p.quads); p.dh = mk_div(p.H);
  p.value = value;
  p.chunk = stream_chunk(ctx, (unsigned long long)dst->n * dst->c, items, 8, 8);
  const dim3 grid((unsigned)((items + p.chunk - 1) / p.chunk), (unsigned)dst->c, (unsigned)dst->n);
  if (frame_only)
    hipLaunchKernelGGL((e2pad_kernel<true>), grid, dim3(256), 0, ctx->stream, p);
  else
    hipLaunchKernelGGL((e2pad_kernel<false>), grid, dim3(256), 0, ctx->stream, p);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}
