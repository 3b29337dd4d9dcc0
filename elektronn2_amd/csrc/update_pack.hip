// update_pack.hip -- the Adam update of optimiser.py:301-329 WRITING the packed weight images
// (VERDICT r3 / r4 lever "Adam writing the packed images"; e2hip.h e2_adam_pack_step).
//
// Until round 5 a training step ran two memory-bound launches over the weights: adam_kernel
// (p, g, m, s read; p, m, s written, g cleared: 28 B per parameter) and, at the head of the next
// step, pack_multi_kernel (p read again, the forward and the data-gradient image of every conv
// written: 8-12 B per parameter with the fetched padding) -- 10.5 + 14.5 us of neuro3d_lite's
// 1.52 ms, 19.3 + 31.9 us of neuro3d's 1.74 ms.  Here a work-group owns a TILE of one conv's
// weight tensor -- 32 output channels x IC input channels x the taps of one kernel plane --,
// applies the update to it (AdamRule of opt_rules.hpp, the rule adam_kernel runs: results are
// bit-identical), keeps the new values in LDS and writes them a second and third time as the
// tile of the forward image Wp[dz][ci / 4][t][ci % 4][co] (taps flipped) and of the
// data-gradient image Wp[dz][co / 4][t][co % 4][ci]: both along their contiguous axis, 128 B per
// 32 lanes.  The padding rows / columns the GEMMs fetch are rewritten as zeros exactly where
// pack_multi_kernel rewrites them (they must stay warm in the memory-side cache, DESIGN finding
// 11).  Parameters without images (biases, the fused first layer, the head, UpConv) take the
// plain path in the same launch.  The images are bit-identical to pack_multi_kernel's
// (tests/test_ops_gpu.py::test_adam_step_that_writes_the_packed_images).
//
// MEASURED (round 5, tools/upd_bench.py, tools/ab_opt.sh; DESIGN finding 46): parity-green and
// SLOWER than the two launches -- isolated 27.6 vs 9.8 + 14.2 us (neuro3d_lite), 63 vs 17.6 + 32.4
// us (neuro3d), 130 vs 37.5 + 59 us (unet3d_lite); in the captured step +52 / +100 us in its first
// cut (256 threads, loads and stores interleaved), about +4 / +14 us as it stands.  A tile can be
// read along ONE contiguous axis only: the update through tiles streams at 1.8 TB/s where
// adam_kernel's float4 sweep reaches 4.6 TB/s (42 vs 17.6 us without the image writes), and the
// image writes alone take what pack_multi_kernel takes (36 us with zeros as source).  Kept as an
// entry point, plan option adam_pack OFF.
#include "stream_common.hpp"
#include "opt_rules.hpp"
#include <algorithm>

namespace {

// (signed operands below 2^31: the tile and element indices of the kernel are ints)
__device__ __forceinline__ int udiv(int n, const FastDiv& f) {
  return (int)fdiv((unsigned)n, f);
}

struct UpdJob {
  long off;                 // element offset of w[cout][cin][kd][kh][kw] in the arenas
  float* wpF;               // forward image or nullptr
  float* wpD;               // data-gradient image or nullptr
  int cout, cin, kd, THW;
  int nCGF, coPF, coWF, icWF;   // forward image: channel groups per plane, row length, written extents
  int nCGD, coPD, coWD, icWD;   // data-gradient image (rows = cin, k channels = cout)
  int IC;                   // input channels per tile
  int nOT, nIT;             // tiles along cout / cin (x kd planes)
  int tile0;                // first tile of this job in the launch's tile sequence
  float reg;                // weight-decay multiplier of the tensor (0: none)
  FastDiv dKT, dTHW, dIC, dOT, dOTIT;
};

struct UpdRest { long off, n; float reg; int pad; };

constexpr int kMaxJobs = 96;
constexpr int kUT = 1024;     // threads per work-group: a tile's update is a chain of load -> compute -> store
                              // trips per thread, and what hides their latency is threads (two work-groups per CU)

__global__ __launch_bounds__(kUT) void adam_pack_kernel(float* __restrict__ p, float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ s,
                                                        const UpdJob* __restrict__ jobs, int njobs, int ntiles,
                                                        const UpdRest* __restrict__ rest, int nrest,
                                                        float* __restrict__ hyper,
                                                        const float* __restrict__ gdiv, float gmul, int zero_g) {
  extern __shared__ __attribute__((aligned(16))) float tile[];
  __shared__ int jt0[kMaxJobs + 1];
  for (int i = threadIdx.x; i <= njobs; i += kUT) jt0[i] = i < njobs ? jobs[i].tile0 : ntiles;
  const AdamRule rule(hyper);
  const float gs = gdiv ? gmul / (gdiv[0] + 1e-5f) : gmul;
  const int tid = threadIdx.x;
  __syncthreads();
  int ji = 0;
  for (int tl_ = blockIdx.x; tl_ < ntiles; tl_ += gridDim.x) {
    while (tl_ >= jt0[ji + 1]) ++ji;                   // (tiles ascend: the scan only moves forward)
    const UpdJob j = jobs[ji];
    const int lt = tl_ - j.tile0;
    const int dz = udiv(lt, j.dOTIT);
    const int r2 = lt - dz * (j.nOT * j.nIT);
    const int it = udiv(r2, j.dOT), ot = r2 - it * j.nOT;
    const int oc0 = ot * 32, ic0 = it * j.IC;
    const int THW = j.THW, T = j.kd * THW, KT = j.IC * THW;
    const int SI = THW * 33 + 1;                       // LDS stride of an input channel
    // a tile that holds neither weights nor padding anyone fetches
    const bool anyF = j.wpF && oc0 < j.coWF && ic0 < j.icWF;
    const bool anyD = j.wpD && ic0 < j.coWD && oc0 < j.icWD;
    if (!anyF && !anyD) continue;
    const float mult = rule.mult(j.reg);
    const bool real = oc0 < j.cout && ic0 < j.cin;     // (else: padding only -- zeros, no LDS trip)
    // ---- the update, tensor order: consecutive threads walk (ci, tap) of one output channel.
    // U elements per thread and trip, every load issued before the first store: g is read AND
    // cleared here, and a load behind a store to the same array waits for it (lesson of finding 43)
    if (real) {
      constexpr int U = 4;
      for (int e0 = tid; e0 < 32 * KT; e0 += kUT * U) {
        long ix[U]; int la[U]; bool ok[U];
        float gv[U], pv[U], ms[U][2];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int e = e0 + kUT * u;
          const int ol = udiv(e, j.dKT), k = e - ol * KT;
          const int il = udiv(k, j.dTHW), tt = k - il * THW;
          const int co = oc0 + ol, ci = ic0 + il;
          la[u] = il * SI + tt * 33 + ol;
          ok[u] = e < 32 * KT && co < j.cout && ci < j.cin;
          ix[u] = j.off + ((long)co * j.cin + ci) * T + dz * THW + tt;
          if (e >= 32 * KT) la[u] = -1;
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (ok[u]) { gv[u] = g[ix[u]]; pv[u] = p[ix[u]]; ms[u][0] = m[ix[u]]; ms[u][1] = s[ix[u]]; }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          float v = 0.f;
          if (ok[u]) {
            float gq = gv[u];
            if (gs != 1.f) gq *= gs;
            rule.apply(pv[u], gq, ms[u], mult);
            v = pv[u];
            p[ix[u]] = pv[u]; m[ix[u]] = ms[u][0]; s[ix[u]] = ms[u][1];
            if (zero_g) g[ix[u]] = 0.f;
          }
          if (la[u] >= 0) tile[la[u]] = v;
        }
      }
    }
    if (real) __syncthreads();
    // ---- forward image: 32 consecutive output channels per (ci, tap), taps flipped -----------
    if (anyF) {
      for (int f = tid; f < 32 * KT; f += kUT) {
        const int ol = f & 31, kk = f >> 5;
        const int il = udiv(kk, j.dTHW), tt = kk - il * THW;
        const int co = oc0 + ol, ci = ic0 + il;
        if (co < j.coWF && ci < j.icWF) {
          const int tlF = T - 1 - (dz * THW + tt);
          const int dzF = udiv(tlF, j.dTHW), tF = tlF - dzF * THW;
          j.wpF[((((long)dzF * j.nCGF + (ci >> 2)) * THW + tF) * 4 + (ci & 3)) * j.coPF + co] =
              real ? tile[il * SI + tt * 33 + ol] : 0.f;
        }
      }
    }
    // ---- data-gradient image: IC consecutive input channels per (co, tap) ---------------------
    if (anyD) {
      for (int f = tid; f < 32 * KT; f += kUT) {
        const int r = udiv(f, j.dIC), il = f - r * j.IC;
        const int ol = r & 31, tt = r >> 5;
        const int co = oc0 + ol, ci = ic0 + il;
        if (ci < j.coWD && co < j.icWD)
          j.wpD[((((long)dz * j.nCGD + (co >> 2)) * THW + tt) * 4 + (co & 3)) * j.coPD + ci] =
              real ? tile[il * SI + tt * 33 + ol] : 0.f;
      }
    }
    if (real) __syncthreads();
  }
  // ---- everything without images: the plain update ------------------------------------------
  for (int r = 0; r < nrest; ++r) {
    const UpdRest q = rest[r];
    const float mult = rule.mult(q.reg);
    for (long i = blockIdx.x * (long)kUT + tid; i < q.n; i += (long)gridDim.x * kUT) {
      const long a = q.off + i;
      float gv = g[a];
      if (gs != 1.f) gv *= gs;
      if (zero_g) g[a] = 0.f;
      float pv = p[a], ms[2] = {m[a], s[a]};
      rule.apply(pv, gv, ms, mult);
      p[a] = pv; m[a] = ms[0]; s[a] = ms[1];
    }
  }
  // publish t once every work-group has read the old value.  Up to 4 x CUs work-groups: 16
  // sub-counters (<= 64 arrivals each) whose last arrivers meet on the top counter -- a thousand
  // arrivals on ONE address serialise for tens of microseconds (finding 6)
  __syncthreads();
  if (tid == 0) {
    unsigned* top = reinterpret_cast<unsigned*>(hyper + 7);
    unsigned* sub = reinterpret_cast<unsigned*>(hyper + 8) + (blockIdx.x & 15);
    const unsigned nsub = (gridDim.x + 15 - (blockIdx.x & 15)) >> 4;     // work-groups on this sub-counter
    const unsigned prev = __hip_atomic_fetch_add(sub, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (prev == nsub - 1) {
      __hip_atomic_store(sub, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const unsigned ntop = gridDim.x < 16 ? gridDim.x : 16;
      const unsigned pt = __hip_atomic_fetch_add(top, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (pt == ntop - 1) {
        __hip_atomic_store(top, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        rule.publish(hyper);
      }
    }
  }
}

int tile_ic(int THW) {
  int ic = 32;
  while (ic > 1 && (size_t)ic * (THW * 33 + 1) * 4 > 40 * 1024) ic >>= 1;
  return ic;
}

}  // namespace

extern "C" size_t e2_upd_job_bytes(void) { return sizeof(UpdJob); }
extern "C" size_t e2_upd_rest_bytes(void) { return sizeof(UpdRest); }

/* fill one host-side record of e2_adam_pack_step: the conv weight tensor w[cout][cin][kd][kh][kw]
 * at element offset `off` of the parameter arena, its forward image wp_f and / or data-gradient
 * image wp_d (e2_conv3d_pack modes 0 / 1; either may be NULL), reg = the tensor's weight-decay
 * multiplier (apply_reg; 0 = none), tile0 = the number of tiles of the records before it;
 * *ntiles receives this record's tile count, *lds_bytes the LDS a launch holding it needs. */
extern "C" int e2_upd_job_fill(void* rec, long off, void* wp_f, void* wp_d, int cout, int cin, int kd,
                               int kh, int kw, float reg, int tile0, int* ntiles, size_t* lds_bytes) {
  E2_REQUIRE(rec && ntiles && lds_bytes && (wp_f || wp_d) && cout > 0 && cin > 0 && kd > 0 && kh > 0 && kw > 0,
             "upd_job_fill: bad argument");
  E2_REQUIRE(kh * kw <= 2048, "upd_job_fill: kernel plane of %d taps", kh * kw);
  UpdJob* j = (UpdJob*)rec;
  j->off = off; j->wpF = (float*)wp_f; j->wpD = (float*)wp_d;
  j->cout = cout; j->cin = cin; j->kd = kd; j->THW = kh * kw;
  int ciP, coP;
  e2i_pack_dims(cout, cin, &ciP, &coP);                 // forward image (rows cout, k channels cin)
  j->nCGF = ciP >> 2; j->coPF = coP;
  j->coWF = std::min(coP, ((cout + 15) / 16) * 16 + 96);
  j->icWF = 4 * std::min(ciP >> 2, ((cin + 3) >> 2) + 4);
  e2i_pack_dims(cin, cout, &ciP, &coP);                 // data-gradient image (rows cin, k channels cout)
  j->nCGD = ciP >> 2; j->coPD = coP;
  j->coWD = std::min(coP, ((cin + 15) / 16) * 16 + 96);
  j->icWD = 4 * std::min(ciP >> 2, ((cout + 3) >> 2) + 4);
  j->IC = tile_ic(j->THW);
  const int ocR = std::max(wp_f ? j->coWF : 0, wp_d ? j->icWD : 0);
  const int icR = std::max(wp_f ? j->icWF : 0, wp_d ? j->coWD : 0);
  j->nOT = (std::max(ocR, cout) + 31) / 32;
  j->nIT = (std::max(icR, cin) + j->IC - 1) / j->IC;
  j->tile0 = tile0; j->reg = reg;
  j->dKT = mk_div(j->IC * j->THW); j->dTHW = mk_div(j->THW); j->dIC = mk_div(j->IC);
  j->dOT = mk_div(j->nOT); j->dOTIT = mk_div(j->nOT * j->nIT);
  const long nt = (long)j->nOT * j->nIT * kd;
  E2_REQUIRE(nt + tile0 < (1L << 30) && (long)32 * j->IC * j->THW < (1L << 30), "upd_job_fill: tensor too large");
  *ntiles = (int)nt;
  *lds_bytes = (size_t)j->IC * (j->THW * 33 + 1) * 4;
  return 0;
}

extern "C" int e2_upd_rest_fill(void* rec, long off, long n, float reg) {
  E2_REQUIRE(rec && off >= 0 && n >= 0, "upd_rest_fill: bad argument");
  UpdRest* q = (UpdRest*)rec;
  q->off = off; q->n = n; q->reg = reg; q->pad = 0;
  return 0;
}

/* optimiser.py:301-329 (Adam: eps 1e-5 inside the sqrt, bias factor, L2 outside the adaptive
 * term) for the whole parameter arena AND the repack of every conv's weight images, one launch:
 * jobs_dev = njobs records of e2_upd_job_fill (tiles ascending, ntiles in all), rest_dev = nrest
 * records of e2_upd_rest_fill covering every trainable element the jobs do not (each element
 * exactly once between the two lists -- the caller's contract), lds_bytes = the largest
 * *lds_bytes of the jobs.  hyper (24 floats here: [8..23] are arrival counters, zero at first) /
 * gdiv / gmul / zero_g as e2_adam_step_ex.  The update is
 * bit-identical to e2_adam_step_ex, the images to e2_conv3d_pack_multi's. */
extern "C" int e2_adam_pack_step(e2_ctx* ctx, float* p, float* g, float* m, float* s,
                                 const void* jobs_dev, int njobs, int ntiles, const void* rest_dev,
                                 int nrest, float* hyper, const float* gdiv, float gmul, int zero_g,
                                 size_t lds_bytes) {
  E2_REQUIRE(ctx && p && g && m && s && hyper && njobs >= 0 && nrest >= 0 && (njobs == 0 || jobs_dev) &&
                 (nrest == 0 || rest_dev), "adam_pack_step: null argument");
  E2_REQUIRE(njobs <= kMaxJobs, "adam_pack_step: %d conv tensors (at most %d)", njobs, kMaxJobs);
  E2_REQUIRE(lds_bytes <= 128 * 1024, "adam_pack_step: a tile of %zu bytes", lds_bytes);
  static bool attr_done = false;
  if (!attr_done) {
    E2_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&adam_pack_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));   // (+ the static job table)
    attr_done = true;
  }
  const int grid = std::max(1, std::min(std::max(ntiles, 1), 2 * ctx->num_cu));
  hipLaunchKernelGGL(adam_pack_kernel, dim3(grid), dim3(kUT), std::max<size_t>(lds_bytes, 16), ctx->stream,
                     p, g, m, s, (const UpdJob*)jobs_dev, njobs, ntiles, (const UpdRest*)rest_dev, nrest,
                     hyper, gdiv, gmul, zero_g ? 1 : 0);
  E2_CHECK_HIP(hipGetLastError());
  return 0;
}
