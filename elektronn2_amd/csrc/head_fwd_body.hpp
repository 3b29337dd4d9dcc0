// head_fwd_body.hpp -- body of head_fwd_kernel / head_fwd_w_kernel (head.hip): in scope are NC, the
// flag WT, the kernel's arguments and `NllW wt`.
  __shared__ float part[4][NC][64];
  const int S = x.d * x.h * x.w;
  const int p = threadIdx.x & 63, cq = threadIdx.x >> 6;
  const int s = blockIdx.x * 64 + p;
  const int n = blockIdx.z;
  const bool valid = s < S;
  int xx = 0, y = 0, z = 0;
  if (valid) {
    xx = s % x.w;
    const int t = s / x.w;
    y = t % x.h; z = t / x.h;
  }
  const int per = (x.c + 3) >> 2;
  const int c0 = cq * per, c1 = min(c0 + per, x.c);
  float acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.f;
  if (valid) {
    const float* xp = x.p + hidx(x, n, z, y, xx);
#pragma unroll 10
    for (int ci = c0; ci < c1; ++ci) {
      const float v = xp[(long)ci * x.sc];
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[c] = fmaf(w[c * x.c + ci], v, acc[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) part[cq][c][p] = acc[c];
  __syncthreads();
  if (cq != 0) return;
  float lsum = 0.f, nlab = 0.f;
  if (valid) {
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      acc[c] = ((part[0][c][p] + part[1][c][p]) + (part[2][c][p] + part[3][c][p])) + bias[c];
      m = fmaxf(m, acc[c]);
    }
    float den = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) den += expf(acc[c] - m);
    const float tv = has_target ? tg.p[hidx(tg, n, z, y, xx)] : -1.f;
    float* pp = pr.p + hidx(pr, n, z, y, xx);
    if constexpr (!WT) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const float pc = expf(acc[c] - m) / den;
      pp[(long)c * pr.sc] = pc;
      if (tv == (float)c) { lsum -= logf(pc + E2_EPS_NLL); nlab += 1.f; }
    }
    } else {
      const HeadW<NC> hw = head_w_load<NC>(wt, n);
      const float ev = wt.ew ? wt.ew[(long)n * wt.esN + (long)z * wt.esD + (long)y * wt.esH + xx] : 1.f;
      float ex[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        ex[c] = expf(acc[c] - m);
        pp[(long)c * pr.sc] = ex[c] / den;
      }
      lsum = head_w_loss<NC>(hw, ex, den, tv, ev, &nlab);
    }
  }
  if (has_target) {                       // wave 0 only
    const float a = wave_sum(lsum);
    float b = wave_sum(nlab);
    if constexpr (WT) {
      if (p == 0 && blockIdx.x == 0 && blockIdx.z == 0) b += head_w_count_dn(wt, x.n * NC, S);
    }
    if (p == 0) {
      if (a != 0.f) unsafeAtomicAdd(stats + 0, a);
      if (b != 0.f) unsafeAtomicAdd(stats + 1, b);
    }
  }
