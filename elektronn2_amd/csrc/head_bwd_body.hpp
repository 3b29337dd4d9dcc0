// head_bwd_body.hpp -- body of head_bwd_kernel / head_bwd_w_kernel (head.hip): in scope are NC, the
// flag WT, the kernel's arguments and `NllW wt`.
  extern __shared__ float hs[];
  const int C = x.c;
  float* dl = hs;                         // [NC][HT]
  float* xs = hs + NC * HT;               // [C][HT + 1]
  const int tid = threadIdx.x;
  const int S = x.d * x.h * x.w;
  float inv = 1.f / (stats[1] + E2_EPS_NLL);
  if (blockIdx.x == 0 && tid == 0 && loss_out) loss_out[0] = stats[0] * inv;
  if (blockIdx.x == 0 && tid == 0 && count_out) count_out[0] = stats[1];
  if (sum_mode) inv = 1.f;                  // (e2_set_loss_grad_mode: unnormalised gradients)
  // thread ci < C (two rounds when C > 256) owns dW[c][ci]
  float aw[2][NC];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < NC; ++c) aw[r][c] = 0.f;
  float ab[NC];                           // dbias partials of threads 0..HT-1
#pragma unroll
  for (int c = 0; c < NC; ++c) ab[c] = 0.f;

  for (int tile = blockIdx.x; tile < nTiles; tile += gridDim.x) {
    const int n = tile / tilesPerN;
    const int s0 = (tile - n * tilesPerN) * HT;
    const int np = min(HT, S - s0);
    // dlogits of the tile's positions
    if (tid < HT) {
      float d[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) d[c] = 0.f;
      if (tid < np) {
        const int s = s0 + tid;
        const int xx = s % x.w;
        const int t = s / x.w;
        const int y = t % x.h, z = t / x.h;
        const float tv = tg.p[hidx(tg, n, z, y, xx)];
        const float* pp = pr.p + hidx(pr, n, z, y, xx);
        float pc[NC], pt = 0.f;
        int tc = -1;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          pc[c] = pp[(long)c * pr.sc];
          if (tv == (float)c) { tc = c; pt = pc[c]; }
        }
        if constexpr (!WT) {
        // dL/dp_t = -inv/(p_t+eps);  dlogit_c = p_c*(dp_c - sum_k dp_k p_k)
        const float gpt = (tc >= 0) ? (-inv / (pt + E2_EPS_NLL)) * pt : 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) d[c] = gpt * ((c == tc ? 1.f : 0.f) - pc[c]);
        } else {
          const HeadW<NC> hw = head_w_load<NC>(wt, n);       // (n is uniform: scalar loads)
          const float ev = wt.ew ? wt.ew[(long)n * wt.esN + (long)z * wt.esD + (long)y * wt.esH + xx] : 1.f;
          head_w_dlogits<NC>(hw, pc, tv, ev * inv, d);
        }
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) { dl[c * HT + tid] = d[c]; ab[c] += d[c]; }
    }
    // the input tile, coalesced: 256/HT channel rows of HT positions per pass
    const int p = tid & (HT - 1);
    int pz = 0, py = 0, px = 0;
    if (p < np) {
      const int s = s0 + p;
      px = s % x.w;
      const int t = s / x.w;
      py = t % x.h; pz = t / x.h;
    }
    {
      const long off = hidx(x, n, pz, py, px);
      const bool pv = p < np;
#pragma unroll 8
      for (int ci = tid / HT; ci < C; ci += 256 / HT)
        xs[ci * (HT + 1) + p] = pv ? x.p[off + (long)ci * x.sc] : 0.f;
    }
    __syncthreads();
    // dW partial sums: thread = input channel
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int ci = tid + 256 * r;
      if (ci < C) {
        const float* row = xs + ci * (HT + 1);
        for (int p = 0; p < HT; ++p) {
          const float v = row[p];
#pragma unroll
          for (int c = 0; c < NC; ++c) aw[r][c] = fmaf(dl[c * HT + p], v, aw[r][c]);
        }
      }
    }
    // dx = W^T dlogits, written (or accumulated) coalesced
    if (want_dx) {
      if (p < np) {
        float* dp = dx.p + hidx(dx, n, pz, py, px);
        float d[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) d[c] = dl[c * HT + p];
#pragma unroll 8
        for (int ci = tid / HT; ci < C; ci += 256 / HT) {
          float g = 0.f;
#pragma unroll
          for (int c = 0; c < NC; ++c) g = fmaf(w[c * C + ci], d[c], g);
          float* q = dp + (long)ci * dx.sc;
          *q = accumulate ? (*q + g) : g;
        }
      }
    }
    __syncthreads();
  }
  // flush: this work-group's partial sums, part[block][NC*C + NC] (plain stores; 400+
  // same-address atomics per address serialise for tens of microseconds)
  float* mine = part + (long)blockIdx.x * (NC * C + NC);
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int ci = tid + 256 * r;
    if (ci < C) {
#pragma unroll
      for (int c = 0; c < NC; ++c) mine[c * C + ci] = aw[r][c];
    }
  }
  if (tid < 64) {           // wave 0 (threads >= HT hold zeros)
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const float sb = wave_sum(ab[c]);
      if (tid == 0) mine[NC * C + c] = sb;
    }
  }
