// body of softmax_nll_fwd_kernel / softmax_nll_fwd_w_kernel and of
// softmax_nll_grouped_fwd_kernel (softmax_nll.hip): in scope are the flags WT and HAS_T (false:
// no target, probabilities only), the kernel's arguments and `NllW wt`.
  __shared__ float red[4];
  const long S = (long)lg.d * lg.h * lg.w;
  const long s = blockIdx.x * 256L + threadIdx.x;
  const int n = blockIdx.z;
  float lsum = 0.f, nlab = 0.f;
  if (s < S) {
    const int x = (int)(s % lg.w);
    const long t = s / lg.w;
    const int y = (int)(t % lg.h), z = (int)(t / lg.h);
    const float* lp = lg.p + vidx(lg, n, 0, z, y, x);
    float m = lp[0];
    for (int c = 1; c < lg.c; ++c) m = fmaxf(m, lp[c * lg.sc]);
    float den = 0.f;
    for (int c = 0; c < lg.c; ++c) den += expf(lp[c * lg.sc] - m);
    const float tv = HAS_T ? tg.p[vidx(tg, n, 0, z, y, x)] : -1.f;
    float* pp = pr.p + vidx(pr, n, 0, z, y, x);
    float ev = 1.f;
    if constexpr (WT) {
      if (wt.ew) ev = wt.ew[(long)n * wt.esN + (long)z * wt.esD + (long)y * wt.esH + x];
    }
    for (int c = 0; c < lg.c; ++c) {
      const float pc = expf(lp[c * lg.sc] - m) / den;
      pp[c * pr.sc] = pc;
      if constexpr (!WT) {
        if (tv == (float)c) { lsum -= logf(pc + E2_EPS_NLL); nlab += 1.f; }
      } else {
        const float wc = wt.cw ? e2_uniform_ld(wt.cw, c) : 1.f;     // (uniform indices: scalar loads)
        const float Lc = wt.lab ? e2_uniform_ld(wt.lab, n * lg.c + c) : 1.f;
        const float Mc = wt.npr ? e2_uniform_ld(wt.npr, n * lg.c + c) : 0.f;
        if (tv == (float)c) { lsum -= (Lc * wc * ev) * logf(pc + E2_EPS_NLL); nlab += Lc; }
        if (Mc != 0.f) {                                               // (uniform branch)
          float oth = 0.f;
          for (int k = 0; k < lg.c; ++k)
            if (k != c) oth += expf(lp[k * lg.sc] - m);
          lsum -= (Mc * wc * ev) * logf(oth / den + E2_EPS_NLL);
        }
      }
    }
  }
  const float a = block_sum256(lsum, red);
  float b = block_sum256(nlab, red);
  if (threadIdx.x == 0) {
    if constexpr (WT) {
      if (wt.npr && blockIdx.x == 0 && blockIdx.z == 0) {
        float sm = 0.f;
        for (int i = 0; i < lg.n * lg.c; ++i) sm += e2_uniform_ld(wt.npr, i);
        b += (float)S * sm;
      }
    }
    if (a != 0.f) unsafeAtomicAdd(stats + 0, a);
    if (b != 0.f) unsafeAtomicAdd(stats + 1, b);
  }
