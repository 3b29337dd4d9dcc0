// body of softmax_nll_bwd_kernel / softmax_nll_bwd_w_kernel and of
// softmax_nll_grouped_bwd_kernel / nll_multi_bwd_kernel (softmax_nll.hip): in scope are the flags
// WT and COEF, the kernel's arguments and `NllW wt`.  COEF (e2_nll_multi_bwd): `stats` points at
// the finished coefficient of this loss term -- nothing is normalised or reported here.
  const long S = (long)pr.d * pr.h * pr.w;
  const long s = blockIdx.x * 256L + threadIdx.x;
  const int n = blockIdx.z;
  float inv;
  if constexpr (COEF) {
    inv = stats[0];
  } else {
    inv = 1.f / (stats[1] + E2_EPS_NLL);
    if (blockIdx.x == 0 && blockIdx.z == 0 && threadIdx.x == 0) {
      if (loss_out) loss_out[0] = stats[0] * inv;
      if (count_out) count_out[0] = stats[1];
    }
    if (sum_mode) inv = 1.f;                // (e2_set_loss_grad_mode: unnormalised gradients)
  }
  if (s >= S) return;
  const int x = (int)(s % pr.w);
  const long t = s / pr.w;
  const int y = (int)(t % pr.h), z = (int)(t / pr.h);
  const float tv = tg.p[vidx(tg, n, 0, z, y, x)];
  const float* pp = pr.p + vidx(pr, n, 0, z, y, x);
  float* dp = dl.p + vidx(dl, n, 0, z, y, x);
  if constexpr (!WT) {
    float pt = 0.f;
    int tc = -1;
    for (int c = 0; c < pr.c; ++c)
      if (tv == (float)c) { tc = c; pt = pp[c * pr.sc]; }
    // dL/dp_t = -inv/(p_t+eps);  dlogit_c = p_c*(dp_c - sum_k dp_k p_k)
    const float gpt = (tc >= 0) ? (-inv / (pt + E2_EPS_NLL)) * pt : 0.f;
    for (int c = 0; c < pr.c; ++c) {
      const float pc = pp[c * pr.sc];
      dp[c * dl.sc] = gpt * ((c == tc ? 1.f : 0.f) - pc);
    }
  } else {
    // g_c = dL/dp_c = (-[t == c] L w e / (p_c + eps) + M w e / (q_c + eps)) * inv, q_c = sum of the
    // other classes' probabilities;  dlogit_c = p_c (g_c q_c - sum_{k != c} g_k p_k): the form
    // without p_c g_c (1 - p_c).  Two sweeps over the classes (C is a run-time number here: no
    // register arrays): ascending leaves the prefix sums of g_k p_k in dlogits, descending adds
    // the suffix sums.
    float ev = inv;
    if (wt.ew) ev *= wt.ew[(long)n * wt.esN + (long)z * wt.esD + (long)y * wt.esH + x];
    auto gq = [&](int c, float& q) {          // g_c (q_c by the way)
      q = 0.f;
      for (int k = 0; k < pr.c; ++k)
        if (k != c) q += pp[k * pr.sc];
      const float wc = (wt.cw ? e2_uniform_ld(wt.cw, c) : 1.f) * ev;
      const float Lc = wt.lab ? e2_uniform_ld(wt.lab, n * pr.c + c) : 1.f;
      const float Mc = wt.npr ? e2_uniform_ld(wt.npr, n * pr.c + c) : 0.f;
      const float a = (tv == (float)c) ? Lc * wc : 0.f;
      return -a / (pp[c * pr.sc] + E2_EPS_NLL) + (Mc * wc) / (q + E2_EPS_NLL);
    };
    float run = 0.f;
    for (int c = 0; c < pr.c; ++c) {
      float q;
      const float g = gq(c, q);
      dp[c * dl.sc] = run;
      run += g * pp[c * pr.sc];
    }
    run = 0.f;
    for (int c = pr.c - 1; c >= 0; --c) {
      float q;
      const float g = gq(c, q);
      const float pc = pp[c * pr.sc];
      dp[c * dl.sc] = pc * (g * q - (dp[c * dl.sc] + run));
      run += g * pc;
    }
  }
