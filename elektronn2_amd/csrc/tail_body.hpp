// tail_body.hpp -- the body of tail_kernel / tail_w_kernel (tail.hip includes it inside both):
// in scope are the template parameters WM, NC, KC, BF, the flag WT, `TailP p` and `NllW wt`.
  using G = Geo<WM, KC>;
  constexpr int kKC = KC;
  [[maybe_unused]] constexpr int WN = G::WN, NP = G::NP, NPP = G::NPP, MTW = G::MTW, BM = G::BM, BMS = G::BMS,
                NQ = G::NQ;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* T = lds;                                   // [TR][NPP]: x, then h, then dpre, then dx
  float* WB = lds + G::TILE_F;                      // 2 x [kKC][BMS] weight chunks
  float* PL = WB + 2 * G::WB_F;                     // [NQ][NC][NP] partial logits
  float* DL = PL + NQ * NC * NP;                    // [NC][NP] dlogits
  float* RED = DL + NC * NP;                        // scalars (16)
  float* WH = RED + 16;                             // [NC][kRows] head weights, then b1 [kRows]
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, kq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave % WM, wn = wave / WM;
  const int n = blockIdx.x / p.tilesPerN;
  const int s0 = (blockIdx.x - n * p.tilesPerN) * NP;
  const int np = min(NP, p.S - s0);
  const int pp = tid % NP, pq = tid / NP;           // (position, channel share) of the passes

  // ---- weight chunks: image rows [c * kKC, + kKC) x columns [0, BM) -> LDS by LDS-DMA --------
  constexpr int PIECES = kKC * BMS / 4;             // 16-byte pieces of a chunk, pad columns too
  constexpr int NI = (PIECES + 255) / 256;
  // piece pi = it * 256 + tid of a chunk [k][BMS]: image row k, columns 4 (pi % (BMS / 4)) ...
  // (pad columns re-read the row's last piece); offsets for both images, once
  int wrow[NI], woffF[NI], woffD[NI], wcol[NI];
#pragma unroll
  for (int it = 0; it < NI; ++it) {
    const int pi = min(it * 256 + tid, PIECES - 1);
    wrow[it] = (pi * 4) / BMS;
    wcol[it] = min(pi * 4 - wrow[it] * BMS, BM - 4);
    woffF[it] = wrow[it] * p.coPf + wcol[it];
    woffD[it] = wrow[it] * p.coPd + wcol[it];
  }
  // the K loop has ONE trip count -- whole chunks, no early exit around the hand-scheduled
  // steps (an exit per step made hipcc keep two sets of accumulators and move all 52
  // registers at every chunk boundary).  Chunk rows past the image (only where K padded to
  // whole chunks exceeds ciP) are never staged: both buffers are zeroed once instead.
  auto stage = [&](const float* img, int coP, int ciP, const int (&woff)[NI], int c, int buf) {
    const float* wc = img + (long)c * kKC * coP;
    unsigned char* lb = reinterpret_cast<unsigned char*>(WB + buf * G::WB_F) + (wave * 64) * 16;
#pragma unroll
    for (int it = 0; it < NI; ++it)
      // (selecting between the image and a zero block per piece made the DMA -- and every load
      // queued behind it -- 30 % slower: rows past the image are SKIPPED, their LDS rows are
      // zeroed once, below)
      if (it * 256 + tid < PIECES && c * kKC + wrow[it] < ciP)
        __builtin_amdgcn_global_load_lds((gbl_vp)(wc + woff[it]), (lds_vp)(lb + it * 256 * 16), 16, 0, 0);
  };
  // WT: the masks and class weights of this batch item (uniform addresses: scalar loads) and the
  // example weight of this lane's position are requested here, with the tile's loads, long before
  // the loss needs them (requested in the loss phase they were a round trip to memory in the one
  // wave every other wave of the work-group waits for)
  HeadW<NC> hw;
  float evw = 1.f;
  if constexpr (WT) {
    hw = head_w_load<NC>(wt, n);
    if (wt.ew && tid < np) evw = wt.ew[(long)n * wt.esN + s0 + tid];
  }
  TAIL_STAMP(0);
  if (p.zero_wb) {
    for (int i = tid; i < 2 * G::WB_F; i += 256) WB[i] = 0.f;
    __syncthreads();
  }
  stage(p.wpf, p.coPf, p.ciPf, woffF, 0, 0);

  // ---- the x tile -> LDS: rows of NP positions, zero past the sample and past C1; every load
  // of the tile is in flight at once ------------------------------------------------------------
  {
    const float* xb = p.x + (long)n * p.xsN + s0 + pp;
    const bool pv = pp < np;
    constexpr int NR = G::TR / NQ;
    static_assert(G::TR % NQ == 0, "tile rows per thread");
    float xv[NR];
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int r = pq + j * NQ;
      xv[j] = (pv && r < p.C1) ? xb[(long)r * p.xsC] : 0.f;
    }
    // (the count's loads are requested BEHIND the tile's: one round trip to memory for both)
    // ---- the labelled voxels of the whole target (every work-group for itself) -----------------
    float cnt = 0.f;
    if (p.count_here) {
      // (the first cut read one float per iteration: 54 dependent round trips to L2 = ~35 us of
      // the kernel on neuro3d_lite's 13,690 targets)
      for (int n2 = 0; n2 < p.N; ++n2) {
        float Lc[NC];                  // what a voxel of class c adds (WT: mask_class_labeled)
#pragma unroll
        for (int c = 0; c < NC; ++c) Lc[c] = 1.f;
        if constexpr (WT) {
          if (wt.lab) {
#pragma unroll
            for (int c = 0; c < NC; ++c) Lc[c] = e2_uniform_ld(wt.lab, n2 * NC + c);
          }
        }
        const float* tp = p.tg + (long)n2 * p.tsN;
        const int head = min(p.S, (int)((4 - (((uintptr_t)tp >> 2) & 3)) & 3));   // floats up to 16-B alignment
        const int nv = (p.S - head) >> 2;
        const f32x4* tv4 = reinterpret_cast<const f32x4*>(tp + head);
        for (int i0 = 0; i0 < nv; i0 += 256 * 8) {
          f32x4 v[8];
  #pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int i = i0 + u * 256 + tid;
            v[u] = i < nv ? tv4[i] : f32x4{-1.f, -1.f, -1.f, -1.f};
          }
  #pragma unroll
          for (int u = 0; u < 8; ++u)
  #pragma unroll
            for (int e = 0; e < 4; ++e)
  #pragma unroll
              for (int c = 0; c < NC; ++c) cnt += (v[u][e] == (float)c) ? Lc[c] : 0.f;
        }
        // the unaligned head and the tail of < 4 floats
        const int rest = p.S - head - 4 * nv;
        if (tid < head + rest) {
          const float tv = tid < head ? tp[tid] : tp[head + 4 * nv + (tid - head)];
  #pragma unroll
          for (int c = 0; c < NC; ++c) cnt += (tv == (float)c) ? Lc[c] : 0.f;
        }
      }
  #pragma unroll
      for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
      if (lane == 0) RED[wave] = cnt;
      if constexpr (WT) {
        if (tid == 0) RED[4] = head_w_count_dn(wt, p.N * NC, p.S);
      }
    }
    TAIL_STAMP(1);
    if (tid < kRows) {                          // head weights and the layer's bias, once
#pragma unroll
      for (int c = 0; c < NC; ++c) WH[c * kRows + tid] = tid < p.C2 ? p.wh[c * p.C2 + tid] : 0.f;
      WH[NC * kRows + tid] = tid < p.C2 ? p.b1[tid] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < NR; ++j) T[(pq + j * NQ) * NPP + pp] = xv[j];
  }

  // ---- one GEMM phase: acc[i] (+)= sum_k img[k][m] * T[k][position] --------------------------
  f32x4 acc[MTW];
  auto lds_a = [](const float* q) { return (unsigned)(uintptr_t)(lds_vp)q; };
  // step s of a chunk: A[i] = chunk[4 s + kq][16 (wm MTW + i) + l15], B = tile[k0 + 4 s + kq][position]
  auto rd = [&](unsigned wb, unsigned tb, int s, float (&A)[MTW], float& B) {
    if (TAIL_DBG(4)) return;
#pragma unroll
    for (int i = 0; i < MTW; ++i)
      asm volatile("ds_read_b32 %0, %1" : "=v"(A[i]) : "v"(wb + (unsigned)(s * 4 * BMS * 4 + i * 64)));
    asm volatile("ds_read_b32 %0, %1" : "=v"(B) : "v"(tb + (unsigned)(s * 4 * NPP * 4)));
  };
  auto fma = [&](float (&A)[MTW], float& B) {
#pragma unroll
    for (int i = 0; i < MTW; ++i) asm volatile("" : "+v"(A[i]));
    asm volatile("" : "+v"(B));
    if (TAIL_DBG(2)) return;
    if constexpr (BF) {
      const float Bb = tail_rnd_bf16(B);
#pragma unroll
      for (int i = 0; i < MTW; ++i)
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(tail_rnd_bf16(A[i]), Bb, acc[i], 0, 0, 0);
    } else {
#pragma unroll
    for (int i = 0; i < MTW; ++i)
      acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[i], B, acc[i], 0, 0, 0);
    }
  };
  // chunk c of a phase sits in buffer (buf0 + c) & 1; its first chunk was staged by the caller
  auto gemm = [&](const float* img, int coP, int ciP, const int (&woff)[NI], int K, int buf0,
                  bool next_d) {
#pragma unroll
    for (int i = 0; i < MTW; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nch = (K + kKC - 1) / kKC;
    for (int c = 0; c < nch; ++c) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();                         // chunk c has landed; the other buffer is free
      if (!TAIL_DBG(1)) {
      if (c + 1 < nch) stage(img, coP, ciP, woff, c + 1, (buf0 + c + 1) & 1);
      else if (next_d) stage(p.wpd, p.coPd, p.ciPd, woffD, 0, (buf0 + c + 1) & 1);   // phase C's first chunk
      }
      const unsigned wb = lds_a(WB + ((buf0 + c) & 1) * G::WB_F + (wm * MTW) * 16 + kq * BMS + l15);
      const unsigned tb = lds_a(T + (c * kKC + kq) * NPP + wn * 16 + l15);
      // operands of step s + 1 are requested before the MFMAs of step s are issued (inline-asm
      // reads, counted lgkmcnt: hipcc's own schedule waited for every pair of reads -- two
      // MFMAs per LDS round trip)
      float A0[MTW], A1[MTW], B0, B1;
      rd(wb, tb, 0, A0, B0);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s = 0; s < kKC / 4; s += 2) {
        rd(wb, tb, s + 1, A1, B1);
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(MTW + 1 < 15 ? MTW + 1 : 15) : "memory");
        __builtin_amdgcn_sched_barrier(0);
        fma(A0, B0);
        __builtin_amdgcn_sched_barrier(0);
        if (s + 2 < kKC / 4) rd(wb, tb, s + 2, A0, B0);
        __builtin_amdgcn_sched_barrier(0);
        if (s + 2 < kKC / 4) asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(MTW + 1 < 15 ? MTW + 1 : 15) : "memory");
        else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        fma(A1, B1);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    return nch;
  };

  TAIL_STAMP(2);
  // ======== phase A: pre = Wf^T x ================================================================
  const int nchA = gemm(p.wpf, p.coPf, p.ciPf, woffF, p.C1, 0, p.dx != nullptr);
  TAIL_STAMP(3);
  __syncthreads();                             // every wave is done with the x tile
  // h = relu(pre + b1) over the tile; rows past C2 are the zero k-rows of phase C
#pragma unroll
  for (int i = 0; i < MTW; ++i) {
    const int r0 = (wm * MTW + i) * 16 + 4 * kq;
    if (r0 < kRows) {
      const f32x4 bv = *reinterpret_cast<const f32x4*>(WH + NC * kRows + r0);   // (0 past C2)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = r0 + r;
        const float t = acc[i][r] + bv[r];       // rows past C2: zero weights, zero bias -> +0.0
        T[row * NPP + wn * 16 + l15] = (t > 0.f) ? t : ((t == 0.f) ? 0.f : -0.f);
      }
    }
  }
  __syncthreads();

  TAIL_STAMP(4);
  // ======== head: logits, softmax, loss, dlogits ================================================
  {
    const int per = (p.C2 + NQ - 1) / NQ;
    const int c0 = pq * per, c1 = min(c0 + per, p.C2);
    float lg[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) lg[c] = 0.f;
#pragma unroll 10
    for (int co = c0; co < c1; ++co) {
      const float hv = fmaxf(T[co * NPP + pp], 0.f);
#pragma unroll
      for (int c = 0; c < NC; ++c) lg[c] = fmaf(WH[c * kRows + co], hv, lg[c]);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) PL[(pq * NC + c) * NP + pp] = lg[c];
  }
  __syncthreads();
  TAIL_STAMP(5);
  float inv;
  {
    float tot = p.count_here ? ((RED[0] + RED[1]) + (RED[2] + RED[3])) : p.stats[1];
    if constexpr (WT) {
      if (p.count_here) tot += RED[4];
    }
    inv = 1.f / (tot + E2_EPS_NLL);
    if (blockIdx.x == 0 && tid == 0 && p.count_here) p.stats[1] = tot;
  }
  if (wave == 0) {                             // (NP <= 64 positions: lanes 0 .. NP-1)
    float lsum = 0.f;
    float d[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) d[c] = 0.f;
    if (tid < np) {
      float lg[NC], m = -INFINITY;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        float s = 0.f;
        for (int q = 0; q < NQ; ++q) s += PL[(q * NC + c) * NP + tid];
        lg[c] = s + p.bh[c];
        m = fmaxf(m, lg[c]);
      }
      float den = 0.f;
#pragma unroll
      for (int c = 0; c < NC; ++c) den += expf(lg[c] - m);
      const float tv = p.tg[(long)n * p.tsN + s0 + tid];
      float* prp = p.pr + (long)n * p.psN + s0 + tid;
      if constexpr (!WT) {
      float pc[NC], pt = 0.f;
      int tc = -1;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        pc[c] = expf(lg[c] - m) / den;
        prp[(long)c * p.psC] = pc[c];
        if (tv == (float)c) { tc = c; pt = pc[c]; lsum -= logf(pc[c] + E2_EPS_NLL); }
      }
      // dL/dp_t = -inv / (p_t + eps);  dlogit_c = p_c (dp_c - sum_k dp_k p_k)   (head.hip)
      const float gpt = (tc >= 0) ? (-(p.sum_mode ? 1.f : inv) / (pt + E2_EPS_NLL)) * pt : 0.f;
#pragma unroll
      for (int c = 0; c < NC; ++c) d[c] = gpt * ((c == tc ? 1.f : 0.f) - pc[c]);
      } else {
        const float ev = evw;
        float ex[NC], pc[NC], unused = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          ex[c] = expf(lg[c] - m);
          pc[c] = ex[c] / den;
          prp[(long)c * p.psC] = pc[c];
        }
        lsum = head_w_loss<NC>(hw, ex, den, tv, ev, &unused);
        head_w_dlogits<NC>(hw, pc, tv, ev * (p.sum_mode ? 1.f : inv), d);
      }
    }
    if (tid < NP) {
#pragma unroll
      for (int c = 0; c < NC; ++c) DL[c * NP + tid] = d[c];
    }
    // this work-group's loss sum and head-bias gradient (lanes >= np hold zeros)
    float* mine = p.part + blockIdx.x;             // element e of this slot: mine[e * gridDim.x]
    const long nS = gridDim.x;
    float v = lsum;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) mine[(NC * p.C2 + NC + p.C2) * nS] = v;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      float sb = d[c];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) sb += __shfl_xor(sb, o, 64);
      if (lane == 0) mine[(NC * p.C2 + c) * nS] = sb;
    }
  }
  __syncthreads();

  TAIL_STAMP(6);
  // ======== dpre = (Wh^T dlogits) * relu'(h), thread = channel row ============================
  if (tid < p.C2) {
    const int row = tid;
    float w[NC], aw[NC], db = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) { w[c] = WH[c * kRows + row]; aw[c] = 0.f; }
    float* tr = T + row * NPP;
#pragma unroll 8
    for (int q = 0; q < NP; ++q) {
      const float hv = tr[q];
      float g = 0.f;
#pragma unroll
      for (int c = 0; c < NC; ++c) g = fmaf(w[c], DL[c * NP + q], g);     // (0 past the sample)
      const float slope = (hv > 0.f) ? 1.f : (__builtin_signbit(hv) ? 0.f : 0.5f);
      const float d = g * slope;
      tr[q] = d;
      db += d;
      const float hp = fmaxf(hv, 0.f);
#pragma unroll
      for (int c = 0; c < NC; ++c) aw[c] = fmaf(DL[c * NP + q], hp, aw[c]);
    }
    float* mine = p.part + blockIdx.x;
    const long nS = gridDim.x;
#pragma unroll
    for (int c = 0; c < NC; ++c) mine[(c * p.C2 + row) * nS] = aw[c];
    mine[(NC * p.C2 + NC + row) * nS] = db;
  }
  __syncthreads();
  TAIL_STAMP(7);
  // the dpre tile to memory (the 1x1x1 layer's weight gradient reads it), rows of NP positions
  if (pp < np) {
    float* db_ = p.dpre + (long)n * p.dsN + s0 + pp;
#pragma unroll 10
    for (int r = pq; r < p.C2; r += NQ) db_[(long)r * p.dsC] = T[r * NPP + pp];
  }
  if (!p.dx) return;                           // (uniform: nothing upstream needs a gradient)

  TAIL_STAMP(8);
  // ======== phase C: dx = Wd^T dpre =============================================================
  gemm(p.wpd, p.coPd, p.ciPd, woffD, p.C2, nchA & 1, false);
  TAIL_STAMP(9);
  __syncthreads();                             // every wave is done with the dpre tile
#pragma unroll
  for (int i = 0; i < MTW; ++i) {
    const int r0 = (wm * MTW + i) * 16 + 4 * kq;
    if (r0 < kRows) {
#pragma unroll
      for (int r = 0; r < 4; ++r) T[(r0 + r) * NPP + wn * 16 + l15] = acc[i][r];
    }
  }
  __syncthreads();
  {
    const int sp = s0 + min(pp, np - 1);
    const int z = sp / (p.H * p.W), rem = sp - z * (p.H * p.W);
    const int y = rem / p.W, xx = rem - y * p.W;
    float* gb = p.dx + (long)n * p.gsN + (long)z * p.gsD + (long)y * p.gsH + xx;
    if (p.gm == 0) {
      if (pp < np) {
#pragma unroll 10
        for (int r = pq; r < p.C1; r += NQ) gb[(long)r * p.gsC] = T[r * NPP + pp];
      }
    } else {
      // through the producing layer's activation backward; its bias gradient = the row sums,
      // reduced over the NP lanes of a row (each lane holds ONE position of the row)
      const float* sb = p.gm_src ? p.gm_src + (long)n * p.msN + s0 + min(pp, np - 1) : nullptr;
      float* red = WB;                           // [C1] row sums (the weight buffers are free)
      constexpr int NR = kRows / NQ;
      // every source value of the thread requested before the first use (one load per loop
      // trip made this pass 13-26 dependent round trips: +12 us on neuro3d_lite)
      float sl[NR];
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        const int r = pq + j * NQ;
        sl[j] = 1.f;
        if (sb && r < p.C1 && pp < np) sl[j] = sb[(long)r * p.msC];
      }
      if (p.gm == 2) {
#pragma unroll
        for (int j = 0; j < NR; ++j) {
          const int r = pq + j * NQ;
          const float o = sl[j] + p.gm_bias[min(r, p.C1 - 1)];
          sl[j] = (o > 0.f) ? 1.f : ((o == 0.f) ? 0.5f : 0.f);
        }
      } else if (p.gm == 1) {
#pragma unroll
        for (int j = 0; j < NR; ++j) sl[j] = (sl[j] > 0.f) ? 1.f : (__builtin_signbit(sl[j]) ? 0.f : 0.5f);
      }
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        const int r = pq + j * NQ;               // (uniform per NP lanes)
        float d = 0.f;
        if (r < p.C1 && pp < np) {
          d = T[r * NPP + pp] * sl[j];
          gb[(long)r * p.gsC] = d;
        }
#pragma unroll
        for (int o = NP / 2; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
        if (pp == 0 && r < p.C1) red[r] = d;
      }
      __syncthreads();
      if (tid < p.C1)
        p.part[((long)(NC * p.C2 + NC + p.C2 + 1) + tid) * gridDim.x + blockIdx.x] = red[tid];
    }
  }
  TAIL_STAMP(10);
