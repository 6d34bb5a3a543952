// lr_attn_bwd_dkv_body.h -- the dK / dV pass of lr_attn_bwd_body.h (described there): the body of a __global__ kernel
//   (const u16* qkv, const u16* d_out, const float* lse, const float* dsum, u16* dqkv, const int32_t* cu, int nh, int nkv,
//    const float* rope_cs)
// that has named its geometry G, included between the kernel's braces. No include guard: one inclusion per kernel.
  static_assert(G::DKV_WAVES * 16 == G::KB, "a wave owns 16 of the workgroup's keys");
  static_assert(G::DKV_WAVES * G::DKV_PIECES * 1024 == G::TILE_BYTES, "the waves' pieces make up a tile");
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [2 stages][Q tile | dO tile], then the statistics
  float* stats = reinterpret_cast<float*>(smem + 2 * G::STAGE_BYTES);  // [2 stages][lse2[64] | D[64]]
  const int hd = G::HD;
  const int b = blockIdx.z, kvh = blockIdx.y, kb = blockIdx.x;
  const int tok0 = cu[b];
  const int T = cu[b + 1] - tok0;
  if (kb * G::KB >= T) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int quad = lane >> 4, li = lane & 15;
  const int rep = nh / nkv;
  const int stride = (nh + 2 * nkv) * hd;
  const int ostride = nh * hd;

  // ---- this lane's key: K and V fragments (B operands), d = 32 ks + 8 quad + 0..7
  const int kabs = kb * G::KB + wave * 16 + li;
  const int kr = min(kabs, T - 1);
  bf16x8 kf[G::KSTEPS], vf[G::KSTEPS];
  {
    const u16* kp = qkv + (size_t)(tok0 + kr) * stride + (nh + kvh) * hd + quad * 8;
    const u16* vp = kp + nkv * hd;
#pragma unroll
    for (int ks = 0; ks < G::KSTEPS; ++ks) {
      kf[ks] = *reinterpret_cast<const bf16x8*>(kp + ks * 32);
      vf[ks] = *reinterpret_cast<const bf16x8*>(vp + ks * 32);
    }
  }
  floatx4 dkt[G::DT], dvt[G::DT];
#pragma unroll
  for (int dt = 0; dt < G::DT; ++dt) dkt[dt] = dvt[dt] = floatx4{0.f, 0.f, 0.f, 0.f};
  const float sl2 = G::SCALE * AB_LOG2E;

  const int qb_first = kb, qb_last = (T - 1) / G::KB;
  const int nqb = qb_last - qb_first + 1;
  const int steps = nqb * rep;  // (query head of the group, query block) pairs, head-major
  // DMA staging as in the dQ pass: wave w moves pieces DKV_PIECES w .. of the Q tile (row stride of qkv) and of the dO tile
  // (row stride of d_out); rows past the prompt's end come back as zeros and are masked in P.
  unsigned qoff[G::DKV_PIECES], ooff[G::DKV_PIECES];
  G::piece_offsets2(wave, lane, stride, ostride, qoff, ooff);
  // a step's tiles are requested at the top of the step before (LDS-DMA) together with its 64 query rows' statistics
  // (ordinary loads into two registers of wave 0); the statistics are written to LDS at the END of that step, so that the
  // wait hipcc puts in front of the write coincides with the hand-written one for the DMA
  float st_l = 0.f, st_dd = 0.f;
  auto stage = [&](int step, int buf) {
    const int h = kvh * rep + step / nqb, qb = qb_first + step % nqb;
    char* base = smem + buf * G::STAGE_BYTES + wave * (G::DKV_PIECES * 1024);
    const int rows_left = T - 1 - qb * G::KB;
    const fa_int4 rq = fa_make_rsrc(
        reinterpret_cast<const char*>(qkv + (size_t)tok0 * stride + h * hd) + (size_t)qb * G::KB * stride * 2,
        (rows_left * stride + hd) * 2);
    const fa_int4 ro = fa_make_rsrc(
        reinterpret_cast<const char*>(d_out + (size_t)tok0 * ostride + h * hd) + (size_t)qb * G::KB * ostride * 2,
        (rows_left * ostride + hd) * 2);
#pragma unroll
    for (int i = 0; i < G::DKV_PIECES; ++i) {
      fa_dma16(rq, base + i * 1024, qoff[i]);
      fa_dma16(ro, base + G::TILE_BYTES + i * 1024, ooff[i]);
    }
    if (tid < 64) {
      const int q = min(qb * G::KB + tid, T - 1);
      st_l = lse[(size_t)(tok0 + q) * nh + h];   // (first use of either value: commit_stats)
      st_dd = dsum[(size_t)(tok0 + q) * nh + h];
    }
  };
  auto commit_stats = [&](int buf) {
    __builtin_amdgcn_sched_barrier(0);
    if (tid < 64) {
      stats[buf * 128 + tid] = st_l * AB_LOG2E;
      stats[buf * 128 + 64 + tid] = st_dd;
    }
  };
  lds_char* const lds = (lds_char*)smem;
  int row_off[G::NROW], tr_off[G::NTR];
  G::row_offsets(quad, li, row_off);
  G::tr_offsets(quad, li, tr_off);

  stage(0, 0);
#pragma unroll
  for (int ks = 0; ks < G::KSTEPS; ++ks) asm volatile("" ::"v"(kf[ks]), "v"(vf[ks]));
  commit_stats(0);
  AB_DMA_LANDED();
  __syncthreads();

  for (int step = 0; step < steps; ++step) {
    const int qb = qb_first + step % nqb;
    const int QS = (step & 1) * G::STAGE_BYTES, OS = QS + G::TILE_BYTES;
    const float* st_lse = stats + (step & 1) * 128;
    const float* st_d = st_lse + 64;
    if (step + 1 < steps) stage(step + 1, (step + 1) & 1);
    // ---- S = Q K^T and dP = dO V^T : rows = queries 16 mt + 4 quad + r, column = this lane's key
    floatx4 s[4], dp[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) s[mt] = dp[mt] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < G::KSTEPS; ++ks)
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const bf16x8 qa = *reinterpret_cast<lds_bf16x8*>(lds + G::row_addr(row_off, QS + mt * 16 * G::ROW_BYTES, ks));
        const bf16x8 oa = *reinterpret_cast<lds_bf16x8*>(lds + G::row_addr(row_off, OS + mt * 16 * G::ROW_BYTES, ks));
        s[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa, kf[ks], s[mt], 0, 0, 0);
        dp[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(oa, vf[ks], dp[mt], 0, 0, 0);
      }
    // ---- P and dS, packed as B operands (k index = query row)
    bf16x8 pb[2], dsb[2];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const floatx4 l4 = *reinterpret_cast<const floatx4*>(st_lse + mt * 16 + quad * 4);
      const floatx4 d4 = *reinterpret_cast<const floatx4*>(st_d + mt * 16 + quad * 4);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = qb * G::KB + mt * 16 + quad * 4 + r;
        float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[mt][r], sl2, -l4[r]));
        p = (kabs <= q && q < T) ? p : 0.f;
        pb[mt >> 1][(mt & 1) * 4 + r] = (__bf16)p;
        dsb[mt >> 1][(mt & 1) * 4 + r] = (__bf16)(p * (dp[mt][r] - d4[r]));
      }
    }
    // ---- dV^T += dO^T P,  dK^T += Q^T dS
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2)
#pragma unroll
      for (int dt = 0; dt < G::DT; ++dt) {
        const int off = G::tr_addr(tr_off, ks2 * 32 * G::ROW_BYTES, dt);
        const bf16x8 ot = fa_read_vt<G::ROW_BYTES>(lds + (OS + off));
        const bf16x8 qt = fa_read_vt<G::ROW_BYTES>(lds + (QS + off));
        dvt[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ot, pb[ks2], dvt[dt], 0, 0, 0);
        dkt[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qt, dsb[ks2], dkt[dt], 0, 0, 0);
      }
    if (step + 1 < steps) commit_stats((step + 1) & 1);
    AB_DMA_LANDED();   // this wave's pieces of step + 1
    __syncthreads();
  }
  if (kabs < T) {
    u16* kp = dqkv + (size_t)(tok0 + kabs) * stride + (nh + kvh) * hd + quad * 4;
    u16* vp = kp + nkv * hd;
#pragma unroll
    for (int dt = 0; dt < G::DT; ++dt) {
      u16x4 ok, ov;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = dkt[dt][r] * G::SCALE;
      attn_bwd_unrotate<G::HD>(v, rope_cs, kabs, dt, quad);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        ok[r] = f2bf(v[r]);
        ov[r] = f2bf(dvt[dt][r]);
      }
      *reinterpret_cast<u16x4*>(kp + dt * 16) = ok;
      *reinterpret_cast<u16x4*>(vp + dt * 16) = ov;
    }
  }
