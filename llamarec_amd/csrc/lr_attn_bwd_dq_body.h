// lr_attn_bwd_dq_body.h -- the dQ pass of lr_attn_bwd_body.h (described there): the body of a __global__ kernel
//   (const u16* qkv, const u16* d_out, const float* lse, const float* dsum, u16* dqkv, const int32_t* cu, int nh, int nkv,
//    int max_qblocks, const float* rope_cs)
// that has named its geometry G, included between the kernel's braces. No include guard: one inclusion per kernel.
  constexpr int QT = G::DQ_QT;
  static_assert(G::DQ_WAVES * 16 * QT == G::QROWS && G::KSTEPS * 32 == G::HD && G::DT * 16 == G::HD, "geometry");
  static_assert(G::DQ_WAVES * G::DQ_PIECES * 1024 == G::TILE_BYTES, "the waves' pieces make up a tile");
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [2 stages][K tile | V tile]
  const int hd = G::HD;
  const int b = blockIdx.z, h = blockIdx.y;
  const int qb = max_qblocks - 1 - (int)blockIdx.x;   // heavy tiles first
  const int tok0 = cu[b];
  const int T = cu[b + 1] - tok0;
  if (qb * G::QROWS >= T) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int quad = lane >> 4, li = lane & 15;
  const int kvh = h / (nh / nkv);
  const int stride = (nh + 2 * nkv) * hd;
  const u16* kbase = qkv + (size_t)tok0 * stride + (nh + kvh) * hd;
  const u16* vbase = kbase + nkv * hd;

  // ---- Q and dO fragments (B operands): row q, d = 32 ks + 8 quad + 0..7; lse and D of the lane's rows
  const int wave_q0 = qb * G::QROWS + wave * (16 * QT);
  bf16x8 qf[QT][G::KSTEPS], dof[QT][G::KSTEPS];
  int qabs[QT];
  float lse2[QT], dq_row[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    qabs[qt] = wave_q0 + qt * 16 + li;
    const int qr = min(qabs[qt], T - 1);
    const u16* qp = qkv + (size_t)(tok0 + qr) * stride + h * hd + quad * 8;
    const u16* dp = d_out + (size_t)(tok0 + qr) * nh * hd + h * hd + quad * 8;
#pragma unroll
    for (int ks = 0; ks < G::KSTEPS; ++ks) {
      qf[qt][ks] = *reinterpret_cast<const bf16x8*>(qp + ks * 32);
      dof[qt][ks] = *reinterpret_cast<const bf16x8*>(dp + ks * 32);
    }
    lse2[qt] = lse[(size_t)(tok0 + qr) * nh + h] * AB_LOG2E;
    dq_row[qt] = dsum[(size_t)(tok0 + qr) * nh + h];
  }
  floatx4 dqt[QT][G::DT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt)
#pragma unroll
    for (int dt = 0; dt < G::DT; ++dt) dqt[qt][dt] = floatx4{0.f, 0.f, 0.f, 0.f};

  const int q_last = min(qb * G::QROWS + G::QROWS - 1, T - 1);
  const int kb_last = q_last / G::KB;
  const int wave_q_last = wave_q0 + 16 * QT - 1;
  const bool wave_live = wave_q0 < T;
  const float sl2 = G::SCALE * AB_LOG2E;

  // ---- DMA staging: a tile is TILE_BYTES / 1024 pieces of 1 KiB (64 lanes x 16 B, lane-linear in LDS); wave w moves pieces
  // DQ_PIECES w .. of K and of V (V's rows stand nkv hd elements behind K's, which the descriptors' bases carry). The swizzle
  // is applied to the SOURCE chunk. Rows past the prompt's end are range-checked to zero by the per-block buffer descriptor
  // (those keys are masked for every query row of the prompt).
  unsigned soff[G::DQ_PIECES];
  G::template piece_offsets<G::DQ_PIECES>(wave, lane, stride, soff);
  auto stage = [&](int kb, int buf) {
    char* base = smem + buf * G::STAGE_BYTES + wave * (G::DQ_PIECES * 1024);
    const size_t blk_off = (size_t)kb * G::KB * stride * 2;
    const int records = ((T - 1 - kb * G::KB) * stride + hd) * 2;   // bytes from the block's first K (V) element
    const fa_int4 rk = fa_make_rsrc(reinterpret_cast<const char*>(kbase) + blk_off, records);
    const fa_int4 rv = fa_make_rsrc(reinterpret_cast<const char*>(vbase) + blk_off, records);
#pragma unroll
    for (int i = 0; i < G::DQ_PIECES; ++i) {
      fa_dma16(rk, base + i * 1024, soff[i]);
      fa_dma16(rv, base + G::TILE_BYTES + i * 1024, soff[i]);
    }
  };
  // LDS read addresses, the lane's part computed once
  lds_char* const lds = (lds_char*)smem;
  int row_off[G::NROW], tr_off[G::NTR];
  G::row_offsets(quad, li, row_off);
  G::tr_offsets(quad, li, tr_off);

  stage(0, 0);
  // Q, dO and the statistics must be resident before the loop: otherwise their loads are waited for behind the in-loop DMA
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
#pragma unroll
    for (int ks = 0; ks < G::KSTEPS; ++ks) asm volatile("" ::"v"(qf[qt][ks]), "v"(dof[qt][ks]));
    asm volatile("" ::"v"(lse2[qt]), "v"(dq_row[qt]));
  }
  AB_DMA_LANDED();
  __syncthreads();

  for (int kb = 0; kb <= kb_last; ++kb) {
    const int KS = (kb & 1) * G::STAGE_BYTES, VS = KS + G::TILE_BYTES;
    if (kb < kb_last) stage(kb + 1, (kb + 1) & 1);
    if (wave_live && kb * G::KB <= wave_q_last) {   // otherwise every key of the block is masked for this wave
      // ---- S^T = K Q^T (rows = keys 16 nt + 4 quad + r, column = query li), then P^T in place
      floatx4 st[QT][4];
#pragma unroll
      for (int qt = 0; qt < QT; ++qt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) st[qt][nt] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < G::KSTEPS; ++ks)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const bf16x8 kf = *reinterpret_cast<lds_bf16x8*>(lds + (KS + nt * 16 * G::ROW_BYTES + G::row_addr(row_off, ks)));
#pragma unroll
          for (int qt = 0; qt < QT; ++qt)
            st[qt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[qt][ks], st[qt][nt], 0, 0, 0);
        }
#pragma unroll
      for (int qt = 0; qt < QT; ++qt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int key = kb * G::KB + nt * 16 + quad * 4 + r;
            const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(st[qt][nt][r], sl2, -lse2[qt]));
            st[qt][nt][r] = (key <= qabs[qt] && qabs[qt] < T) ? p : 0.f;
          }
      // ---- dP^T = V dO^T and dS^T = P^T .* (dP^T - D), packed as the B operand of dQ^T += K^T dS^T
      // (k index 8 quad + j <-> key 32 ks2 + 16 (j >> 2) + 4 quad + (j & 3), as the S^T layout gives it)
      bf16x8 dsb[QT][2];
      if constexpr (G::DPT_WHOLE) {
        floatx4 dpt[QT][4];
#pragma unroll
        for (int qt = 0; qt < QT; ++qt)
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) dpt[qt][nt] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < G::KSTEPS; ++ks)
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) {
            const bf16x8 vf = *reinterpret_cast<lds_bf16x8*>(lds + (VS + nt * 16 * G::ROW_BYTES + G::row_addr(row_off, ks)));
#pragma unroll
            for (int qt = 0; qt < QT; ++qt)
              dpt[qt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, dof[qt][ks], dpt[qt][nt], 0, 0, 0);
          }
#pragma unroll
        for (int qt = 0; qt < QT; ++qt)
#pragma unroll
          for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              dsb[qt][nt >> 1][(nt & 1) * 4 + r] = (__bf16)(st[qt][nt][r] * (dpt[qt][nt][r] - dq_row[qt]));
      } else {   // one 16-key tile at a time, dS^T from it at once
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          floatx4 dpt[QT];
#pragma unroll
          for (int qt = 0; qt < QT; ++qt) dpt[qt] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < G::KSTEPS; ++ks) {
            const bf16x8 vf = *reinterpret_cast<lds_bf16x8*>(lds + (VS + nt * 16 * G::ROW_BYTES + G::row_addr(row_off, ks)));
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) dpt[qt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, dof[qt][ks], dpt[qt], 0, 0, 0);
          }
#pragma unroll
          for (int qt = 0; qt < QT; ++qt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              dsb[qt][nt >> 1][(nt & 1) * 4 + r] = (__bf16)(st[qt][nt][r] * (dpt[qt][r] - dq_row[qt]));
        }
      }
#pragma unroll
      for (int ks2 = 0; ks2 < 2; ++ks2)
#pragma unroll
        for (int dt = 0; dt < G::DT; ++dt) {
          const bf16x8 kt = fa_read_vt<G::ROW_BYTES>(lds + (KS + ks2 * 32 * G::ROW_BYTES + G::tr_addr(tr_off, dt)));
#pragma unroll
          for (int qt = 0; qt < QT; ++qt)
            dqt[qt][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kt, dsb[qt][ks2], dqt[qt][dt], 0, 0, 0);
        }
    }
    AB_DMA_LANDED();   // this wave's pieces of block kb + 1
    __syncthreads();
  }
  // ---- store scale * dQ: lane owns query row li, d = 16 dt + 4 quad + r
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    if (qabs[qt] < T) {
      u16* op = dqkv + (size_t)(tok0 + qabs[qt]) * stride + h * hd + quad * 4;
#pragma unroll
      for (int dt = 0; dt < G::DT; ++dt) {
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = dqt[qt][dt][r] * G::SCALE;
        attn_bwd_unrotate<G::HD>(v, rope_cs, qabs[qt], dt, quad);
        u16x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = f2bf(v[r]);
        *reinterpret_cast<u16x4*>(op + dt * 16) = o;
      }
    }
  }
