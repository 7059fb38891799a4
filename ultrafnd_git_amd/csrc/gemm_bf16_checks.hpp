// Host-side argument checks of the one-tile bf16 GEMM entries (ufnd_gemm_bf16[_ex|_live], ufnd_gemm_bf16_ln[_live],
// ufnd_gemm_bf16_dgrad) and the launch setup of the fused Q/K/V + attention entries (at the end), in one place: the product entries (gemm_bf16.hip, gemm_bf16_bwd.hip) and the host-only plan entry of the
// diagnostics library (diag/gemm_diag.hip: ufnd_diag_gemm_bf16_plan, which tests/test_gemm_bf16_cases.py reads the tile, the grid
// and every refusal from) call the same functions, so a check cannot exist in one and be missing in the other.  Nothing here
// dereferences an operand or touches the device.  Include after gemm_bf16_kernel.hpp.
#pragma once

// (`prod`, not `built`: the diagnostics library builds every tile of the table, the product library the PROD ones; in the product
//  library the two are equal)
static inline int gemm_bf16_check_args(const void* A, const void* W, const float* bias, const float* residual, const void* out_bf16,
                                       const float* out_f32, int M, int N, int K, int lda, int ldw, int ldr, int ldo, int ldf, int act) {
  UFND_REQUIRE(A && W && (out_bf16 || out_f32), "gemm_bf16: null operand");
  UFND_REQUIRE(M >= 1 && N >= 64 && K >= 64 && N % 64 == 0 && K % 64 == 0, "gemm_bf16: M=%d N=%d K=%d (need N%%64==0, K%%64==0)", M, N, K);
  UFND_REQUIRE(lda % 8 == 0 && ldw % 8 == 0 && lda >= K && ldw >= K && ufnd_aligned(A, 16) && ufnd_aligned(W, 16),
               "gemm_bf16: A/W strides must be multiples of 8 and pointers 16-B aligned");
  UFND_REQUIRE(!residual || (ldr % 4 == 0 && ldr >= N && ufnd_aligned(residual, 16)), "gemm_bf16: residual alignment");
  UFND_REQUIRE(!out_f32 || (ldf % 4 == 0 && ldf >= N && ufnd_aligned(out_f32, 16)), "gemm_bf16: out_f32 alignment");
  UFND_REQUIRE(!out_bf16 || (ldo % 8 == 0 && ldo >= N && ufnd_aligned(out_bf16, 16)), "gemm_bf16: out_bf16 alignment");
  UFND_REQUIRE(!bias || ufnd_aligned(bias, 4), "gemm_bf16: bias alignment");
  UFND_REQUIRE(act >= 0 && act <= 2, "gemm_bf16: act=%d", act);
  return UFND_OK;
}
static inline int gemm_bf16_check_tile(int cfg, int N) {
  UFND_REQUIRE(cfg >= 0 && cfg < kNumTiles && kTiles[cfg].prod, "gemm_bf16: tile config %d is not part of this library (ufnd_gemm_bf16_tile_info)", cfg);
  UFND_REQUIRE(N % kTiles[cfg].bn == 0, "gemm_bf16: tile config %d needs N %% %d == 0", cfg, kTiles[cfg].bn);
  return UFND_OK;
}

// {sum, sumsq} partials per row a LayerNorm-aware tile writes to out_stats (0: that tile has no statistics epilogue for this N)
static inline int stat_parts_for(int cfg, int N) {
  const TileCfg& t = kTiles[cfg];
  const int tn = t.bn / t.wn;
  if (!t.prod || !t.lnx || N % t.bn != 0 || tn % 32 != 0 || (N / 32) % 2 != 0 || N / 32 > 24) return 0;
  return N / 32;
}

static inline int gemm_bf16_ln_check_args(const void* A, const void* W, const float* bias, const float* residual, const void* out_bf16,
                                          const float* out_f32, int M, int N, int K, int lda, int ldw, int ldr, int ldo, int ldf, int act,
                                          const ufnd_gemm_ln* ln) {
  UFND_REQUIRE(A && W && ln && (out_bf16 || out_f32), "gemm_bf16_ln: null operand");
  UFND_REQUIRE(M >= 1 && N >= 64 && K >= 64 && N % 64 == 0 && K % 64 == 0, "gemm_bf16_ln: M=%d N=%d K=%d (need N%%64==0, K%%64==0)", M, N, K);
  UFND_REQUIRE(lda % 8 == 0 && ldw % 8 == 0 && lda >= K && ldw >= K && ufnd_aligned(A, 16) && ufnd_aligned(W, 16),
               "gemm_bf16_ln: A/W strides must be multiples of 8 and pointers 16-B aligned");
  UFND_REQUIRE(!residual || (ldr % 4 == 0 && ldr >= N && ufnd_aligned(residual, 16)), "gemm_bf16_ln: residual alignment");
  UFND_REQUIRE(!out_f32 || (ldf % 4 == 0 && ldf >= N && ufnd_aligned(out_f32, 16)), "gemm_bf16_ln: out_f32 alignment");
  UFND_REQUIRE(!out_bf16 || (ldo % 8 == 0 && ldo >= N && ufnd_aligned(out_bf16, 16)), "gemm_bf16_ln: out_bf16 alignment");
  UFND_REQUIRE(!bias || ufnd_aligned(bias, 16), "gemm_bf16_ln: bias must be 16-B aligned");
  UFND_REQUIRE(act >= 0 && act <= 2, "gemm_bf16_ln: act=%d", act);
  UFND_REQUIRE(!(ln->a_stats && ln->r_stats), "gemm_bf16_ln: a_stats and r_stats are mutually exclusive");
  UFND_REQUIRE(!(residual && ln->residual_bf16), "gemm_bf16_ln: residual (fp32) and residual_bf16 are mutually exclusive");
  UFND_REQUIRE(!ln->residual_bf16 || (ln->ldrb % 8 == 0 && ln->ldrb >= N && ufnd_aligned(ln->residual_bf16, 16)), "gemm_bf16_ln: residual_bf16 alignment");
  UFND_REQUIRE(ln->a_stats || act == UFND_ACT_NONE, "gemm_bf16_ln: an activation is only fused together with a folded LayerNorm (a_stats)");
  UFND_REQUIRE(ln->width > 0, "gemm_bf16_ln: width (the LayerNorm dimension) must be positive");
  if (ln->a_stats) {
    UFND_REQUIRE(!residual && !ln->residual_bf16 && !ln->out_stats,
                 "gemm_bf16_ln: a folded LayerNorm (a_stats) takes no residual and writes no out_stats (that epilogue is compiled without them)");
    UFND_REQUIRE(ln->colsum && ufnd_aligned(ln->colsum, 16) && ufnd_aligned(ln->a_stats, 16), "gemm_bf16_ln: colsum / a_stats alignment");
    UFND_REQUIRE(ln->a_parts >= 2 && ln->a_parts <= 24 && ln->a_parts % 2 == 0, "gemm_bf16_ln: a_parts=%d (even, 2..24)", ln->a_parts);
  }
  if (ln->r_stats) {
    UFND_REQUIRE((residual || ln->residual_bf16) && ln->r_gamma && ln->r_beta && ufnd_aligned(ln->r_gamma, 16) && ufnd_aligned(ln->r_beta, 16) &&
                     ufnd_aligned(ln->r_stats, 16), "gemm_bf16_ln: r_stats needs residual, r_gamma, r_beta (16-B aligned)");
    UFND_REQUIRE(ln->r_parts >= 2 && ln->r_parts <= 24 && ln->r_parts % 2 == 0, "gemm_bf16_ln: r_parts=%d (even, 2..24)", ln->r_parts);
  }
  return UFND_OK;
}
static inline int gemm_bf16_ln_check_tile(int cfg, int M, int N, int K, const ufnd_gemm_ln* ln) {
  UFND_REQUIRE(cfg >= 0 && cfg < kNumTiles && kTiles[cfg].prod && kTiles[cfg].lnx && N % kTiles[cfg].bn == 0,
               "gemm_bf16_ln: no LayerNorm-aware kernel for M=%d N=%d K=%d (tile %d)", M, N, K, cfg);
  if (ln->out_stats) {
    UFND_REQUIRE(stat_parts_for(cfg, N) > 0 && ufnd_aligned(ln->out_stats, 16), "gemm_bf16_ln: out_stats unsupported for this shape / tile");
  }
  return UFND_OK;
}

static inline int gemm_bf16_dgrad_check_args(const void* dY, const void* Wt, const float* residual, const void* aux, const void* out_bf16,
                                             const float* out_f32, int M, int N, int K, int lda, int ldw, int ldr, int ldaux, int ldo, int ldf,
                                             int act) {
  UFND_REQUIRE(dY && Wt && (out_bf16 || out_f32), "gemm_bf16_dgrad: null operand");
  UFND_REQUIRE(M >= 1 && N >= 64 && K >= 64 && N % 64 == 0 && K % 64 == 0, "gemm_bf16_dgrad: M=%d N=%d K=%d (need N%%64==0, K%%64==0)", M, N, K);
  UFND_REQUIRE(lda % 8 == 0 && ldw % 8 == 0 && lda >= K && ldw >= K && ufnd_aligned(dY, 16) && ufnd_aligned(Wt, 16),
               "gemm_bf16_dgrad: operand strides must be multiples of 8 and pointers 16-B aligned");
  UFND_REQUIRE(!residual || (ldr % 4 == 0 && ldr >= N && ufnd_aligned(residual, 16)), "gemm_bf16_dgrad: residual alignment");
  UFND_REQUIRE(!out_f32 || (ldf % 4 == 0 && ldf >= N && ufnd_aligned(out_f32, 16)), "gemm_bf16_dgrad: out_f32 alignment");
  UFND_REQUIRE(!out_bf16 || (ldo % 8 == 0 && ldo >= N && ufnd_aligned(out_bf16, 16)), "gemm_bf16_dgrad: out_bf16 alignment");
  UFND_REQUIRE(act == UFND_ACT_NONE || act == UFND_ACT_GELU_BWD || act == UFND_ACT_QUICK_GELU_BWD, "gemm_bf16_dgrad: act=%d", act);
  UFND_REQUIRE((act == UFND_ACT_NONE) == (aux == nullptr), "gemm_bf16_dgrad: aux (the pre-activations) goes with an activation backward, and only with one");
  UFND_REQUIRE(!aux || (!residual && ldaux % 8 == 0 && ldaux >= N && ufnd_aligned(aux, 16)), "gemm_bf16_dgrad: aux alignment (and no residual beside it)");
  return UFND_OK;
}
static inline int gemm_bf16_dgrad_check_tile(int cfg, int N) {
  UFND_REQUIRE(N % kTiles[cfg].bn == 0, "gemm_bf16_dgrad: tile %d needs N %% %d == 0", cfg, kTiles[cfg].bn);
  UFND_REQUIRE(gemm_bwd_tile(cfg), "gemm_bf16 backward: tile %d has no backward kernel", cfg);
  return UFND_OK;
}

// ---- The fused Q/K/V projection + attention launches (ATT kernels): checks, arguments and grid of the three geometries, for the product
// entries (gemm_bf16.hip) and the stamps entries of the diagnostics library (diag/gemm_diag.hip: the same setup, then a.stamps and
// the DBG instantiation).
// What the three share, after their own shape checks: the operand checks, the projection's arguments (M rows of X against the 3H
// stacked weight rows), the folded LayerNorm and the attention output.  `name` is the entry's name in its messages.
static inline int qkv_attention_args(const char* name, GemmArgs& a, const void* X, const void* Wqkv, const float* bqkv, void* ctx, int M, int heads,
                                     int ldx, int ldw, const ufnd_gemm_ln* ln) {
  const int H = heads * 64;
  UFND_REQUIRE(ldx % 8 == 0 && ldw % 8 == 0 && ldx >= H && ldw >= H && ufnd_aligned(X, 16) && ufnd_aligned(Wqkv, 16) && ufnd_aligned(ctx, 16),
               "%s: strides must be multiples of 8 and pointers 16-B aligned", name);
  UFND_REQUIRE(!bqkv || ufnd_aligned(bqkv, 16), "%s: bias alignment", name);
  a = GemmArgs{(const __bf16*)X, (const __bf16*)Wqkv, bqkv, nullptr, nullptr, nullptr, M, 3 * H, H, ldx, ldw, 0, 0, 0, UFND_ACT_NONE, 0, 0, nullptr};
  if (ln && ln->a_stats) {
    UFND_REQUIRE(ln->colsum && ufnd_aligned(ln->colsum, 16) && ufnd_aligned(ln->a_stats, 16), "%s: colsum / a_stats alignment", name);
    UFND_REQUIRE(ln->a_parts >= 2 && ln->a_parts <= 24 && ln->a_parts % 2 == 0 && ln->width > 0, "%s: a_parts=%d width=%d", name, ln->a_parts, ln->width);
    a.a_stats = ln->a_stats; a.colsum = ln->colsum; a.a_parts = ln->a_parts; a.a_eps = ln->a_eps;
    a.inv_h = 1.0f / (float)ln->width;
    a.guard = ln->guard;
  }
  a.att_ctx = (__bf16*)ctx;
  a.att_h = H;
  a.att_scale_log2e = 0.125f * 1.44269504088896340736f;      // 1 / sqrt(64) * log2(e)
  return UFND_OK;
}
// 128-token samples, one workgroup per (sample or slot bin, head pair): padded (cu_seqlens NULL), packed rows, slot bins
static inline int qkv_attention_pair_setup(GemmArgs& a, const void* X, const void* Wqkv, const float* bqkv, const int32_t* key_mask,
                                           const int32_t* cu_seqlens, const int32_t* bins, const int32_t* nbins, void* ctx, int B, int L, int heads,
                                           int ldx, int ldw, const ufnd_gemm_ln* ln) {
  UFND_REQUIRE(X && Wqkv && ctx, "qkv_attention: null operand");
  UFND_REQUIRE(!bins == !nbins && (!bins || cu_seqlens), "qkv_attention: slot bins need cu_seqlens, bins and nbins");
  UFND_REQUIRE(L == 128 && heads >= 2 && heads % 2 == 0 && heads <= 64 && B >= 1 && B <= 16384,
               "qkv_attention: B=%d L=%d heads=%d (this kernel is built for 128-token samples and an even head count; "
               "use ufnd_gemm_bf16[_ln] + ufnd_attention_bf16 otherwise)", B, L, heads);
  const int rc = qkv_attention_args("qkv_attention", a, X, Wqkv, bqkv, ctx, B * L, heads, ldx, ldw, ln);
  if (rc != UFND_OK) return rc;
  a.att_mask = key_mask;
  a.att_cu = cu_seqlens;
  a.att_bins = bins;
  a.att_nbins = nbins;
  a.m_live = cu_seqlens ? cu_seqlens + B : nullptr;      // (the live row count is cu_seqlens[B])
  a.m_tiles = B;
  a.n_tiles = heads / 2;
  a.xcd_cols = (a.n_tiles % 2 == 0 && a.m_tiles >= 4) ? 2 : 1;
  return UFND_OK;
}
// sample tiles (ufnd_text_pack_tiles): one workgroup per (256-row tile of whole samples, head)
static inline int qkv_attention_tiles_setup(GemmArgs& a, const void* X, const void* Wqkv, const float* bqkv, const int32_t* tiles,
                                            const int32_t* ntiles, void* ctx, int cap_tiles, int heads, int ldx, int ldw, const ufnd_gemm_ln* ln) {
  UFND_REQUIRE(X && Wqkv && ctx && tiles && ntiles, "qkv_attention_tiles: null operand");
  UFND_REQUIRE(heads >= 1 && heads <= 64 && cap_tiles >= 1 && cap_tiles <= (UFND_TEXT_TILE_MAX_B + 1) / 2, "qkv_attention_tiles: cap_tiles=%d heads=%d",
               cap_tiles, heads);
  const int rc = qkv_attention_args("qkv_attention_tiles", a, X, Wqkv, bqkv, ctx, cap_tiles * 256, heads, ldx, ldw, ln);
  if (rc != UFND_OK) return rc;
  a.att_bins = tiles;
  a.att_nbins = ntiles;
  a.m_tiles = cap_tiles;
  a.n_tiles = heads;
  a.xcd_cols = 1;                         // an XCD takes whole row tiles: the `heads` workgroups of a tile share its A rows in one L2
  return UFND_OK;
}
// samples of T <= 64 rows (a ViT layer: T = 50): one workgroup per (256 / T whole samples, head)
static inline int qkv_attention_vit_setup(GemmArgs& a, const void* X, const void* Wqkv, const float* bqkv, void* ctx, int N, int T, int heads, int ldx,
                                          int ldw, const ufnd_gemm_ln* ln) {
  UFND_REQUIRE(X && Wqkv && ctx, "qkv_attention_vit: null operand");
  UFND_REQUIRE(T >= 1 && T <= 64, "qkv_attention_vit: T=%d (this kernel is built for samples of 1 to 64 rows; use ufnd_gemm_bf16[_ln] + "
               "ufnd_attention_bf16 otherwise)", T);
  UFND_REQUIRE(heads >= 1 && heads <= 64 && N >= 1 && (long long)N * T <= (1 << 24), "qkv_attention_vit: N=%d T=%d heads=%d", N, T, heads);
  const int rc = qkv_attention_args("qkv_attention_vit", a, X, Wqkv, bqkv, ctx, N * T, heads, ldx, ldw, ln);
  if (rc != UFND_OK) return rc;
  a.att_t = T;
  a.m_tiles = ufnd_cdiv(N, 256 / T);      // 256 / T whole samples per row tile
  a.n_tiles = heads;
  a.xcd_cols = 1;                         // an XCD takes whole row tiles: the `heads` workgroups of a row tile share its A rows in one L2
  return UFND_OK;
}
// the launch of an ATT kernel after its setup (rings 3 / 2, eight waves; DBG = 1: the stamps build, a.stamps set)
template <int BM, int BN, int WM, int WN, int ATT, int DBG>
static inline void qkv_attention_launch(const GemmArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL((gemm_bf16_kernel<BM, BN, WM, WN, 3, 2, 16, 0, DBG, 1, ATT>), dim3(a.m_tiles * a.n_tiles), dim3(512), 0, stream, a);
}
