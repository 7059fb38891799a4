// Host-side argument checks of the one-tile bf16 GEMM entries (ufnd_gemm_bf16[_ex|_live], ufnd_gemm_bf16_ln[_live],
// ufnd_gemm_bf16_dgrad), in one place: the product entries (gemm_bf16.hip, gemm_bf16_bwd.hip) and the host-only plan entry of the
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
