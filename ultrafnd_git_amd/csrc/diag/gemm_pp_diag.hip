// Diagnostics build of the persistent bf16 GEMM (libultrafnd_hip_diag.so): stamps and timing-only ablations.  Compiled like
// gemm_bf16_pp.hip, without packed fp32 instructions.
#define UFND_DIAG 1
#include "../gemm_bf16_pp.hpp"
#include "../gemm_bf16_checks.hpp"

// The persistent form (gemm_bf16_pp.hpp) with stamps: 8 uint64 per workgroup -- {s_memtime, s_memrealtime} at entry, ring
// prologue landed, last K loop done, END -- followed by one uint64 per workgroup: its tile count (stamps holds 9 * 256 words).
// dbg = 1: stamps; dbg = 3: stamps on the timing-only build without epilogue slices (results are garbage).
// The dbg = 1 build is for timing: tests/test_gpu_gemm_pp_cases.py holds the tile counts and the output of its PLAIN instantiation to
// the product kernel's, nothing checks the others, and tools/audit_pp_asm.py covers the product listing only -- the dbg = 1
// instantiations of the other three modes spill (scratch traffic inside the hand-counted vmcnt schedule).
extern "C" int ufnd_diag_gemm_pp_stamps(const void* A, const void* W, void* out_bf16, int M, int N, int K, unsigned long long* stamps,
                                        const ufnd_gemm_ln* ln, const float* bias, int act, int dbg, void* stream_) {
  UFND_REQUIRE(A && W && out_bf16 && stamps, "gemm_pp_stamps: null operand");
  GemmArgs a{(const __bf16*)A, (const __bf16*)W, bias, nullptr, (__bf16*)out_bf16, nullptr, M, N, K, K, K, N, N, N, act, 0, 0, stamps};
  if (ln) {
    a.a_stats = ln->a_stats; a.colsum = ln->colsum; a.r_stats = ln->r_stats; a.r_gamma = ln->r_gamma; a.r_beta = ln->r_beta;
    a.out_stats = ln->out_stats; a.a_parts = ln->a_parts; a.r_parts = ln->r_parts; a.a_eps = ln->a_eps; a.r_eps = ln->r_eps;
    a.inv_h = 1.0f / (float)ln->width;
    a.residual_b = (const __bf16*)ln->residual_bf16;
    a.ldrb = ln->ldrb;
    a.guard = ln->a_stats ? ln->guard : nullptr;
  }
  int rc = launch_pp(a, dbg, (hipStream_t)stream_);
  if (rc != UFND_OK) return rc;
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

// Validation, mode, walk geometry and automatic choice of one call of the persistent form, on the host only: nothing is launched
// and no operand is dereferenced -- the pointers only have to carry the alignment of the real ones -- so this answers on a machine
// without a GPU (tests/test_gemm_pp_cases.py).  The arguments are ufnd_gemm_bf16_ln's (ln = NULL: ufnd_gemm_bf16_ex's) with the tile
// as an argument of its own (ln->tile_cfg is not read) and the CU count the geometry and the choice are asked about (0: the
// device's).  The checks are the product entries' own: gemm_bf16_ln_check_args / gemm_bf16_check_args, then pp_check_args.
//   tile_cfg = UFND_GEMM_TILE_PERSISTENT   a forced call: whatever pp_check_args refuses is refused here, in its words
//   tile_cfg < 0                            the automatic choice: out[6] says whether pp_pick takes the call; a call it does not
//                                           take for failing pp_check_args answers UFND_OK with mode = -1 and zeros
//   out   {mode (0 plain, 1 fold, 2 residual through a LayerNorm, 3 residual), act, m_tiles, n_tiles, pp_rows, G (the grid),
//          picked by the automatic choice (0 / 1), out_stats partials per row (0 without out_stats)}
extern "C" int ufnd_diag_gemm_pp_plan(const void* A, const void* W, const float* bias, const float* residual, const void* out_bf16,
                                      const float* out_f32, int M, int N, int K, int lda, int ldw, int ldr, int ldo, int ldf, int act,
                                      const ufnd_gemm_ln* ln, int tile_cfg, int cus, int* out) {
  UFND_REQUIRE(out, "gemm_pp_plan: null result pointer");
  UFND_REQUIRE(tile_cfg == UFND_GEMM_TILE_PERSISTENT || tile_cfg < 0, "gemm_pp_plan: tile_cfg %d (UFND_GEMM_TILE_PERSISTENT or the automatic choice)", tile_cfg);
  UFND_REQUIRE(cus == 0 || (cus >= 8 && cus <= 4096), "gemm_pp_plan: %d compute units", cus);
  int rc = ln ? gemm_bf16_ln_check_args(A, W, bias, residual, out_bf16, out_f32, M, N, K, lda, ldw, ldr, ldo, ldf, act, ln)
              : gemm_bf16_check_args(A, W, bias, residual, out_bf16, out_f32, M, N, K, lda, ldw, ldr, ldo, ldf, act);
  if (rc != UFND_OK) return rc;
  GemmArgs a{(const __bf16*)A, (const __bf16*)W, bias, residual, (__bf16*)out_bf16, const_cast<float*>(out_f32), M, N, K, lda, ldw, ldr, ldo, ldf, act, 0, 0, nullptr};
  if (ln) {      // (as ufnd_gemm_bf16_ln_live)
    a.a_stats = ln->a_stats; a.colsum = ln->colsum; a.r_stats = ln->r_stats; a.r_gamma = ln->r_gamma; a.r_beta = ln->r_beta;
    a.out_stats = ln->out_stats; a.a_parts = ln->a_parts; a.r_parts = ln->r_parts; a.a_eps = ln->a_eps; a.r_eps = ln->r_eps;
    a.inv_h = 1.0f / (float)ln->width;
    a.residual_b = (const __bf16*)ln->residual_bf16;
    a.ldrb = ln->ldrb;
    a.guard = ln->a_stats ? ln->guard : nullptr;
  }
  for (int i = 0; i < 8; ++i) out[i] = 0;
  out[0] = -1;
  rc = pp_check_args(a, tile_cfg < 0);
  if (rc != UFND_OK) return tile_cfg < 0 ? UFND_OK : rc;
  const int G = pp_geometry(a, pp_cu_count(cus));
  out[0] = pp_mode_of(a);
  out[1] = a.act;
  out[2] = a.m_tiles;
  out[3] = a.n_tiles;
  out[4] = a.pp_rows;
  out[5] = G;
  out[6] = pp_pick(a, cus) ? 1 : 0;
  out[7] = a.out_stats ? pp_stat_parts(a.N) : 0;
  return UFND_OK;
}

// whether the persistent form's shape conditions hold (the host-only plan entry of gemm_diag.hip refuses to plan such a call)
int ufnd_diag_pp_shape_ok(int M, int N, int K) { return pp_shape_ok(M, N, K) ? 1 : 0; }
