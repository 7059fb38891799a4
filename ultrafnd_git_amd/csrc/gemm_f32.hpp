// fp32 skinny-GEMM family for the Tier-A head (batch rows M = 4..256, weights streamed once).
// All three use v_mfma_f32_32x32x2_f32: exact fp32 (bit-identical to an fmaf chain), 157 TF peak,
// so at M = 32 the kernels are HBM-bound on the weight stream, not MFMA-bound.
#pragma once
#include "common.hpp"

#define UFND_GEMM_MAX_PROB 16

// The 20 kernel instantiations the three launchers choose between (gemm_f32.hip: choose_nt / choose_nn / choose_tn validate a
// launch and name its form on the host; the diagnostics library reports the choice to the op-level tests).
enum GemmF32Form {
  GEMM_F32_NT16_W4 = 0,         // nt16_kernel<4>: 16x16 tiles, 16-B weight loads
  GEMM_F32_NT16_W2,             // nt16_kernel<2>: 8-B weight loads
  GEMM_F32_NT_M1_W4,            // nt_kernel<1, 4>: one 32-row tile per workgroup
  GEMM_F32_NT_M1_W2,            // nt_kernel<1, 2>
  GEMM_F32_NT_M2_W4,            // nt_kernel<2, 4>: two 32-row tiles per workgroup
  GEMM_F32_NT_M2_W2,            // nt_kernel<2, 2>
  GEMM_F32_NN16,                // nn16_kernel
  GEMM_F32_NN_V4,               // nn_kernel<4>
  GEMM_F32_NN_V2,               // nn_kernel<2>
  GEMM_F32_NN_V1,               // nn_kernel<1>
  GEMM_F32_TN_V4,               // tn_kernel<4, 0, 0>: one wave per tile
  GEMM_F32_TN_V2,               // tn_kernel<2, 0, 0>
  GEMM_F32_TN_MIXED,            // tn_kernel<-1, 0, 0>: every problem with its own width
  GEMM_F32_TN_V4_MSPLIT,        // tn_kernel<4, 1, 0>: batch rows split over the four waves
  GEMM_F32_TN_V2_MSPLIT,        // tn_kernel<2, 1, 0>
  GEMM_F32_TN_V4_SEG,           // tn_kernel<4, 0, 1>: batch rows in segments
  GEMM_F32_TN_V2_SEG,           // tn_kernel<2, 0, 1>
  GEMM_F32_TN_MIXED_SEG,        // tn_kernel<-1, 0, 1>
  GEMM_F32_TN_V4_MSPLIT_SEG,    // tn_kernel<4, 1, 1>
  GEMM_F32_TN_V2_MSPLIT_SEG,    // tn_kernel<2, 1, 1>
  GEMM_F32_FORMS
};

// Y[m][n] = act(sum_k X[m][k] W[n][k] + bias[n])            (nn.Linear forward)
struct NtProb {
  const float* X;     // (M, K) row stride ldx (ldx % 4 == 0, 16-B aligned)
  const float* W;     // (N, K) row stride ldw
  const float* bias;  // (N) or null
  float* Y;           // (M, N) row stride ldy; when ksplit > 1: partials [ksplit][M][N]
  float* Z;           // optional pre-activation copy (M, N) row stride ldz
  int M, N, K, ldx, ldw, ldy, ldz;
  int act;            // 0 none, 1 exact GELU
  float drop_p;       // dropout on the output (train), 0 = off
  uint32_t drop_layer;
  int ksplit;         // grid-level split of K (1 => epilogue in-kernel)
};
int launch_nt(const NtProb* probs, int nprob, const ufnd_step_state* st, hipStream_t stream);

// dX[m][k] = (sum_n dY[m][n] W[n][k]) * [gelu'(actZ[m][k]) * dropmask] + add[m][k]
// The bracket is the activation backward and exists only with actZ: the mask is the dropout that followed the activation in the
// forward (element index m * drop_ld + k), so drop_p > 0 without actZ is refused.  With nsplit > 1 the kernels write bare partial
// sums and apply neither the bracket nor add.
struct NnProb {
  const float* dY;    // (M, N) row stride lddy (lddy % 4 == 0)
  const float* W;     // (N, K) row stride ldw
  float* out;         // (M, K) row stride ldo; when nsplit > 1: partials [nsplit][M] rows of stride ldo
  const float* actZ;  // optional (M, K) row stride ldz
  const float* add;   // optional (M, K) row stride ldadd
  int M, N, K, lddy, ldw, ldo, ldz, ldadd;
  float drop_p;       // needs actZ
  uint32_t drop_layer;
  int drop_ld;        // logical row stride used for the dropout element index (with drop_p > 0: >= K, M * drop_ld < 2^31)
  int nsplit;
};
int launch_nn(const NnProb* probs, int nprob, const ufnd_step_state* st, hipStream_t stream);

// dW[n][k] = sum_m dY[m][n] X[m][k];  db[n] = sum_m dY[m][n]
struct TnProb {
  const float* dY;    // (M, N) row stride lddy
  const float* X;     // (M, K) row stride ldx
  float* dW;          // (N, K) row stride ldw
  float* db;          // (N) or null
  int M, N, K, lddy, ldx, ldw;
  // Batch rows in SEGMENTS (gathered data-parallel factors: rank r's rows live at dY + r * seg_dy, X + r * seg_x, seg_rows rows
  // each, M = ranks x seg_rows); seg_rows == 0: one contiguous panel.
  int seg_rows, seg_dy, seg_x;
};
int launch_tn(const TnProb* probs, int nprob, hipStream_t stream);
