// fp32 skinny-GEMM family for the Tier-A head (batch rows M = 4..256, weights streamed once).
// All three use v_mfma_f32_32x32x2_f32: exact fp32 (bit-identical to an fmaf chain), 157 TF peak,
// so at M = 32 the kernels are HBM-bound on the weight stream, not MFMA-bound.
#pragma once
#include "common.hpp"

#define UFND_GEMM_MAX_PROB 16

// The 20 kernel instantiations the three launchers choose between (gemm_f32.hip: the three overloads of choose() validate a
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

// The three problem structures are filled through the builders below them (host only): every leading dimension sits next to
// its pointer and every optional feature is one named call.  The kernels and the ctypes mirrors read the plain members.

// Y[m][n] = act(sum_k X[m][k] W[n][k] + bias[n])            (nn.Linear forward)
struct NtProb {
  const float* X;
  const float* W;
  const float* bias;
  float* Y;
  float* Z;
  int M, N, K, ldx, ldw, ldy, ldz;
  int act;            // 0 none, 1 exact GELU
  float drop_p;
  uint32_t drop_layer;
  int ksplit;

  // Y = gelu(.), exact; Z: optional copy of the pre-activation (M, N), row stride ldz (16-B aligned, ldz % 4 == 0)
  NtProb& gelu(float* Z_, int ldz_) { Z = Z_; ldz = ldz_; act = 1; return *this; }
  // dropout on the output (train), p == 0 = off; the mask's element index is m * N + n in the stream `layer`
  NtProb& dropout(float p, uint32_t layer) { drop_p = p; drop_layer = layer; return *this; }
  // grid-level split of K: Y receives bare partials [n][M][N] and neither bias, Z, activation nor mask is applied
  NtProb& split_k(int n) { ksplit = n; return *this; }
};
// X: (M, K) row stride ldx (16-B aligned, ldx % 4 == 0); W: (N, K) row stride ldw; bias: (N) or null; Y: (M, N) row stride ldy
inline NtProb nt_linear(const float* X, int ldx, const float* W, int ldw, const float* bias, float* Y, int ldy, int M, int N, int K) {
  NtProb p{};
  p.X = X; p.ldx = ldx; p.W = W; p.ldw = ldw; p.bias = bias; p.Y = Y; p.ldy = ldy;
  p.M = M; p.N = N; p.K = K; p.ksplit = 1;
  return p;
}
int launch_nt(const NtProb* probs, int nprob, const ufnd_step_state* st, hipStream_t stream);

// dX[m][k] = (sum_n dY[m][n] W[n][k]) * [gelu'(actZ[m][k]) * dropmask] + add[m][k]
// The bracket is the activation backward and exists only with actZ: the mask is the dropout that followed the activation in the
// forward (element index m * drop_ld + k), so drop_p > 0 without actZ is refused.  With nsplit > 1 the kernels write bare partial
// sums and apply neither the bracket nor add.
struct NnProb {
  const float* dY;
  const float* W;
  float* out;
  const float* actZ;
  const float* add;
  int M, N, K, lddy, ldw, ldo, ldz, ldadd;
  float drop_p;
  uint32_t drop_layer;
  int drop_ld;
  int nsplit;

  // the activation backward: Z (M, K) row stride ldz, the forward's pre-activation; p, layer: the dropout that followed the
  // activation; drop_ld: the logical row stride of the mask's element index (with p > 0: >= K, M * drop_ld < 2^31)
  NnProb& act_bwd(const float* Z, int ldz_, float p, uint32_t layer, int drop_ld_) {
    actZ = Z; ldz = ldz_; drop_p = p; drop_layer = layer; drop_ld = drop_ld_;
    return *this;
  }
  // out += add: (M, K) row stride ldadd
  NnProb& plus(const float* add_, int ldadd_) { add = add_; ldadd = ldadd_; return *this; }
  // grid-level split of N: out receives partials [n][M] rows of stride ldo
  NnProb& split_n(int n) { nsplit = n; return *this; }
};
// dY: (M, N) row stride lddy (lddy % 4 == 0); W: (N, K) row stride ldw; out: (M, K) row stride ldo
inline NnProb nn_dgrad(const float* dY, int lddy, const float* W, int ldw, float* out, int ldo, int M, int N, int K) {
  NnProb p{};
  p.dY = dY; p.lddy = lddy; p.W = W; p.ldw = ldw; p.out = out; p.ldo = ldo;
  p.M = M; p.N = N; p.K = K; p.nsplit = 1;
  return p;
}
int launch_nn(const NnProb* probs, int nprob, const ufnd_step_state* st, hipStream_t stream);

// dW[n][k] = sum_m dY[m][n] X[m][k];  db[n] = sum_m dY[m][n]
struct TnProb {
  const float* dY;
  const float* X;
  float* dW;
  float* db;
  int M, N, K, lddy, ldx, ldw;
  int seg_rows, seg_dy, seg_x;

  // Batch rows in SEGMENTS (gathered data-parallel factors: rank r's rows live at dY + r * seg_dy, X + r * seg_x, `rows` rows
  // each, M = ranks x rows); rows == 0: one contiguous panel.
  TnProb& segments(int rows, int seg_dy_, int seg_x_) { seg_rows = rows; seg_dy = seg_dy_; seg_x = seg_x_; return *this; }
};
// dY: (M, N) row stride lddy; X: (M, K) row stride ldx; dW: (N, K) row stride ldw; db: (N) or null
inline TnProb tn_wgrad(const float* dY, int lddy, const float* X, int ldx, float* dW, int ldw, float* db, int M, int N, int K) {
  TnProb p{};
  p.dY = dY; p.lddy = lddy; p.X = X; p.ldx = ldx; p.dW = dW; p.ldw = ldw; p.db = db;
  p.M = M; p.N = N; p.K = K;
  return p;
}
int launch_tn(const TnProb* probs, int nprob, hipStream_t stream);

