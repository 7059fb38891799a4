// fp32 skinny GEMMs on v_mfma_f32_32x32x2_f32 (see gemm_f32.hpp).
//
// MFMA 32x32x2 f32 operand maps (guide section 3): lane l, i = j = l & 31, h = l >> 5
//   A[i][k=h], B[k=h][j];  C/D: column j = l & 31, row = (r & 3) + 8 * (r >> 2) + 4 * h, r in [0,16).
// The contraction index may be permuted freely as long as A and B agree, so each lane loads
// FOUR consecutive contraction elements (16 B) and feeds element e to MFMA step e: half h of
// the wave covers k = kb + 4h + e of every 8-wide chunk.  The free index of the streamed
// weight matrix is likewise permuted so that a lane owns VEC consecutive output columns.
#include "gemm_f32.hpp"

namespace {

// ------------------------------------------------------------------------------------------
// The pieces the kernels share
// ------------------------------------------------------------------------------------------
// A launch: up to UFND_GEMM_MAX_PROB problems, laid out one after the other over the grid.
template <class Prob>
struct GemmArgs {
  Prob p[UFND_GEMM_MAX_PROB];
  int begin[UFND_GEMM_MAX_PROB + 1];  // first tile of every problem, begin[nprob] = all (NT, NN: a tile is a workgroup; TN: a wave-tile)
  int vec[UFND_GEMM_MAX_PROB];        // TN: per-problem vector width (tn_kernel<-1>)
  int nprob;
  const ufnd_step_state* st;          // NT, NN: the step state of the dropout streams
  __device__ __forceinline__ int find(int tile) const {      // the problem `tile` belongs to
    int pi = 0;
    for (int q = 1; q < nprob; ++q)
      if (tile >= begin[q]) pi = q;
    return pi;
  }
};
using NtArgs = GemmArgs<NtProb>;
using NnArgs = GemmArgs<NnProb>;
using TnArgs = GemmArgs<TnProb>;

// four consecutive floats as one 16-B (WVEC = 4) or two 8-B (WVEC = 2) loads
template <int WVEC>
__device__ __forceinline__ void load4(const float* p, float (&o)[4]) {
#pragma unroll
  for (int i = 0; i < 4; i += WVEC) {
    float t[WVEC];
    ld_vec<WVEC>(p + i, t);
#pragma unroll
    for (int q = 0; q < WVEC; ++q) o[i + q] = t[q];
  }
}

__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.0f;
  return z;
}

// The cross-wave reduction of the 32x32 forms whose four waves split the contraction: every wave parks its NA accumulators in
// LDS, barrier, and register r of accumulator a is then 0 + w0 + w1 + w2 + w3 (this order: the 16x16 forms add
// ((w0 + w1) + w2) + w3, which differs in the sign of a zero).  Wave w finalises registers 4w..4w+3.
template <int NA>
__device__ __forceinline__ void park_waves(float (&red)[4][NA][16][64], const f32x16 (&acc)[NA], int w, int lane) {
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) red[w][a][r][lane] = acc[a][r];
  __syncthreads();
}
template <int NA>
__device__ __forceinline__ float sum_waves(const float (&red)[4][NA][16][64], int a, int r, int lane) {
  float s = 0.0f;
#pragma unroll
  for (int ww = 0; ww < 4; ++ww) s += red[ww][a][r][lane];
  return s;
}

// NT finish: v = the sums of outputs n .. n + 3 of batch row m -> + bias, Z copy, GELU, dropout, store
__device__ __forceinline__ void nt_finish(const NtProb& P, const ufnd_step_state* st, int m, int n, f32x4 v) {
  if (P.bias) v += *reinterpret_cast<const f32x4*>(P.bias + n);
  if (P.Z) *reinterpret_cast<f32x4*>(P.Z + (size_t)m * P.ldz + n) = v;
  if (P.act == 1) {
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = gelu_f(v[q]);
  }
  if (P.drop_p > 0.0f) {
    float dm[4];      // (n is a multiple of 4 and N of 32: four aligned elements, one Philox evaluation)
    dropout_mul4(st, P.drop_p, P.drop_layer, (uint32_t)(m * P.N + n), dm);
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] *= dm[q];
  }
  *reinterpret_cast<f32x4*>(P.Y + (size_t)m * P.ldy + n) = v;
}

// NN finish: val = the sums of columns kcol .. kcol + VEC - 1 of row mrow -> activation backward, + add, store
template <int VEC>
__device__ __forceinline__ void nn_finish(const NnProb& P, const ufnd_step_state* st, int mrow, int kcol, float (&val)[VEC]) {
  if (P.actZ) {
    const float* z = P.actZ + (size_t)mrow * P.ldz + kcol;
    float dm[VEC];
    bool drawn = false;
    if constexpr (VEC == 4) {      // four aligned elements (kcol is a multiple of 4 in this form, drop_ld where it is): one Philox evaluation
      drawn = (P.drop_ld & 3) == 0;
      if (drawn) dropout_mul4(st, P.drop_p, P.drop_layer, (uint32_t)(mrow * P.drop_ld + kcol), dm);
    }
    if (!drawn) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) dm[v] = dropout_mul(st, P.drop_p, P.drop_layer, (uint32_t)(mrow * P.drop_ld + kcol + v));
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) val[v] = val[v] * gelu_grad_f(z[v]) * dm[v];      // (d g) m: the order of act_bwd_kernel and of autograd (the head's fused backward swaps one for the other)
  }
  if (P.add) {
    const float* ad = P.add + (size_t)mrow * P.ldadd + kcol;
#pragma unroll
    for (int v = 0; v < VEC; ++v) val[v] += ad[v];
  }
  float* dst = P.out + (size_t)mrow * P.ldo + kcol;
#pragma unroll
  for (int v = 0; v < VEC; ++v) dst[v] = val[v];
}

// ------------------------------------------------------------------------------------------
// NT: Y = act(X W^T + b).   block = 4 waves splitting the block's K range; LDS tree-free sum.
// ------------------------------------------------------------------------------------------
// U 8-wide chunks from kk on: every load is issued before the first MFMA
template <int MT, int WVEC, int U>
__device__ __forceinline__ void nt_k_step(const float* wrow, const float* const (&xrow)[MT], const bool (&xok)[MT], int kk, f32x16 (&acc)[MT]) {
  float a[U][4], b[U][MT][4];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    load4<WVEC>(wrow + kk + 8 * u, a[u]);
#pragma unroll
    for (int t = 0; t < MT; ++t) ld_vec_or_zero<4>(xrow[t] + kk + 8 * u, xok[t], b[u][t]);
  }
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int t = 0; t < MT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][e], b[u][t][e], acc[t], 0, 0, 0);
}

template <int MT, int WVEC>
__global__ __launch_bounds__(256) void nt_kernel(const NtArgs args) {
  __shared__ float red[4][MT][16][64];
  const int pi = args.find(blockIdx.x);
  const NtProb& P = args.p[pi];
  int local = blockIdx.x - args.begin[pi];
  const int ks = local % P.ksplit;
  local /= P.ksplit;
  const int n_tiles = P.N >> 5;
  const int n0 = (local % n_tiles) << 5;
  const int m0 = (local / n_tiles) * (32 * MT);

  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
  // K range of this block, then of this wave (multiples of 8 except at the very end of K)
  int kblk = (P.K + P.ksplit - 1) / P.ksplit;
  kblk = (kblk + 31) & ~31;
  const int kb0 = ks * kblk;
  const int kb1 = min(P.K, kb0 + kblk);
  const int sub = kblk >> 2;
  const int k0 = kb0 + w * sub;
  const int k1 = min(kb1, k0 + sub);

  f32x16 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = zero16();

  const float* wrow = P.W + (size_t)(n0 + j) * P.ldw;
  const float* xrow[MT];
  bool xok[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = m0 + 32 * t + j;
    xok[t] = m < P.M;
    xrow[t] = P.X + (size_t)(xok[t] ? m : 0) * P.ldx;
  }

  // Batches of U 8-wide chunks: every load of a batch is issued before its first MFMA, so a wave
  // keeps U x (1 + MT) 16-B loads in flight (the loop is latency-bound, not bandwidth-bound).
  constexpr int U = 4;      // (8 chunks per batch measured in round 4: no change, 0.2337 vs 0.2334 ms per head step)
  int k = k0;
  for (; k + 8 * U <= k1; k += 8 * U) nt_k_step<MT, WVEC, U>(wrow, xrow, xok, k + 4 * h, acc);
  for (; k + 8 <= k1; k += 8) nt_k_step<MT, WVEC, 1>(wrow, xrow, xok, k + 4 * h, acc);
  if (k < k1) {  // ragged tail (K not a multiple of 8), element-guarded
    const int kk = k + 4 * h;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool ok = (kk + e) < k1;
      const float a = ok ? wrow[kk + e] : 0.0f;
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const float b = (ok && xok[t]) ? xrow[t][kk + e] : 0.0f;
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[t], 0, 0, 0);
      }
    }
  }

  park_waves(red, acc, w, lane);
  // wave w finalises accumulator registers 4w..4w+3: rows n = n0 + 8w + 4h + q, column m
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    f32x4 v;
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = sum_waves(red, t, 4 * w + q, lane);
    const int m = m0 + 32 * t + j;
    const int n = n0 + 8 * w + 4 * h;
    if (m >= P.M) continue;
    if (P.ksplit > 1) *reinterpret_cast<f32x4*>(P.Y + ((size_t)ks * P.M + m) * P.N + n) = v;      // bare partials
    else nt_finish(P, args.st, m, n, v);
  }
}

// ------------------------------------------------------------------------------------------
// NT on 16x16 tiles (v_mfma_f32_16x16x4_f32), for launches that are too small to fill the chip with 32x32 tiles (round 3).
// The fp32 MFMA rate is per SIMD, so a 32-row batch against N = 512 outputs -- 16 tiles of 32x32 -- runs its whole contraction
// on 16 CUs: 128 dependent MFMAs per wave at K = 1,024.  With 16x16 tiles the same launch has 64 workgroups and a quarter of
// the chain per wave.  Operand maps: A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15]; C/D: column j = l & 15, row 4 (l >> 4) + r.
// A lane loads four consecutive contraction elements (16 B) and feeds element e to MFMA step e (a chunk = 16 contraction
// elements = 4 MFMAs); rows n of W are the A operand, batch rows m the B operand, so a lane ends with four consecutive n of one m.
// The four waves split the K range; their partial tiles are added in wave order in LDS and wave 0 runs the epilogue.
// ------------------------------------------------------------------------------------------
// U 16-wide chunks from kk on: every load is issued before the first MFMA
template <int WVEC, int U>
__device__ __forceinline__ void nt16_k_step(const float* wrow, const float* xrow, bool xok, int kk, f32x4& acc) {
  float a[U][4], b[U][4];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    load4<WVEC>(wrow + kk + 16 * u, a[u]);
    ld_vec_or_zero<4>(xrow + kk + 16 * u, xok, b[u]);
  }
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][e], b[u][e], acc, 0, 0, 0);
}

template <int WVEC>
__global__ __launch_bounds__(256) void nt16_kernel(const NtArgs args) {
  __shared__ float red[4][4][64];
  const int pi = args.find(blockIdx.x);
  const NtProb& P = args.p[pi];
  const int local = blockIdx.x - args.begin[pi];
  const int n_tiles = P.N >> 4;
  const int n0 = (local % n_tiles) << 4;
  const int m0 = (local / n_tiles) << 4;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
  // K range of this wave (multiples of 16 except at the very end of K); ksplit == 1 in this form
  int sub = (P.K + 3) / 4;
  sub = (sub + 15) & ~15;
  const int k0 = min(P.K, w * sub), k1 = min(P.K, k0 + sub);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const float* wrow = P.W + (size_t)(n0 + j) * P.ldw;
  const int m = m0 + j;
  const bool xok = m < P.M;
  const float* xrow = P.X + (size_t)(xok ? m : 0) * P.ldx;
  constexpr int U = 8;      // 8 chunks = 128 contraction elements per batch: 16 loads of 16 B in flight, then 32 MFMAs
  int k = k0;
  for (; k + 16 * U <= k1; k += 16 * U) nt16_k_step<WVEC, U>(wrow, xrow, xok, k + 4 * g, acc);
  for (; k + 16 <= k1; k += 16) nt16_k_step<WVEC, 1>(wrow, xrow, xok, k + 4 * g, acc);
  if (k < k1) {  // ragged tail (K not a multiple of 16), element-guarded
    const int kk = k + 4 * g;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool ok = (kk + e) < k1;
      const float a = ok ? wrow[kk + e] : 0.0f;
      const float b = (ok && xok) ? xrow[kk + e] : 0.0f;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) red[w][r][lane] = acc[r];
  __syncthreads();
  if (w != 0 || !xok) return;
  f32x4 v;
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = ((red[0][r][lane] + red[1][r][lane]) + red[2][r][lane]) + red[3][r][lane];
  nt_finish(P, args.st, m, n0 + 4 * g, v);      // this lane: outputs n .. n + 3 of batch row m
}

// ------------------------------------------------------------------------------------------
// NN: dX = dY W  (contraction over the weight's ROW index n; weight rows stream coalesced).
// A wave owns a strip of 32*VEC output columns (lane j owns columns kc + VEC*j .. +VEC-1).
// ------------------------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(256) void nn_kernel(const NnArgs args) {
  __shared__ float red[4][VEC][16][64];
  const int pi = args.find(blockIdx.x);
  const NnProb& P = args.p[pi];
  int local = blockIdx.x - args.begin[pi];
  const int ns = local % P.nsplit;
  local /= P.nsplit;
  const int strips = (P.K + 32 * VEC - 1) / (32 * VEC);
  const int kc = (local % strips) * 32 * VEC;
  const int m0 = (local / strips) * 32;

  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
  int nblk = (P.N + P.nsplit - 1) / P.nsplit;
  nblk = (nblk + 31) & ~31;
  const int nb0 = ns * nblk;
  const int nb1 = min(P.N, nb0 + nblk);
  const int sub = nblk >> 2;
  const int n0 = nb0 + w * sub;
  const int n1 = min(nb1, n0 + sub);  // N % 32 == 0 (host-checked) => multiples of 8

  f32x16 acc[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc[v] = zero16();

  const int m = m0 + j;
  const bool mok = m < P.M;
  const float* dyrow = P.dY + (size_t)(mok ? m : 0) * P.lddy;
  const int kcol = kc + VEC * j;
  const bool kok = kcol < P.K;  // K % VEC == 0 (host-checked)
  const float* wcol = P.W + (kok ? kcol : 0);

  // batches of U chunks (8 weight rows each): all 5U loads of a batch in flight before its MFMAs
  constexpr int U = (VEC == 4) ? 4 : (VEC == 2 ? 6 : 8);
  for (int n = n0; n < n1; n += 8 * U) {
    float a[U][4], b[U][4][VEC];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int nn = n + 8 * u + 4 * h;
      const bool nok = (n + 8 * u) < n1;
      ld_vec_or_zero<4>(dyrow + nn, mok && nok, a[u]);
#pragma unroll
      for (int e = 0; e < 4; ++e) ld_vec_or_zero<VEC>(wcol + (size_t)(nn + e) * P.ldw, kok && nok, b[u][e]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][e], b[u][e][v], acc[v], 0, 0, 0);
  }

  park_waves(red, acc, w, lane);
  // wave w finalises registers 4w..4w+3: rows mrow = m0 + q + 8w + 4h, columns kc + VEC*j + v
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float val[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) val[v] = sum_waves(red, v, 4 * w + q, lane);
    const int mrow = m0 + q + 8 * w + 4 * h;
    if (mrow >= P.M || !kok) continue;
    if (P.nsplit > 1) {
      float* dst = P.out + ((size_t)ns * P.M + mrow) * P.ldo + kcol;      // partials [nsplit][M][ldo] (the one caller has ldo == K or the consumer's row stride)
#pragma unroll
      for (int v = 0; v < VEC; ++v) dst[v] = val[v];
      continue;
    }
    nn_finish<VEC>(P, args.st, mrow, kcol, val);
  }
}

// ------------------------------------------------------------------------------------------
// NN on 16x16 tiles (v_mfma_f32_16x16x4_f32) for narrow layers (see nt16_kernel): tile = 16 batch rows x 16 output columns.
// A = dY rows (lane (i, g) loads dY[m0 + i][n + 4 g .. + 3] as 16 B), B = W[n + 4 g + e][kcol0 + j] (four 4-B loads, 16 lanes
// contiguous); C/D: column kcol0 + (l & 15), rows m0 + 4 (l >> 4) + r.  The four waves split the contraction range, partial
// tiles are added in wave order in LDS, wave 0 runs the epilogue.  nsplit == 1 only.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nn16_kernel(const NnArgs args) {
  __shared__ float red[4][4][64];
  const int pi = args.find(blockIdx.x);
  const NnProb& P = args.p[pi];
  const int local = blockIdx.x - args.begin[pi];
  const int strips = (P.K + 15) >> 4;
  const int kc = (local % strips) << 4;
  const int m0 = (local / strips) << 4;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
  int sub = (P.N + 3) / 4;
  sub = (sub + 15) & ~15;
  const int n0 = min(P.N, w * sub), n1 = min(P.N, n0 + sub);      // N % 32 == 0 (host-checked) => multiples of 16
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const int m = m0 + j;
  const bool mok = m < P.M;
  const float* dyrow = P.dY + (size_t)(mok ? m : 0) * P.lddy;
  const int kcol = kc + j;
  const bool kok = kcol < P.K;
  const float* wcol = P.W + (kok ? kcol : 0);
  constexpr int U = 4;      // 4 chunks = 64 contraction rows per batch: 4 + 16 loads in flight, then 16 MFMAs
  for (int n = n0; n < n1; n += 16 * U) {
    float a[U][4], b[U][4];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int nn = n + 16 * u + 4 * g;
      const bool nok = (n + 16 * u) < n1;
      ld_vec_or_zero<4>(dyrow + nn, mok && nok, a[u]);
#pragma unroll
      for (int e = 0; e < 4; ++e) b[u][e] = (kok && nok) ? wcol[(size_t)(nn + e) * P.ldw] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][e], b[u][e], acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) red[w][r][lane] = acc[r];
  __syncthreads();
  if (w != 0 || !kok) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int mrow = m0 + 4 * g + r;
    if (mrow >= P.M) continue;
    float val[1] = {((red[0][r][lane] + red[1][r][lane]) + red[2][r][lane]) + red[3][r][lane]};
    nn_finish<1>(P, args.st, mrow, kcol, val);
  }
}

// ------------------------------------------------------------------------------------------
// TN: dW = dY^T X (contraction over the batch rows), db = column sums of dY.
// One wave per (32 weight rows) x (32*VEC weight columns) tile; no LDS, no barrier.
// ------------------------------------------------------------------------------------------
// MSPLIT = 0: one wave per tile (4 tiles per workgroup), the whole batch in one wave's chain -- small batches.
// MSPLIT = 1 (M >= 128): one WORKGROUP per tile, wave w takes the w-th quarter of the batch rows (rounded to 8), the four
// partial tiles meet in LDS and are added in wave order; wave w stores accumulator registers 4w..4w+3.  At B = 256 the
// one-wave form is a chain of 8 load-then-MFMA passes with about one wave per SIMD to hide them behind (139 us for the
// grouped launch, 72 us for the classifier's 272 tiles); this form has 4 x the waves and a quarter of the chain.
// SEG = 1: the batch rows come in segments (TnProb::seg_rows; the factor form of the data-parallel exchange) -- its own
// instantiation, so that the one-panel kernels keep their code.
template <int VEC, int MSPLIT, int SEG>
__device__ __forceinline__ void tn_tile(const TnProb& P, int local, int w, int lane) {
  const int j = lane & 31, h = lane >> 5;
  const int strips = (P.K + 32 * VEC - 1) / (32 * VEC);
  const int strip = local % strips;
  const int n0 = (local / strips) << 5;
  const int kcol = strip * 32 * VEC + VEC * j;
  const bool kok = kcol < P.K;

  f32x16 acc[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc[v] = zero16();
  float dbsum = 0.0f;
  const float* dycol = P.dY + n0 + j;
  const float* xcol = P.X + (kok ? kcol : 0);

  int m_lo = 0, m_hi = P.M;
  if constexpr (MSPLIT) {
    const int per = ((P.M + 3) / 4 + 7) & ~7;
    m_lo = w * per;
    m_hi = m_lo + per < P.M ? m_lo + per : P.M;
  }
  constexpr int U = 4;   // 32 batch rows per pass: every load of the pass is issued before its MFMAs
  for (int mb = m_lo; mb < m_hi; mb += 8 * U) {
    float a[U][4];
    float b[U][4][VEC];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int m = mb + 8 * u + 4 * h + e;
        const bool ok = m < m_hi;
        size_t oy = (size_t)m * P.lddy, ox = (size_t)m * P.ldx;
        if constexpr (SEG) {
          const int sg = m / P.seg_rows, r = m - sg * P.seg_rows;
          oy = (size_t)sg * P.seg_dy + (size_t)r * P.lddy;
          ox = (size_t)sg * P.seg_x + (size_t)r * P.ldx;
        }
        a[u][e] = ok ? dycol[oy] : 0.0f;
        ld_vec_or_zero<VEC>(xcol + ox, ok && kok, b[u][e]);
      }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        dbsum += a[u][e];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][e], b[u][e][v], acc[v], 0, 0, 0);
      }
  }

  if constexpr (MSPLIT) {
    __shared__ float red[4][VEC][16][64];
    __shared__ float dbr[4][64];
    dbr[w][lane] = dbsum;
    park_waves(red, acc, w, lane);
    // wave w finalises accumulator registers 4w..4w+3: weight rows n0 + q + 8w + 4h
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float val[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) val[v] = sum_waves(red, v, 4 * w + q, lane);
      if (kok) st_vec<VEC>(P.dW + (size_t)(n0 + q + 8 * w + 4 * h) * P.ldw + kcol, val);
    }
    if (strip == 0 && P.db && w == 0) {
      float t = 0.0f;
#pragma unroll
      for (int ww = 0; ww < 4; ++ww) t += dbr[ww][lane];
      t += __shfl_xor(t, 32, 64);
      if (h == 0) P.db[n0 + j] = t;
    }
  } else {
    if (kok) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float val[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) val[v] = acc[v][r];
        st_vec<VEC>(P.dW + (size_t)(n0 + (r & 3) + 8 * (r >> 2) + 4 * h) * P.ldw + kcol, val);
      }
    }
    if (strip == 0 && P.db) {
      const float s = dbsum + __shfl_xor(dbsum, 32, 64);
      if (h == 0) P.db[n0 + j] = s;
    }
  }
}
// VEC < 0: every problem with its OWN vector width (TnArgs::vec: 4 where its operands allow 16-byte accesses, else 2) -- a
// (hidden + aux)-wide problem then no longer puts a whole grouped launch on 8-byte accesses (one-wave-per-tile form only).
template <int VEC, int MSPLIT = 0, int SEG = 0>
__global__ __launch_bounds__(256) void tn_kernel(const TnArgs args) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tile = MSPLIT ? (int)blockIdx.x : blockIdx.x * 4 + w;
  if (tile >= args.begin[args.nprob]) return;
  const int pi = args.find(tile);
  const TnProb& P = args.p[pi];
  const int local = tile - args.begin[pi];
  if constexpr (VEC > 0) {
    tn_tile<VEC, MSPLIT, SEG>(P, local, w, lane);
  } else {
    static_assert(VEC > 0 || MSPLIT == 0, "per-problem widths: one wave per tile");
    if (args.vec[pi] == 4) tn_tile<4, 0, SEG>(P, local, w, lane);      // (wave-uniform)
    else tn_tile<2, 0, SEG>(P, local, w, lane);
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------
// host launchers (argument checks guard every assumption the kernels make).  Each launcher is two steps: choose() validates the
// problems, fills the kernel arguments and names the instantiation and its grid without touching the device; run() launches it.
// ------------------------------------------------------------------------------------------
namespace {

// begin[] from a per-problem tile count; returns the launch's tiles
template <class Prob, class Tiles>
int lay_out(GemmArgs<Prob>& a, Tiles tiles) {
  int total = 0;
  for (int i = 0; i < a.nprob; ++i) {
    a.begin[i] = total;
    total += tiles(a.p[i], i);
  }
  a.begin[a.nprob] = total;
  return total;
}

// Can the streamed operands of a problem be read (TN: and written) `v` floats at a time?  v = 2 is what every kernel needs
// (refused otherwise), v = 4 picks the 16-byte forms.
bool wide(const NtProb& p, int v) { return p.ldw % v == 0 && ufnd_aligned(p.W, 4 * v); }
bool wide(const NnProb& p, int v) { return p.K % v == 0 && p.ldw % v == 0 && ufnd_aligned(p.W, 4 * v); }
bool wide(const TnProb& p, int v) { return p.K % v == 0 && p.ldx % v == 0 && p.ldw % v == 0 && ufnd_aligned(p.X, 4 * v) && ufnd_aligned(p.dW, 4 * v); }
bool wide_seg(const TnProb& p, int v) { return p.seg_rows == 0 || p.seg_x % v == 0; }

int choose(const NtProb* probs, int nprob, NtArgs& a, GemmF32Form* form, int* grid) {
  UFND_REQUIRE(nprob >= 1 && nprob <= UFND_GEMM_MAX_PROB, "nt: %d problems", nprob);
  UFND_REQUIRE(probs, "nt: null problem array");
  a.nprob = nprob;
  int maxM = 0, t32 = 0;
  bool vec4 = true, plain = true;
  for (int i = 0; i < nprob; ++i) {
    const NtProb& p = probs[i];
    UFND_REQUIRE(p.X && p.W && p.Y && p.M > 0 && p.K > 0, "nt[%d]: null/empty operand", i);
    UFND_REQUIRE(p.N % 32 == 0, "nt[%d]: N=%d not a multiple of 32", i, p.N);
    UFND_REQUIRE(p.ldx % 4 == 0 && ufnd_aligned(p.X, 16), "nt[%d]: X must be 16-B aligned with ldx%%4==0", i);
    UFND_REQUIRE(wide(p, 2), "nt[%d]: W must be 8-B aligned with even ldw", i);
    UFND_REQUIRE(p.ksplit >= 1 && p.ksplit <= 64, "nt[%d]: ksplit=%d", i, p.ksplit);
    UFND_REQUIRE(ufnd_aligned(p.Y, 16) && (p.ksplit > 1 || p.ldy % 4 == 0), "nt[%d]: Y alignment", i);
    UFND_REQUIRE(!p.Z || (ufnd_aligned(p.Z, 16) && p.ldz % 4 == 0), "nt[%d]: Z alignment", i);
    UFND_REQUIRE(!p.bias || ufnd_aligned(p.bias, 16), "nt[%d]: bias alignment", i);
    UFND_REQUIRE((long long)p.M * p.N < (1ll << 31), "nt[%d]: M*N too large", i);
    vec4 = vec4 && wide(p, 4);
    plain = plain && p.ksplit == 1;
    t32 += p.N / 32;
    maxM = p.M > maxM ? p.M : maxM;
    a.p[i] = p;
  }
  // narrow layers: 16x16 tiles (four times the workgroups, a quarter of the MFMA chain per wave).  The choice looks at the
  // layers' widths only, never at the batch: a row's arithmetic must not depend on the batch it is computed in
  if (plain && t32 <= 128) {
    *grid = lay_out(a, [](const NtProb& p, int) { return (p.N / 16) * ufnd_cdiv(p.M, 16); });
    *form = vec4 ? GEMM_F32_NT16_W4 : GEMM_F32_NT16_W2;
    return UFND_OK;
  }
  // two 32-row tiles per workgroup (the weight tile is read once for 64 rows) only when the launch still fills the chip that way:
  // the fp32 MFMA rate is per SIMD, so a launch of a few dozen workgroups is matrix-bound on the CUs it occupies
  auto blocks = [&](int mt) { return lay_out(a, [mt](const NtProb& p, int) { return (p.N / 32) * ufnd_cdiv(p.M, 32 * mt) * p.ksplit; }); };
  const int MT = (maxM > 32 && blocks(1) >= 512) ? 2 : 1;
  *grid = blocks(MT);
  *form = MT == 1 ? (vec4 ? GEMM_F32_NT_M1_W4 : GEMM_F32_NT_M1_W2) : (vec4 ? GEMM_F32_NT_M2_W4 : GEMM_F32_NT_M2_W2);
  return UFND_OK;
}

int choose(const NnProb* probs, int nprob, NnArgs& a, GemmF32Form* form, int* grid) {
  UFND_REQUIRE(nprob >= 1 && nprob <= UFND_GEMM_MAX_PROB, "nn: %d problems", nprob);
  UFND_REQUIRE(probs, "nn: null problem array");
  a.nprob = nprob;
  int s32 = 0;
  bool vec4 = true, plain = true;
  for (int i = 0; i < nprob; ++i) {
    const NnProb& p = probs[i];
    UFND_REQUIRE(p.dY && p.W && p.out && p.M > 0 && p.K > 0, "nn[%d]: null/empty operand", i);
    UFND_REQUIRE(p.N % 32 == 0, "nn[%d]: N=%d not a multiple of 32", i, p.N);
    UFND_REQUIRE(p.lddy % 4 == 0 && ufnd_aligned(p.dY, 16), "nn[%d]: dY alignment", i);
    UFND_REQUIRE(wide(p, 2), "nn[%d]: W alignment", i);
    UFND_REQUIRE(p.nsplit >= 1 && p.nsplit <= 64, "nn[%d]: nsplit=%d", i, p.nsplit);
    UFND_REQUIRE((long long)p.M * p.K < (1ll << 31), "nn[%d]: M*K too large", i);
    // the mask is the dropout that followed the activation in the forward: the kernels regenerate it inside the activation
    // backward, so a mask without actZ would be dropped without a word
    UFND_REQUIRE(!(p.drop_p > 0.0f) || p.actZ, "nn[%d]: drop_p=%g without actZ (the dropout mask belongs to the activation backward)", i,
                 (double)p.drop_p);
    // the mask's element index m * drop_ld + k is formed in 32 bits and must name one element per (m, k)
    UFND_REQUIRE(!(p.drop_p > 0.0f) || (p.drop_ld >= p.K && (long long)p.M * p.drop_ld < (1ll << 31)),
                 "nn[%d]: drop_ld=%d with K=%d, M=%d (drop_ld >= K and M*drop_ld < 2^31)", i, p.drop_ld, p.K, p.M);
    vec4 = vec4 && wide(p, 4);
    plain = plain && p.nsplit == 1;
    s32 += ufnd_cdiv(p.K, 32);
    a.p[i] = p;
  }
  // narrow layers: 16x16 tiles (chosen by the layers' widths only, never by the batch: see the NT choice)
  if (plain && s32 <= 128) {
    *grid = lay_out(a, [](const NnProb& p, int) { return ufnd_cdiv(p.K, 16) * ufnd_cdiv(p.M, 16); });
    *form = GEMM_F32_NN16;
    return UFND_OK;
  }
  int VEC = vec4 ? 4 : 2;
  auto blocks = [&](int vec) { return lay_out(a, [vec](const NnProb& p, int) { return ufnd_cdiv(p.K, 32 * vec) * ufnd_cdiv(p.M, 32) * p.nsplit; }); };
  // A wave's MFMA chain is (contraction / 32) * VEC long at 64 cycles each: when a launch has only a
  // handful of blocks, narrow the strips (more blocks, shorter chains) -- the work is latency-, not
  // bandwidth-bound at that size.
  // (the fp32 MFMA rate is per SIMD: with few workgroups the launch is matrix-bound on the CUs it occupies, so the strips narrow
  //  until the launch has about one workgroup per CU)
  if (blocks(VEC) < 64) VEC = 1;
  else if (blocks(VEC) < 256) VEC = (VEC == 4 && blocks(2) >= 256) ? 2 : 1;
  *grid = blocks(VEC);
  *form = VEC == 4 ? GEMM_F32_NN_V4 : (VEC == 2 ? GEMM_F32_NN_V2 : GEMM_F32_NN_V1);
  return UFND_OK;
}

int choose(const TnProb* probs, int nprob, TnArgs& a, GemmF32Form* form, int* grid) {
  UFND_REQUIRE(nprob >= 1 && nprob <= UFND_GEMM_MAX_PROB, "tn: %d problems", nprob);
  UFND_REQUIRE(probs, "tn: null problem array");
  a.nprob = nprob;
  bool vec4 = true;
  for (int i = 0; i < nprob; ++i) {
    const TnProb& p = probs[i];
    UFND_REQUIRE(p.dY && p.X && p.dW && p.M > 0 && p.K > 0, "tn[%d]: null/empty operand", i);
    UFND_REQUIRE(p.N % 32 == 0, "tn[%d]: N=%d not a multiple of 32", i, p.N);
    UFND_REQUIRE(wide(p, 2), "tn[%d]: X/dW alignment", i);
    UFND_REQUIRE(p.seg_rows >= 0 && (p.seg_rows == 0 || (p.M % p.seg_rows == 0 && p.seg_dy > 0 && p.seg_x > 0)), "tn[%d]: %d rows in segments of %d",
                 i, p.M, p.seg_rows);
    UFND_REQUIRE((p.seg_rows != 0) == (probs[0].seg_rows != 0), "tn[%d]: segmented and one-panel problems in one launch", i);
    UFND_REQUIRE(wide_seg(p, 2), "tn[%d]: segment stride alignment", i);
    a.vec[i] = wide(p, 4) && wide_seg(p, 4) ? 4 : 2;
    vec4 = vec4 && a.vec[i] == 4;
    a.p[i] = p;
  }
  const bool seg = probs[0].seg_rows != 0;
  // Measured for the 32-row grouped launch in round 4 and not kept: 32 x 64 tiles (VEC = 2, twice the waves, half the MFMA chain each):
  // head-only step 0.254-0.256 -> 0.264 ms; a form whose accumulator v owns 32 CONSECUTIVE columns (4-byte accesses) and stores each
  // accumulator as soon as it is complete, so that the store phase starts under the matrix phase: 182 VGPRs (two waves per SIMD instead
  // of three), 24.7 -> 31.0 us for the launch (profiles/r04_head_tn_small.txt).  The 32 x 128 form with 16-B accesses stays.
  int minM = a.p[0].M;
  for (int i = 1; i < nprob; ++i) minM = a.p[i].M < minM ? a.p[i].M : minM;
  // one wave per tile (small batches) and mixed alignments: each problem keeps its own width (the same tiles and bits it would
  // have in a launch of its own); every other launch runs all its problems at the narrowest one
  const bool mixed = minM < 128 && !vec4 && nprob > 1;
  if (!mixed && !vec4)
    for (int i = 0; i < nprob; ++i) a.vec[i] = 2;
  const int total = lay_out(a, [&a](const TnProb& p, int i) { return (p.N / 32) * ufnd_cdiv(p.K, 32 * a.vec[i]); });
  if (minM >= 128) {      // batch rows split over the four waves of a workgroup (one workgroup per tile)
    *form = seg ? (vec4 ? GEMM_F32_TN_V4_MSPLIT_SEG : GEMM_F32_TN_V2_MSPLIT_SEG) : (vec4 ? GEMM_F32_TN_V4_MSPLIT : GEMM_F32_TN_V2_MSPLIT);
    *grid = total;
  } else {                // one wave per tile; segmented rows (gathered factors) are the same forms, rows addressed by segment
    if (mixed) *form = seg ? GEMM_F32_TN_MIXED_SEG : GEMM_F32_TN_MIXED;
    else if (vec4) *form = seg ? GEMM_F32_TN_V4_SEG : GEMM_F32_TN_V4;
    else *form = seg ? GEMM_F32_TN_V2_SEG : GEMM_F32_TN_V2;
    *grid = ufnd_cdiv(total, 4);
  }
  return UFND_OK;
}

#define UFND_FORM(form, ...) \
  case form: hipLaunchKernelGGL((__VA_ARGS__), dim3(grid), dim3(256), 0, stream, a); return true
bool launch_form(GemmF32Form form, const NtArgs& a, int grid, hipStream_t stream) {
  switch (form) {
    UFND_FORM(GEMM_F32_NT16_W4, nt16_kernel<4>);
    UFND_FORM(GEMM_F32_NT16_W2, nt16_kernel<2>);
    UFND_FORM(GEMM_F32_NT_M1_W4, nt_kernel<1, 4>);
    UFND_FORM(GEMM_F32_NT_M1_W2, nt_kernel<1, 2>);
    UFND_FORM(GEMM_F32_NT_M2_W4, nt_kernel<2, 4>);
    UFND_FORM(GEMM_F32_NT_M2_W2, nt_kernel<2, 2>);
    default: return false;
  }
}
bool launch_form(GemmF32Form form, const NnArgs& a, int grid, hipStream_t stream) {
  switch (form) {
    UFND_FORM(GEMM_F32_NN16, nn16_kernel);
    UFND_FORM(GEMM_F32_NN_V4, nn_kernel<4>);
    UFND_FORM(GEMM_F32_NN_V2, nn_kernel<2>);
    UFND_FORM(GEMM_F32_NN_V1, nn_kernel<1>);
    default: return false;
  }
}
bool launch_form(GemmF32Form form, const TnArgs& a, int grid, hipStream_t stream) {
  switch (form) {
    UFND_FORM(GEMM_F32_TN_V4, tn_kernel<4>);
    UFND_FORM(GEMM_F32_TN_V2, tn_kernel<2>);
    UFND_FORM(GEMM_F32_TN_MIXED, tn_kernel<-1>);
    UFND_FORM(GEMM_F32_TN_V4_MSPLIT, tn_kernel<4, 1>);
    UFND_FORM(GEMM_F32_TN_V2_MSPLIT, tn_kernel<2, 1>);
    UFND_FORM(GEMM_F32_TN_V4_SEG, tn_kernel<4, 0, 1>);
    UFND_FORM(GEMM_F32_TN_V2_SEG, tn_kernel<2, 0, 1>);
    UFND_FORM(GEMM_F32_TN_MIXED_SEG, tn_kernel<-1, 0, 1>);
    UFND_FORM(GEMM_F32_TN_V4_MSPLIT_SEG, tn_kernel<4, 1, 1>);
    UFND_FORM(GEMM_F32_TN_V2_MSPLIT_SEG, tn_kernel<2, 1, 1>);
    default: return false;
  }
}
#undef UFND_FORM

// choose, report, launch (st: the dropout streams' state of NT and NN; TN has none)
template <class Prob>
int run(const Prob* probs, int nprob, const ufnd_step_state* st, hipStream_t stream, GemmF32Form* form_out, int* grid_out) {
  GemmArgs<Prob> a;
  GemmF32Form form;
  int grid;
  const int rc = choose(probs, nprob, a, &form, &grid);
  if (rc != UFND_OK) return rc;
  a.st = st;
  if (form_out) *form_out = form;
  if (grid_out) *grid_out = grid;
  UFND_REQUIRE(launch_form(form, a, grid, stream), "gemm_f32: form %d", (int)form);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

}  // namespace

int launch_nt(const NtProb* probs, int nprob, const ufnd_step_state* st, hipStream_t stream) { return run(probs, nprob, st, stream, nullptr, nullptr); }
int launch_nn(const NnProb* probs, int nprob, const ufnd_step_state* st, hipStream_t stream) { return run(probs, nprob, st, stream, nullptr, nullptr); }
int launch_tn(const TnProb* probs, int nprob, hipStream_t stream) { return run(probs, nprob, nullptr, stream, nullptr, nullptr); }
