// The reference's post graph (src/models/gnn/graph_builder.py), SURVEY.md section 2 row 13:
//   cosine_knn                  :4-28    S = Xn Xn^T + a Python argpartition loop  -> ufnd_cosine_knn (indices) + ufnd_dense_adj (KNN)
//   add_ocr_overlap_weights     :30-45   O(N^2) Python set intersections           -> ufnd_dense_adj (OCR)
//   add_temporal_inconsistency  :47-59   O(N^2) Python loop                        -> ufnd_dense_adj (TEMPORAL)
//   build_dense_adj             :61-68   the three in a row                        -> both entries, A written once
// S never exists in memory: a workgroup owns 32 query rows, streams 128-column tiles of S past them on the exact-fp32 MFMA
// (v_mfma_f32_32x32x2_f32, operands staged through LDS) and keeps each row's running top list in the registers of one wave
// (entry t in lane t, sorted by (S descending, j ascending)).  No atomics: the result is a pure function of the input.
#include "common.hpp"

namespace {

constexpr int KNN_QB = 32;        // query rows of a workgroup
constexpr int KNN_CB = 128;       // columns of S per pass: 32 per wave
constexpr int KNN_KC = 32;        // contraction chunk staged in LDS
constexpr int KNN_LD = KNN_KC + 4;   // LDS row stride (floats): 16-B aligned rows, rows 4 banks apart
constexpr int KNN_SLD = KNN_CB + 1;  // row stride of the score tile
constexpr int KNN_MAX_K = 64;     // one list entry per lane
constexpr int SET_LDS = 2048;     // as in gcn.hip: phrase ids of the block's own set kept in LDS

int knn_dp(int D) { return (D + KNN_KC - 1) / KNN_KC * KNN_KC; }

// xn (N, Dp) = rows of X divided by (||row||_2 + 1e-9), zero in the pad columns [D, Dp); one wave per row
__global__ __launch_bounds__(256) void knn_normalize_kernel(const float* __restrict__ X, int ldx, int N, int D, int Dp,
                                                            float* __restrict__ xn) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const float* x = X + (size_t)row * ldx;
  float ss = 0.0f;
  for (int c = lane; c < D; c += 64) ss += x[c] * x[c];
  ss = wave_sum(ss);
  const float den = sqrtf(ss) + 1e-9f;
  float* o = xn + (size_t)row * Dp;
  for (int c = lane; c < Dp; c += 64) o[c] = c < D ? x[c] / den : 0.0f;
}

// (s, j) ranks before (ts, tj): larger similarity first, ties to the lower index
__device__ __forceinline__ bool knn_before(float s, int j, float ts, int tj) { return s > ts || (s == ts && j < tj); }

__device__ __forceinline__ float lane_bcast(float v, int src) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), src));
}

// insert (s, j) into the wave's sorted list (entry t in lane t); the last entry falls off
__device__ __forceinline__ void knn_insert(float& ls, int& lj, float s, int j, int lane) {
  const int pos = __popcll(__ballot(knn_before(ls, lj, s, j)));       // the entries before the candidate are a prefix
  const float us = __shfl_up(ls, 1);
  const int uj = __shfl_up(lj, 1);
  if (lane == pos) {
    ls = s;
    lj = j;
  } else if (lane > pos) {
    ls = us;
    lj = uj;
  }
}

__global__ __launch_bounds__(256) void cosine_knn_kernel(const float* __restrict__ xn, int N, int Dp, int k, int32_t* __restrict__ idx) {
  __shared__ __attribute__((aligned(16))) float qs[KNN_QB][KNN_LD];
  __shared__ __attribute__((aligned(16))) float cs[KNN_CB][KNN_LD];
  __shared__ float sc[KNN_QB][KNN_SLD];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, j31 = lane & 31, h = lane >> 5;
  const int q0 = blockIdx.x * KNN_QB;

  float ls[8];      // wave w keeps the lists of query rows q0 + 8w .. q0 + 8w + 7
  int lj[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    ls[t] = -INFINITY;
    lj[t] = 0x7FFFFFFF;
  }

  const int srow = tid >> 3, scol = (tid & 7) * 4;      // staging: thread -> (row, 4 floats) of a 32 x 32 panel
  // The panels of contraction chunk kc of pass c0 travel global -> registers -> LDS; the loads of the NEXT chunk (of the next
  // pass after a pass's last chunk) are issued before this chunk's MFMAs, so their latency hides behind the MFMAs and, at a
  // pass boundary, behind the selection.
  f32x4 pq, pc[4];
  auto fetch = [&](int c0, int kc) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const int q = q0 + srow;
    pq = q < N ? *reinterpret_cast<const f32x4*>(xn + (size_t)q * Dp + kc + scol) : zero;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int c = c0 + 32 * p + srow;
      pc[p] = c < N ? *reinterpret_cast<const f32x4*>(xn + (size_t)c * Dp + kc + scol) : zero;
    }
  };
  fetch(0, 0);
  for (int c0 = 0; c0 < N; c0 += KNN_CB) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int kc = 0; kc < Dp; kc += KNN_KC) {
      *reinterpret_cast<f32x4*>(&qs[srow][scol]) = pq;
#pragma unroll
      for (int p = 0; p < 4; ++p) *reinterpret_cast<f32x4*>(&cs[32 * p + srow][scol]) = pc[p];
      __syncthreads();
      if (kc + KNN_KC < Dp) {
        fetch(c0, kc + KNN_KC);
      } else if (c0 + KNN_CB < N) {
        fetch(c0 + KNN_CB, 0);
      }
      // A = the wave's 32 candidate rows, B = the query rows; half h of the wave feeds k = 8u + 4h + e to step (u, e)
#pragma unroll
      for (int u = 0; u < KNN_KC / 8; ++u) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(&cs[32 * w + j31][8 * u + 4 * h]);
        const f32x4 b = *reinterpret_cast<const f32x4*>(&qs[j31][8 * u + 4 * h]);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[e], acc, 0, 0, 0);
      }
      __syncthreads();
    }
    // accumulator register r of lane (j31, h): query j31, candidate (r & 3) + 8 (r >> 2) + 4 h of the wave's 32
#pragma unroll
    for (int r = 0; r < 16; ++r) sc[j31][32 * w + (r & 3) + 8 * (r >> 2) + 4 * h] = acc[r];
    __syncthreads();
    // selection: the wave looks at a query row's 128 scores two per lane; only candidates that rank before the row's
    // current k-th entry are inserted (one at a time, in lane order)
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int ql = 8 * w + t, qi = q0 + ql;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int cl = lane + 64 * half, cj = c0 + cl;
        const float s = sc[ql][cl];
        const bool ok = cj < N && cj != qi;
        float ts = lane_bcast(ls[t], k - 1);
        int tj = __builtin_amdgcn_readlane(lj[t], k - 1);
        unsigned long long m = __ballot(ok && knn_before(s, cj, ts, tj));
        while (m) {
          const int src = __ffsll((long long)m) - 1;
          m &= m - 1;
          const float s1 = lane_bcast(s, src);
          const int j1 = c0 + src + 64 * half;
          if (knn_before(s1, j1, ts, tj)) {      // (uniform) the k-th entry may have moved since the ballot
            knn_insert(ls[t], lj[t], s1, j1, lane);
            ts = lane_bcast(ls[t], k - 1);
            tj = __builtin_amdgcn_readlane(lj[t], k - 1);
          }
        }
      }
    }
    // (the next pass writes sc only after its own staging barriers)
  }
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int qi = q0 + 8 * w + t;
    if (qi < N && lane < k) idx[(size_t)qi * k + lane] = lj[t];
  }
}

// a * (1 + beta |d_i - d_j|) as NumPy evaluates it on float32 operands: four operations, four roundings.  Plain operators under
// contract(off): the compiler's default contraction would turn 1 + beta x into one fused multiply-add.
__device__ __forceinline__ float temporal_weighted(float a, float beta, float di, float dj) {
#pragma clang fp contract(off)
  const float diff = fabsf(di - dj);
  const float scaled = beta * diff;
  const float w = 1.0f + scaled;
  return a * w;
}

// One block per row i of A (as ocr_adjacency_kernel).  a = kNN membership (KNN) or the entry already there; then, off the
// diagonal, a = (float)((double)a + alpha log1p(|set_i ^ set_j|)) where the sets meet (OCR), then a = a * (1 + beta |d_i - d_j|)
// op by op in fp32 (TEMPORAL).
__global__ __launch_bounds__(256) void dense_adj_kernel(const int32_t* __restrict__ idx, int k, const int32_t* __restrict__ offs,
                                                        const int32_t* __restrict__ toks, const float* __restrict__ delay, double alpha,
                                                        float beta, int N, float* __restrict__ adj, int ld, int flags) {
#pragma clang fp contract(off)
  __shared__ int32_t mine[SET_LDS];
  __shared__ int32_t nbr[KNN_MAX_K];
  const int i = blockIdx.x;
  const bool knn = flags & UFND_ADJ_KNN, ocr = flags & UFND_ADJ_OCR, tmp = flags & UFND_ADJ_TEMPORAL;
  int a0 = 0, na = 0;
  if (ocr) {
    a0 = offs[i];
    na = offs[i + 1] - a0;
  }
  const bool in_lds = na <= SET_LDS;
  if (in_lds)
    for (int t = threadIdx.x; t < na; t += 256) mine[t] = toks[a0 + t];
  if (knn && (int)threadIdx.x < k) nbr[threadIdx.x] = idx[(size_t)i * k + threadIdx.x];
  __syncthreads();
  const int32_t* A = in_lds ? mine : toks + a0;
  const float di = tmp ? delay[i] : 0.0f;
  const bool vec4 = (k & 3) == 0 && (reinterpret_cast<uintptr_t>(idx) & 15) == 0;      // rows of idx are 16-B aligned: 16-B loads
  float* row = adj + (size_t)i * ld;
  for (int j = threadIdx.x; j < N; j += 256) {
    float a;
    if (knn) {
      bool e = j == i;
      const int32_t* rj = idx + (size_t)j * k;       // the reverse test reads row j of idx (L2-resident: N k int32)
      if (vec4) {
        for (int t = 0; t < k; t += 4) {
          const int4 v = *reinterpret_cast<const int4*>(rj + t);
          e |= (v.x == i) | (v.y == i) | (v.z == i) | (v.w == i) | (nbr[t] == j) | (nbr[t + 1] == j) | (nbr[t + 2] == j) | (nbr[t + 3] == j);
        }
      } else {
        for (int t = 0; t < k; ++t) e |= (nbr[t] == j) | (rj[t] == i);
      }
      a = e ? 1.0f : 0.0f;
    } else {
      a = row[j];
    }
    if (j != i) {
      if (ocr && na > 0) {
        const int b0 = offs[j], nb = offs[j + 1] - b0;
        int p = 0, q = 0, ov = 0;
        while (p < na && q < nb) {       // sorted-merge intersection
          const int32_t x = A[p], y = toks[b0 + q];
          ov += (x == y);
          p += (x <= y);
          q += (y <= x);
        }
        if (ov > 0) a = (float)((double)a + alpha * log1p((double)ov));
      }
      if (tmp) a = temporal_weighted(a, beta, di, delay[j]);
    }
    row[j] = a;
  }
}

}  // namespace

extern "C" size_t ufnd_cosine_knn_workspace_floats(int N, int D, int k) {
  if (N < 1 || D < 1 || k < 1) return 0;
  return (size_t)N * knn_dp(D);
}

extern "C" int ufnd_cosine_knn(const float* X, int ldx, int N, int D, int k, int32_t* idx, float* workspace, void* stream_) {
  UFND_REQUIRE(X && idx && workspace, "cosine_knn: null argument");
  UFND_REQUIRE(N >= 1 && D >= 1 && ldx >= D, "cosine_knn: N=%d D=%d ldx=%d (N >= 1, D >= 1, ldx >= D)", N, D, ldx);
  UFND_REQUIRE(k >= 1 && k <= KNN_MAX_K, "cosine_knn: k=%d outside 1..%d", k, KNN_MAX_K);
  UFND_REQUIRE(k < N, "cosine_knn: k=%d needs k < N=%d (a row has N - 1 candidates)", k, N);
  UFND_REQUIRE(ufnd_aligned(workspace, 16), "cosine_knn: the workspace must be 16-B aligned");
  hipStream_t stream = (hipStream_t)stream_;
  const int Dp = knn_dp(D);
  hipLaunchKernelGGL(knn_normalize_kernel, dim3(ufnd_cdiv(N, 4)), dim3(256), 0, stream, X, ldx, N, D, Dp, workspace);
  UFND_CHECK_LAUNCH();
  hipLaunchKernelGGL(cosine_knn_kernel, dim3(ufnd_cdiv(N, KNN_QB)), dim3(256), 0, stream, (const float*)workspace, N, Dp, k, idx);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_dense_adj(const int32_t* idx, int k, const int32_t* offsets, const int32_t* tokens, const float* delay, double alpha,
                              double beta, int N, float* adj, int ld, int flags, void* stream_) {
  UFND_REQUIRE(adj && N >= 1 && ld >= N, "dense_adj: N=%d ld=%d", N, ld);
  UFND_REQUIRE(flags != 0 && (flags & ~(UFND_ADJ_KNN | UFND_ADJ_OCR | UFND_ADJ_TEMPORAL)) == 0, "dense_adj: flags=%d", flags);
  if (flags & UFND_ADJ_KNN) {
    UFND_REQUIRE(idx, "dense_adj: KNN needs idx");
    UFND_REQUIRE(k >= 1 && k <= KNN_MAX_K, "dense_adj: k=%d outside 1..%d", k, KNN_MAX_K);
    UFND_REQUIRE(k < N, "dense_adj: k=%d needs k < N=%d", k, N);
  }
  UFND_REQUIRE(!(flags & UFND_ADJ_OCR) || (offsets && tokens), "dense_adj: OCR needs offsets / tokens");
  UFND_REQUIRE(!(flags & UFND_ADJ_TEMPORAL) || delay, "dense_adj: TEMPORAL needs delay");
  hipLaunchKernelGGL(dense_adj_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream_, idx, k, offsets, tokens, delay, alpha, (float)beta, N,
                     adj, ld, flags);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}
