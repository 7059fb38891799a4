// A/V lag estimation, the lip-sync signal of the reference (TemporalSyncNet.estimate_av_lag, src/core_blocks/temporal_blocks.py:176-223,
// and ChronosGuard.estimate_av_lag, src/models/chronos_guard.py:175-196), batched on the device: the lag at which an audio envelope
// and a mouth-opening series correlate best inside +-max_lag samples.  The reference spends three FFTs of >= 2 n points to read a
// window of 2 max_lag + 1 lags; this is the DIRECT windowed correlation, an exact fp32 fmaf chain per value (include/ultrafnd_hip.h
// states the arithmetic).  For pair b:  n = min(len_a, len_m),  Kc = min(max_lag, n - 1),
//     c[k] = sum_i ahat[i + k] mhat[i]   over the i with both indices in 0 .. n - 1,   k = -Kc .. Kc,   lag = argmax_k c[k] (lowest k).
// Three launches:
//   standardise_kernel   grid (B, 2), 1024 threads: one signal of one pair.  Sum and sum of squared deviations in double (thread t adds
//                        x[t], x[t + 1024], ... in ascending order, then the 1024 partials fold by halves, 512 .. 1); mean and std
//                        rounded to fp32;  xhat = (x - mean) / (std + 1e-9f)  in fp32, zeros from n to the padded row end.
//   correlate_kernel     grid (lag blocks of 1024, segments of 2048, B), 128 threads.  The hot path, structurally the FIR of
//                        resample.hip: the workgroup stages ahat[seg0 + kb .. seg0 + kb + 2048 + 1024) into LDS (zero outside 0 .. n - 1
//                        by index), a wave owns 512 lags, lane l the 8 consecutive lags kw + 8 l .. kw + 8 l + 7.  Per step of 8 samples
//                        the lane reads TWO 16-byte vectors from LDS (the register window of 16 slides by 8), the wave fetches
//                        mhat[i .. i + 7] through a wave-uniform address and issues 64 fmaf.  A wave walks only the i for which one
//                        of its lags has both indices inside the pair (the triangle of a full window is not computed).
//   finish_kernel        grid (B), 1024 threads: folds the segment partials in ascending segment order, takes the argmax under the tie
//                        rule, writes the peak, the -inf padding of xcorr and the lag.
//
// One value, one arithmetic.  P[s][k] is ONE chain of fmaf from +0 over the i of segment s (i in [2048 s, 2048 (s + 1)) and < n) in
// ASCENDING i:  acc = fmaf(ahat[i + k], mhat[i], acc);  the terms with i + k outside 0 .. n - 1 multiply a staged zero and leave acc's
// value unchanged.  c[k] = ((P[0][k] + P[1][k]) + ...) + P[S - 1][k] + 0.0f,  S = ceil(n / 2048), plain fp32 additions in ascending
// s; the closing + 0.0f makes a zero +0 whatever the signs of the zero terms were.  The order depends on (n, k) alone: not on B, the
// row, other rows' lengths, max_lag or the launch geometry.  No atomics, no scratch, no host synchronisation; hipGraph-capturable;
// lengths are read on the device only and clamped to the row width; nothing at or past a row's length is read.
#include <math.h>

#include "common.hpp"

namespace {

constexpr int SEG = UFND_AVLAG_SEGMENT;             // samples i of one partial chain
constexpr int LB = UFND_AVLAG_LAG_BLOCK;            // lags of a workgroup
constexpr int R = 8;                                // consecutive lags of a lane
constexpr int US = 8;                               // samples of a loop step
constexpr int CT = 128, WAVES = CT / 64, WL = 64 * R;      // correlate: threads, waves, lags of a wave
constexpr int RT = 1024;                            // threads of the two row kernels: the fold order of the statistics is tied to it
static_assert(WAVES * WL == LB && SEG % US == 0 && LB % 4 == 0 && R % 4 == 0 && US == 8, "a wave per 512 lags; 16-byte LDS reads");

__device__ __forceinline__ int pair_len(const int32_t* len_a, const int32_t* len_m, int b, int na_max, int nm_max) {
  int la = len_a ? len_a[b] : na_max, lm = len_m ? len_m[b] : nm_max;
  la = la < 0 ? 0 : (la > na_max ? na_max : la);
  lm = lm < 0 ? 0 : (lm > nm_max ? nm_max : lm);
  return la < lm ? la : lm;
}

// the workspace: offsets in bytes
struct Layout {
  size_t astd, mstd, part, bytes;
  int nw, nwp, S, LJ;
};
__host__ inline Layout layout(int B, int n_max, int max_lag) {
  Layout l;
  l.nw = n_max;
  l.nwp = (n_max + US - 1) / US * US;
  l.S = ufnd_cdiv(n_max, SEG);
  l.LJ = 2 * max_lag + 1;
  size_t o = 0;
  auto take = [&](size_t n) {
    const size_t at = o;
    o += (n + 15) / 16 * 16;
    return at;
  };
  l.astd = take((size_t)B * l.nwp * sizeof(float));
  l.mstd = take((size_t)B * l.nwp * sizeof(float));
  l.part = take((size_t)B * l.S * l.LJ * sizeof(float));
  l.bytes = o;
  return l;
}

// the sum of the block's values: the 1024 partials fold by halves, red[t] += red[t + o] for o = 512 .. 1
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();      // (red may still be read from the previous fold)
  red[tid] = v;
  __syncthreads();
  for (int o = RT / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] = red[tid] + red[tid + o];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(RT) void standardise_kernel(const float* __restrict__ a, long long a_stride, const float* __restrict__ m, long long m_stride,
                                                         const int32_t* __restrict__ len_a, const int32_t* __restrict__ len_m, float* __restrict__ ws_a,
                                                         float* __restrict__ ws_m, float* __restrict__ out_a, float* __restrict__ out_m, int na_max,
                                                         int nm_max, int nw, int nwp) {
  __shared__ double red[RT];
  const int tid = threadIdx.x, b = blockIdx.x, which = blockIdx.y;
  const int n = pair_len(len_a, len_m, b, na_max, nm_max);
  const float* x = which ? m + (long long)b * m_stride : a + (long long)b * a_stride;
  float* ws = (which ? ws_m : ws_a) + (size_t)b * nwp;
  float* out = which ? out_m : out_a;
  if (out) out += (size_t)b * nw;
  if (n < 4) {      // (uniform) the reference returns before it standardises: zeros, and the row's workspace is never read
    if (out)
      for (int i = tid; i < nw; i += RT) out[i] = 0.0f;
    return;
  }
  double s = 0.0;
  for (int i = tid; i < n; i += RT) s = s + (double)x[i];
  const double mean = block_sum(s, red) / (double)n;
  double q = 0.0;
  for (int i = tid; i < n; i += RT) {
    const double d = (double)x[i] - mean;
    q = q + d * d;      // (this file is built with contraction off: a product, then a sum)
  }
  const double var = block_sum(q, red) / (double)n;
  const float mean32 = (float)mean, den = (float)sqrt(var) + 1e-9f;
  for (int i = tid; i < nwp; i += RT) {
    const float v = i < n ? (x[i] - mean32) / den : 0.0f;
    ws[i] = v;
    if (out && i < nw) out[i] = v;
  }
}

__global__ __launch_bounds__(CT) void correlate_kernel(const float* __restrict__ astd, const float* __restrict__ mstd, const int32_t* __restrict__ len_a,
                                                       const int32_t* __restrict__ len_m, float* __restrict__ part, int na_max, int nm_max, int nwp,
                                                       int K, int S, int LJ) {
  __shared__ __attribute__((aligned(16))) float xs[SEG + LB];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int blk = blockIdx.x, s = blockIdx.y, b = blockIdx.z;
  const int n = pair_len(len_a, len_m, b, na_max, nm_max);
  const int seg0 = s * SEG;
  if (n < 4 || seg0 >= n) return;      // (uniform) the finish reads no partial of this segment
  const int Kc = K < n - 1 ? K : n - 1;
  const int j0 = blk * LB, kb = j0 - K;      // the block's first column and its lag
  if (kb > Kc || kb + LB - 1 < -Kc) return;      // (uniform) no lag of the pair's window here

  const float* arow = astd + (size_t)b * nwp;
  for (int t = tid; t < SEG + LB; t += CT) {      // xs[t] = ahat[seg0 + kb + t], zero outside the pair
    const int g = seg0 + kb + t;
    xs[t] = (g >= 0 && g < n) ? arow[g] : 0.0f;
  }
  __syncthreads();

  const int kw = kb + wave * WL;      // the wave's first lag
  if (kw > Kc || kw + WL - 1 < -Kc) return;      // (wave-uniform, after the only barrier)
  const int seg1 = seg0 + SEG < n ? seg0 + SEG : n;
  int i_lo = -(kw + WL - 1), i_hi = n - kw;      // the i for which some lag of the wave has 0 <= i + k < n ...
  i_lo = i_lo < seg0 ? seg0 : (i_lo & ~(US - 1));      // ... inside the segment, rounded out to steps of 8 (the extra terms are zeros)
  i_hi = i_hi > seg1 ? seg1 : i_hi;
  i_hi = (i_hi + US - 1) & ~(US - 1);                  // <= the padded row: mhat holds zeros from n on
  float acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.0f;
  if (i_lo < i_hi) {
    const float* xp = xs + wave * WL + lane * R;      // indexed by i - seg0: xp[i - seg0 + r] = ahat[i + k_r]
    const float* mrow = mstd + (size_t)b * nwp;       // indexed by i (wave-uniform)
    f32x4 w0 = *reinterpret_cast<const f32x4*>(xp + (i_lo - seg0)), w1 = *reinterpret_cast<const f32x4*>(xp + (i_lo - seg0) + 4);
    for (int i = i_lo; i < i_hi; i += US) {
      const f32x4 w2 = *reinterpret_cast<const f32x4*>(xp + (i - seg0) + 8), w3 = *reinterpret_cast<const f32x4*>(xp + (i - seg0) + 12);
      const f32x4 ma = *reinterpret_cast<const f32x4*>(mrow + i), mb = *reinterpret_cast<const f32x4*>(mrow + i + 4);
      const float w[16] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3], w2[0], w2[1], w2[2], w2[3], w3[0], w3[1], w3[2], w3[3]};
      const float mv[US] = {ma[0], ma[1], ma[2], ma[3], mb[0], mb[1], mb[2], mb[3]};
#pragma unroll
      for (int u = 0; u < US; ++u) {
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = fmaf(w[u + r], mv[u], acc[r]);
      }
      w0 = w2, w1 = w3;
    }
  }
  const int j = j0 + wave * WL + lane * R;
  float* out = part + ((size_t)b * S + s) * LJ;
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (j + r < LJ) out[j + r] = acc[r];
}

__global__ __launch_bounds__(RT) void finish_kernel(const float* __restrict__ part, const int32_t* __restrict__ len_a, const int32_t* __restrict__ len_m,
                                                    int32_t* __restrict__ lag_samples, float* __restrict__ peak_corr, float* __restrict__ xcorr,
                                                    int na_max, int nm_max, int K, int S, int LJ) {
  __shared__ float bv[RT];
  __shared__ int bj[RT];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int n = pair_len(len_a, len_m, b, na_max, nm_max);
  const bool on = n >= 4;
  const int Kc = K < n - 1 ? K : n - 1;
  const int Sb = (n + SEG - 1) / SEG;
  const float* p = part + (size_t)b * S * LJ;
  float best = -INFINITY;
  int best_j = 0x7fffffff;
  for (int j = tid; j < LJ; j += RT) {      // ascending j per thread: `>` keeps the lowest of equals
    const int k = j - K;
    float c = -INFINITY;
    if (on && k >= -Kc && k <= Kc) {
      c = p[j];
      for (int s = 1; s < Sb; ++s) c = c + p[(size_t)s * LJ + j];
      c = c + 0.0f;
      if (c > best) best = c, best_j = j;
    }
    if (xcorr) xcorr[(size_t)b * LJ + j] = c;
  }
  bv[tid] = best, bj[tid] = best_j;
  __syncthreads();
  for (int o = RT / 2; o > 0; o >>= 1) {
    if (tid < o) {
      const float v = bv[tid + o];
      const int j = bj[tid + o];
      if (v > bv[tid] || (v == bv[tid] && j < bj[tid])) bv[tid] = v, bj[tid] = j;
    }
    __syncthreads();
  }
  if (tid == 0) {
    const bool found = on && bj[0] != 0x7fffffff;      // (a window of non-finite values only: outside the contract, lag 0)
    if (lag_samples) lag_samples[b] = found ? bj[0] - K : 0;
    if (peak_corr) peak_corr[b] = found ? bv[0] / (float)n : 0.0f;
  }
}

bool shape_ok(int B, int n_max, int max_lag) {
  if (!(B >= 1 && B <= UFND_AVLAG_MAX_B && n_max >= 1 && n_max <= UFND_AVLAG_MAX_N && max_lag >= 0 && max_lag <= UFND_AVLAG_MAX_LAG)) return false;
  return (long long)B * ufnd_cdiv(n_max, SEG) * (2ll * max_lag + 1) <= UFND_AVLAG_MAX_PARTIAL_FLOATS;
}

}  // namespace

extern "C" size_t ufnd_av_lag_workspace_bytes(int B, int n_max, int max_lag) { return shape_ok(B, n_max, max_lag) ? layout(B, n_max, max_lag).bytes : 0; }

extern "C" int ufnd_av_lag(const float* a, int64_t a_row_stride, const float* m, int64_t m_row_stride, const int32_t* len_a, const int32_t* len_m,
                           void* workspace, int32_t* lag_samples, float* peak_corr, float* xcorr, float* a_std, float* m_std, int B, int na_max,
                           int nm_max, int max_lag, void* stream_) {
  UFND_REQUIRE(a && m && workspace, "av_lag: null argument (a, m, workspace)");
  UFND_REQUIRE(lag_samples || peak_corr || xcorr || a_std || m_std, "av_lag: no output asked for (lag_samples, peak_corr, xcorr, a_std, m_std)");
  UFND_REQUIRE(B >= 1 && B <= UFND_AVLAG_MAX_B, "av_lag: B=%d (1 <= B <= %d pairs)", B, UFND_AVLAG_MAX_B);
  UFND_REQUIRE(na_max >= 1 && na_max <= UFND_AVLAG_MAX_N && nm_max >= 1 && nm_max <= UFND_AVLAG_MAX_N,
               "av_lag: na_max=%d nm_max=%d (rows of 1 .. 2^26 samples)", na_max, nm_max);
  UFND_REQUIRE(max_lag >= 0 && max_lag <= UFND_AVLAG_MAX_LAG, "av_lag: max_lag=%d (0 <= max_lag <= 2^26 samples)", max_lag);
  const int n_max = na_max < nm_max ? na_max : nm_max;
  UFND_REQUIRE(shape_ok(B, n_max, max_lag), "av_lag: partials=%lld floats (B ceil(min(na_max, nm_max) / %d) (2 max_lag + 1) <= 2^31)",
               (long long)B * ufnd_cdiv(n_max, SEG) * (2ll * max_lag + 1), SEG);
  UFND_REQUIRE(a_row_stride >= 0 && m_row_stride >= 0, "av_lag: negative row stride");
  UFND_REQUIRE(ufnd_aligned(workspace, 16) && ufnd_aligned(a, 4) && ufnd_aligned(m, 4), "av_lag: alignment (workspace: 16 bytes; a, m: 4 bytes)");
  hipStream_t stream = (hipStream_t)stream_;
  const Layout l = layout(B, n_max, max_lag);
  float* ws_a = (float*)((char*)workspace + l.astd);
  float* ws_m = (float*)((char*)workspace + l.mstd);
  float* part = (float*)((char*)workspace + l.part);
  hipLaunchKernelGGL(standardise_kernel, dim3(B, 2), dim3(RT), 0, stream, a, (long long)a_row_stride, m, (long long)m_row_stride, len_a, len_m, ws_a, ws_m,
                     a_std, m_std, na_max, nm_max, l.nw, l.nwp);
  UFND_CHECK_LAUNCH();
  if (lag_samples || peak_corr || xcorr) {
    hipLaunchKernelGGL(correlate_kernel, dim3(ufnd_cdiv(l.LJ, LB), l.S, B), dim3(CT), 0, stream, ws_a, ws_m, len_a, len_m, part, na_max, nm_max, l.nwp,
                       max_lag, l.S, l.LJ);
    UFND_CHECK_LAUNCH();
    hipLaunchKernelGGL(finish_kernel, dim3(B), dim3(RT), 0, stream, part, len_a, len_m, lag_samples, peak_corr, xcorr, na_max, nm_max, max_lag, l.S, l.LJ);
    UFND_CHECK_LAUNCH();
  }
  return UFND_OK;
}
