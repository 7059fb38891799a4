// Device helpers of the row-wise kernels (one wave per row of H = 256 NI columns, 16-B loads, fp32 statistics) and the host
// pieces of their launches: encoders.hip, encoders_bwd.hip, clip_text.hip, audio.hip, explain_inputs.hip, tier_a.hip.
// Include it at the top of a file, in front of any `clang fp contract` pragma: the helpers are compiled with the default
// contraction whoever calls them (ln_row and row_stats are the only ones with a multiply next to an add), so a row gets the
// same bits from every kernel.
#pragma once
#include "common.hpp"

namespace {

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// normalise NI*4 values per lane (row of H = 256*NI) held in v[]; returns via v[]
template <int NI>
__device__ __forceinline__ void ln_row(f32x4 (&v)[NI], int H, float eps, const float* gamma, const float* beta, int lane) {
  float s = 0.0f;
#pragma unroll
  for (int i = 0; i < NI; ++i) s += v[i][0] + v[i][1] + v[i][2] + v[i][3];
  const float mean = wave_sum(s) / (float)H;
  float q = 0.0f;
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float d = v[i][k] - mean;
      q += d * d;
    }
  const float rstd = rsqrtf(wave_sum(q) / (float)H + eps);
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int col = 4 * lane + 256 * i;
    const f32x4 gm = ld4(gamma + col), bt = ld4(beta + col);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[i][k] = (v[i][k] - mean) * rstd * gm[k] + bt[k];
  }
}

template <int NI>
__device__ __forceinline__ void store_row(const f32x4 (&v)[NI], __bf16* ob, float* of, size_t row, int H, int lane) {
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int col = 4 * lane + 256 * i;
    if (of) *reinterpret_cast<f32x4*>(of + row * H + col) = v[i];
    if (ob) {
      bf16x4 o = {(__bf16)v[i][0], (__bf16)v[i][1], (__bf16)v[i][2], (__bf16)v[i][3]};
      *reinterpret_cast<bf16x4*>(ob + row * H + col) = o;
    }
  }
}

// {sum, sum of squares} of the row held in v[] -> stats[row] as TWO partials ({s, q}, {0, 0}): the
// layout ufnd_gemm_bf16_ln reads its a_stats in (even partial counts)
template <int NI>
__device__ __forceinline__ void row_stats(const f32x4 (&v)[NI], float* stats, size_t row, int lane) {
  float s = 0.0f, q = 0.0f;
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) { s += v[i][k]; q += v[i][k] * v[i][k]; }
  s = wave_sum(s);
  q = wave_sum(q);
  if (lane == 0) *reinterpret_cast<f32x4*>(stats + row * 4) = f32x4{s, q, 0.0f, 0.0f};
}

// block-wide sum of a 256-thread workgroup in a fixed order: DPP wave sums, then the four waves' totals in wave order.  The
// barrier in front lets a caller reuse `red` from one sum to the next.
__device__ __forceinline__ float block_sum4(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// sum of x[i]^2 over a clip's first n samples by a 256-thread workgroup: thread t adds the squares of samples t, t + 256, ... in
// order (one fmaf each), then block_sum4's tree (ufnd_audio_arousal, ufnd_wave_energy)
__device__ __forceinline__ float block_square_sum(const float* row, int n, float* red) {
  float q = 0.0f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float v = row[i];
    q = fmaf(v, v, q);
  }
  return block_sum4(q, red);
}

// The pack kernels (ufnd_text_pack, ufnd_clip_text_pack): ONE workgroup of PACK_THREADS threads over up to PACK_MAX_B samples.
// In: lens[b] = n_b, the rows sample b keeps, written by all threads and not yet synchronised.  Out: cu = the exclusive prefix
// sum of n_b in a fixed order (cu[B] = the live row count, which is returned), lens[b] = cu[b], and
// row_src[cu[b] + l] = b L + l for l < n_b.  Thread t scans the contiguous samples [t per, (t + 1) per).
constexpr int PACK_THREADS = 1024, PACK_MAX_B = 16384;
__device__ __forceinline__ int pack_scan_rows(int* lens, int B, int L, int32_t* cu, int32_t* row_src) {
  __shared__ int wsum[PACK_THREADS / 64];
  __shared__ int total;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  __syncthreads();
  const int per = (B + PACK_THREADS - 1) / PACK_THREADS, b0 = tid * per, b1 = min(b0 + per, B);
  int own = 0;
  for (int b = b0; b < b1; ++b) own += lens[b];
  int inc = own;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(inc, o, 64);
    if (lane >= o) inc += y;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += wsum[w];
  int run = base + inc - own;
  for (int b = b0; b < b1; ++b) {
    const int n = lens[b];
    lens[b] = run;      // (only this thread touches its samples' slots)
    cu[b] = run;
    run += n;
  }
  if (tid == PACK_THREADS - 1) {
    cu[B] = run;
    total = run;
  }
  __syncthreads();
  const int all = total;
  for (int b = wave; b < B; b += PACK_THREADS / 64) {
    const int r0 = lens[b], n = (b + 1 < B ? lens[b + 1] : all) - r0;
    for (int l = lane; l < n; l += 64) row_src[r0 + l] = b * L + l;
  }
  return all;
}

// a row kernel's H: 256 NI columns, NI = 1 .. 4
inline bool h_ok(int H) { return H == 256 || H == 512 || H == 768 || H == 1024; }

}  // namespace

// launch KERNEL<NI> (256 threads) for a row width H that h_ok() accepted
#define NI_LAUNCH(H, KERNEL, GRID, STREAM, ...)                                                       \
  do {                                                                                                \
    if ((H) == 256) hipLaunchKernelGGL((KERNEL<1>), GRID, dim3(256), 0, STREAM, __VA_ARGS__);         \
    else if ((H) == 512) hipLaunchKernelGGL((KERNEL<2>), GRID, dim3(256), 0, STREAM, __VA_ARGS__);    \
    else if ((H) == 768) hipLaunchKernelGGL((KERNEL<3>), GRID, dim3(256), 0, STREAM, __VA_ARGS__);    \
    else hipLaunchKernelGGL((KERNEL<4>), GRID, dim3(256), 0, STREAM, __VA_ARGS__);                    \
  } while (0)

// the same over a kernel with a second template argument T
#define NI_LAUNCH_T(H, KERNEL, T, GRID, STREAM, ...)                                                       \
  do {                                                                                                     \
    if ((H) == 256) hipLaunchKernelGGL((KERNEL<1, T>), GRID, dim3(256), 0, STREAM, __VA_ARGS__);           \
    else if ((H) == 512) hipLaunchKernelGGL((KERNEL<2, T>), GRID, dim3(256), 0, STREAM, __VA_ARGS__);      \
    else if ((H) == 768) hipLaunchKernelGGL((KERNEL<3, T>), GRID, dim3(256), 0, STREAM, __VA_ARGS__);      \
    else hipLaunchKernelGGL((KERNEL<4, T>), GRID, dim3(256), 0, STREAM, __VA_ARGS__);                      \
  } while (0)
