// The reference's librosa branches (src/core_blocks/audio_blocks.py), batched on the device:
//   SpectralForensics._librosa_spectral  :141-176  11 descriptors of a 16 kHz clip, tiled to dim and L2-normalised
//   VoiceCloneDetector.score             :244-254  0.4 mean(flatness) + 0.3 mean(zcr) + 0.3 tanh(mean(centroid) / 3000), clipped
// The definitions are restated from librosa's documented algorithms (0.10 defaults; include/ultrafnd_hip.h spells them out) and are
// NOT verified against librosa itself.  Two STFTs, both with a periodic Hann window and ZERO padding (center=True):
//   path A   n_fft 400, hop 160, 201 bins: magnitude statistics, spectral contrast, spectral flatness.  The 64-frame x 201-bin tile
//            form of csrc/spectral.hip: the window is folded into the (402, 400) basis on the host, staging zero-pads where that
//            kernel mirrors, and the epilogue reads the LDS tile per frame (7 band peaks and valleys, flatness) and per tile (the
//            statistics partials).
//   path B   n_fft 2048, hop 512, 1025 bins: centroid, rolloff, flatness.  The same exact-fp32 DFT-GEMM with K = 2048: a workgroup
//            owns 32 frames of one clip (their overlapping samples, 72 KB of LDS) and 4 of the 33 bin blocks, streams the
//            (2050, 2048) basis through LDS in 32-tap slabs and writes magnitudes frame-major to the workspace; a second launch
//            reduces every frame over its ascending bins in double.
// plus a VALU kernel for the zero-crossing counts (edge padding, integers) and one finish workgroup per clip.
//
// One value, one arithmetic: re and im of a (frame, bin) are each ONE chain of n_fft fmaf from zero, in the tap order
// 8u + e, 8u + 4 + e (u = 0 .. n_fft / 8 - 1, e = 0 .. 3), whatever the tile, the batch or the outputs asked for;
// |S| = sqrtf(fmaf(re, re, im * im)).  No atomics; every reduction is a fixed order in double.  A clip is computed as if alone and
// nothing at or past x[len] is read.
#include <float.h>
#include <limits.h>

#include "common.hpp"

namespace {

constexpr int DESC = 11;
// ---- path A (the tile geometry of csrc/spectral.hip)
constexpr int NFFT = 400, HOP = 160, BINS = 201, PAD = 200, NBAND = 7;
constexpr int FT = UFND_DESC_FRAME_TILE_A;
constexpr int BIN_BLOCKS = 7, ROUNDS = 4, KC = 40, SLABS = NFFT / KC, BLD = KC + 4, ALD = HOP + 4;
constexpr int A_FLOATS = ALD * (FT - 1) + NFFT + 8 + 4;
constexpr int MLD = FT + 1;
constexpr int PART = 4;      // doubles per tile partial: sum, centred second moment, max, min
static_assert(FT == 64 && HOP % KC == 0 && NFFT % KC == 0 && KC % 8 == 0 && (128 * KC / 4) % 256 == 0, "tile geometry (A)");
// ---- path B
constexpr int NFFT2 = 2048, HOP2 = 512, BINS2 = 1025, PAD2 = 1024;
constexpr int FT2 = UFND_DESC_FRAME_TILE_B;      // frames of a workgroup: one 32-row MFMA block
constexpr int BIN_BLOCKS2 = 33;                  // 32-bin blocks (1056 columns; the basis of bins 1025 .. 1055 is zero)
constexpr int GROUPS2 = 9;                       // workgroups over the bins: wave w of group g owns bin block 4 g + w
constexpr int MAG_LD = 32 * BIN_BLOCKS2;         // row stride of the frame-major magnitudes in the workspace
constexpr int KC2 = 32, SLABS2 = NFFT2 / KC2;
constexpr int BLD2 = KC2 + 4;                    // 9 x 16 B, odd: 16-B reads of 32 rows spread over all banks
constexpr int ALD2 = HOP2 + 4;                   // 129 x 16 B, odd: frame i starts at 516 i
constexpr int A2_FLOATS = ALD2 * (FT2 - 1) + NFFT2 + 4 * (NFFT2 / HOP2 - 1);
constexpr int CHUNK2 = 17;                       // bins of a lane in the per-frame reduction: 64 x 17 >= 1025
static_assert(FT2 == 32 && HOP2 % KC2 == 0 && KC2 % 8 == 0 && (256 * KC2 / 4) % 256 == 0 && 64 * CHUNK2 >= BINS2, "tile geometry (B)");
constexpr double BIN_HZ2 = 16000.0 / NFFT2;      // 7.8125, exact

__host__ __device__ inline int frames_a(int len) { return len >= 1 ? 1 + len / HOP : 0; }
__host__ __device__ inline int frames_b(int len) { return len >= 1 ? 1 + len / HOP2 : 0; }
__device__ __forceinline__ int clip_len(const int32_t* lengths, int b, int n_max) {
  const int n = lengths ? lengths[b] : n_max;
  return n < 0 ? 0 : (n > n_max ? n_max : n);
}

// the workspace: offsets in bytes, doubles first
struct Layout {
  size_t partials, peak, valley, flat_a, cent, roll, flat_b, zc, mag_b, bytes;
  int TA, TB, tiles_a, tiles_b;
};
__host__ inline Layout layout(int B, int n_max) {
  Layout l;
  l.TA = 1 + n_max / HOP;
  l.TB = 1 + n_max / HOP2;
  l.tiles_a = ufnd_cdiv(l.TA, FT);
  l.tiles_b = ufnd_cdiv(l.TB, FT2);
  size_t o = 0;
  auto take = [&](size_t n) {
    const size_t at = o;
    o += (n + 15) / 16 * 16;
    return at;
  };
  l.partials = take((size_t)B * l.tiles_a * PART * sizeof(double));
  l.peak = take((size_t)B * NBAND * l.TA * sizeof(float));
  l.valley = take((size_t)B * NBAND * l.TA * sizeof(float));
  l.flat_a = take((size_t)B * l.TA * sizeof(float));
  l.cent = take((size_t)B * l.TB * sizeof(float));
  l.roll = take((size_t)B * l.TB * sizeof(float));
  l.flat_b = take((size_t)B * l.TB * sizeof(float));
  l.zc = take((size_t)B * l.TB * sizeof(int32_t));
  l.mag_b = take((size_t)B * l.tiles_b * FT2 * MAG_LD * sizeof(float));
  l.bytes = o;
  return l;
}

// block-wide reduction of one double per thread (256 threads) by a fixed binary tree in LDS; every thread returns the total
template <class Op>
__device__ __forceinline__ double block_tree(double v, double* red, Op op) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = op(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  return red[0];
}
__device__ __forceinline__ double dadd(double x, double y) { return x + y; }
__device__ __forceinline__ double dmax(double x, double y) { return fmax(x, y); }

// exp(mean log P) / mean P from the two sums over n bins
__device__ __forceinline__ float flatness_of(double sum_log, double sum_p, int n) { return (float)(exp(sum_log / (double)n) / (sum_p / (double)n)); }
__device__ __forceinline__ double power_of(float s) { return fmax(1e-10, (double)s * (double)s); }

// ---------------------------------------------------------------------------------------------------------------- path A
__global__ __launch_bounds__(256) void desc_a_kernel(const float* __restrict__ waves, const int32_t* __restrict__ lengths,
                                                     const float* __restrict__ basis, double* __restrict__ partials, float* __restrict__ peak,
                                                     float* __restrict__ valley, float* __restrict__ flat, float* __restrict__ magnitude,
                                                     float* __restrict__ flat_out, int n_max, int T_max, int tiles_max) {
  __shared__ __attribute__((aligned(16))) float as[A_FLOATS];
  __shared__ __attribute__((aligned(16))) float bs[128 * BLD];
  __shared__ float ms[BINS * MLD];
  __shared__ double red[256];
  const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
  const int len = clip_len(lengths, b, n_max);
  const int f0 = tile * FT;
  const int Tb = frames_a(len);
  const int fv = min(max(Tb - f0, 0), FT);      // the clip's frames in this tile
  const int fo = min(T_max - f0, FT);           // output columns of this tile (zeros from fv on)
  float* mag_out = magnitude ? magnitude + (size_t)b * BINS * T_max + f0 : nullptr;
  float* fl_out = flat_out ? flat_out + (size_t)b * T_max + f0 : nullptr;

  if (fl_out && tid < fo && tid >= fv) fl_out[tid] = 0.0f;
  if (fv == 0) {      // (uniform) nothing of the clip here: the outputs' zero padding; the finish kernel counts tiles and frames from T_b
    if (mag_out)
      for (int idx = tid; idx < BINS * FT; idx += 256) {
        const int row = idx >> 6, f = idx & 63;
        if (f < fo) mag_out[(size_t)row * T_max + f] = 0.0f;
      }
    return;
  }

  // ---- the A operand: padded samples p0 .. p0 + 63 * 160 + 399 of the clip, zeros outside [0, len); nothing at or past x[len] is read
  {
    const float* x = waves + (size_t)b * n_max;
    const int p0 = f0 * HOP;
    constexpr int SPAN = (FT - 1) * HOP + NFFT, BATCH = 21;
    for (int s0 = tid; s0 < SPAN; s0 += 256 * BATCH) {
      float v[BATCH];
#pragma unroll
      for (int j = 0; j < BATCH; ++j) {      // branch-free: a sample outside the clip loads x[0] and stores zero
        const int i = p0 + s0 + 256 * j - PAD;
        const bool ok = s0 + 256 * j < SPAN && i >= 0 && i < len;
        v[j] = x[ok ? i : 0];
        v[j] = ok ? v[j] : 0.0f;
      }
#pragma unroll
      for (int j = 0; j < BATCH; ++j) {
        const int s = s0 + 256 * j;
        if (s < SPAN) as[s + 4 * (s / HOP)] = v[j];
      }
    }
  }

  const int w = tid >> 6, lane = tid & 63, j31 = lane & 31, h = lane >> 5, fb = w & 1, g = w >> 1;
  // staging of a slab: 128 columns (bin block 2 r: cos, -sin; bin block 2 r + 1: cos, -sin) x 40 taps, five 16-B pieces per thread
  f32x4 pre[5];
  auto fetch = [&](int r, int kc) {
#pragma unroll
    for (int m = 0; m < 5; ++m) {
      const int q = tid + 256 * m, lc = q / (KC / 4), kq = (q % (KC / 4)) * 4;
      const int bin = 32 * (2 * r + (lc >> 6)) + (lc & 31), part = (lc >> 5) & 1;
      const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
      pre[m] = bin < BINS ? *reinterpret_cast<const f32x4*>(basis + (size_t)(part * BINS + bin) * NFFT + kc * KC + kq) : zero;
    }
  };
  fetch(0, 0);
  for (int r = 0; r < ROUNDS; ++r) {
    const int bb = 2 * r + g;
    const bool live = bb < BIN_BLOCKS;
    f32x16 re, im;
#pragma unroll
    for (int q = 0; q < 16; ++q) re[q] = im[q] = 0.0f;
    for (int kc = 0; kc < SLABS; ++kc) {
#pragma unroll
      for (int m = 0; m < 5; ++m) {
        const int q = tid + 256 * m;
        *reinterpret_cast<f32x4*>(&bs[(q / (KC / 4)) * BLD + (q % (KC / 4)) * 4]) = pre[m];
      }
      __syncthreads();      // (the first one also publishes `as`)
      if (kc + 1 < SLABS) {
        fetch(r, kc + 1);
      } else if (r + 1 < ROUNDS) {
        fetch(r + 1, 0);
      }
      if (live) {
        // frame 32 fb + j31, taps 40 kc + 8 u + 4 h + e: half h of the wave feeds the second tap of MFMA step (u, e)
        const float* ap = as + ALD * (32 * fb + j31) + kc * KC + 4 * (kc >> 2) + 4 * h;
        const float* bre = bs + (64 * g + j31) * BLD + 4 * h;
        const float* bim = bre + 32 * BLD;
#pragma unroll
        for (int u = 0; u < KC / 8; ++u) {
          const f32x4 a = *reinterpret_cast<const f32x4*>(ap + 8 * u);
          const f32x4 c = *reinterpret_cast<const f32x4*>(bre + 8 * u);
          const f32x4 s = *reinterpret_cast<const f32x4*>(bim + 8 * u);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            re = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], c[e], re, 0, 0, 0);
            im = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], s[e], im, 0, 0, 0);
          }
        }
      }
      __syncthreads();
    }
    // accumulator register q of lane (j31, h): frame (q & 3) + 8 (q >> 2) + 4 h of the wave's 32, bin 32 bb + j31
    const int bin = 32 * bb + j31;
    if (live && bin < BINS) {
#pragma unroll
      for (int q = 0; q < 16; ++q)
        ms[bin * MLD + 32 * fb + (q & 3) + 8 * (q >> 2) + 4 * h] = sqrtf(fmaf(re[q], re[q], im[q] * im[q]));
    }
  }
  __syncthreads();

  // ---- outputs, all from the tile in LDS
  if (mag_out) {
    for (int idx = tid; idx < BINS * FT; idx += 256) {
      const int bin = idx >> 6, f = idx & 63;
      if (f < fo) mag_out[(size_t)bin * T_max + f] = f < fv ? ms[bin * MLD + f] : 0.0f;
    }
  }
  // per frame: task k < 7 is octave band k (peak = mean of the idx largest, valley = mean of the idx smallest of its rows; idx = 2 for
  // band 5, else 1), task 7 the flatness over the 201 bins in ascending order
  for (int idx = tid; idx < (NBAND + 1) * FT; idx += 256) {
    const int f = idx & 63, k = idx >> 6;
    if (f >= fv) continue;
    if (k < NBAND) {
      const int lo = k == 0 ? 0 : (5 << (k - 1)) - 1, hi = k == NBAND - 1 ? BINS - 1 : (5 << k) - 1;      // rows lo .. hi
      float s1 = INFINITY, s2 = INFINITY, l1 = -INFINITY, l2 = -INFINITY;      // two smallest (s1 <= s2), two largest (l1 >= l2)
      for (int bin = lo; bin <= hi; ++bin) {
        const float v = ms[bin * MLD + f];
        if (v < s1) {
          s2 = s1;
          s1 = v;
        } else if (v < s2) {
          s2 = v;
        }
        if (v > l1) {
          l2 = l1;
          l1 = v;
        } else if (v > l2) {
          l2 = v;
        }
      }
      const bool two = k == 5;
      const size_t at = ((size_t)b * NBAND + k) * T_max + f0 + f;
      valley[at] = two ? (s1 + s2) * 0.5f : s1;
      peak[at] = two ? (l1 + l2) * 0.5f : l1;
    } else {
      double sl = 0.0, sp = 0.0;
      for (int bin = 0; bin < BINS; ++bin) {
        const double p = power_of(ms[bin * MLD + f]);
        sl += log(p);
        sp += p;
      }
      const float v = flatness_of(sl, sp, BINS);
      flat[(size_t)b * T_max + f0 + f] = v;
      if (fl_out) fl_out[f] = v;
    }
  }
  {
    double s = 0.0, mx = -INFINITY, mn = INFINITY;
    for (int idx = tid; idx < BINS * FT; idx += 256) {
      const int bin = idx >> 6, f = idx & 63;
      if (f < fv) {
        const double v = ms[bin * MLD + f];
        s += v;
        mx = fmax(mx, v);
        mn = fmin(mn, v);
      }
    }
    const double sum = block_tree(s, red, dadd);
    const double mean = sum / (double)(BINS * fv);
    double q = 0.0;
    for (int idx = tid; idx < BINS * FT; idx += 256) {
      const int bin = idx >> 6, f = idx & 63;
      if (f < fv) {
        const double d = (double)ms[bin * MLD + f] - mean;
        q = fma(d, d, q);
      }
    }
    const double m2 = block_tree(q, red, dadd);
    mx = block_tree(mx, red, dmax);
    mn = block_tree(mn, red, [](double x, double y) { return fmin(x, y); });
    if (tid == 0) {
      double* o = partials + ((size_t)b * tiles_max + tile) * PART;
      o[0] = sum;
      o[1] = m2;
      o[2] = mx;
      o[3] = mn;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- path B
// grid (frame tiles, GROUPS2, B): 32 frames x 4 bin blocks; wave w owns bin block 4 blockIdx.y + w
__global__ __launch_bounds__(256) void desc_b_kernel(const float* __restrict__ waves, const int32_t* __restrict__ lengths,
                                                     const float* __restrict__ basis, float* __restrict__ mag_ws, float* __restrict__ magnitude,
                                                     int n_max, int T_max, int tiles_max) {
  __shared__ __attribute__((aligned(16))) float as[A2_FLOATS];
  __shared__ __attribute__((aligned(16))) float bs[256 * BLD2];
  const int tid = threadIdx.x, tile = blockIdx.x, grp = blockIdx.y, b = blockIdx.z;
  const int len = clip_len(lengths, b, n_max);
  const int f0 = tile * FT2;
  const int Tb = frames_b(len);
  const int fv = min(max(Tb - f0, 0), FT2);
  const int fo = min(T_max - f0, FT2);
  const int w = tid >> 6, lane = tid & 63, j31 = lane & 31, h = lane >> 5;
  const int bb = 4 * grp + w;
  const bool live = bb < BIN_BLOCKS2;
  float* mag_out = magnitude ? magnitude + (size_t)b * BINS2 * T_max + f0 : nullptr;

  if (fv == 0) {      // (uniform) the optional output's zero padding; nothing of the workspace is written or read for these frames
    if (mag_out)
      for (int idx = tid; idx < 128 * FT2; idx += 256) {
        const int bin = 128 * grp + (idx >> 5), f = idx & 31;
        if (bin < BINS2 && f < fo) mag_out[(size_t)bin * T_max + f] = 0.0f;
      }
    return;
  }

  // ---- the A operand: padded samples p0 .. p0 + 31 * 512 + 2047 of the clip, zeros outside [0, len)
  {
    const float* x = waves + (size_t)b * n_max;
    const int p0 = f0 * HOP2;
    constexpr int SPAN = (FT2 - 1) * HOP2 + NFFT2, BATCH = 14;      // 70 samples per thread in five batches of independent loads
    for (int s0 = tid; s0 < SPAN; s0 += 256 * BATCH) {
      float v[BATCH];
#pragma unroll
      for (int j = 0; j < BATCH; ++j) {
        const int i = p0 + s0 + 256 * j - PAD2;
        const bool ok = s0 + 256 * j < SPAN && i >= 0 && i < len;
        v[j] = x[ok ? i : 0];
        v[j] = ok ? v[j] : 0.0f;
      }
#pragma unroll
      for (int j = 0; j < BATCH; ++j) {
        const int s = s0 + 256 * j;
        if (s < SPAN) as[s + 4 * (s / HOP2)] = v[j];
      }
    }
  }

  // staging of a slab: 256 columns (per wave: cos of its 32 bins, then -sin) x 32 taps, eight 16-B pieces per thread
  f32x4 pre[8];
  auto fetch = [&](int kc) {
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int q = tid + 256 * m, lc = q / (KC2 / 4), kq = (q % (KC2 / 4)) * 4;
      const int bin = 32 * (4 * grp + (lc >> 6)) + (lc & 31), part = (lc >> 5) & 1;
      const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
      pre[m] = bin < BINS2 ? *reinterpret_cast<const f32x4*>(basis + (size_t)(part * BINS2 + bin) * NFFT2 + kc * KC2 + kq) : zero;
    }
  };
  fetch(0);
  f32x16 re, im;
#pragma unroll
  for (int q = 0; q < 16; ++q) re[q] = im[q] = 0.0f;
  for (int kc = 0; kc < SLABS2; ++kc) {
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int q = tid + 256 * m;
      *reinterpret_cast<f32x4*>(&bs[(q / (KC2 / 4)) * BLD2 + (q % (KC2 / 4)) * 4]) = pre[m];
    }
    __syncthreads();      // (the first one also publishes `as`)
    if (kc + 1 < SLABS2) fetch(kc + 1);
    if (live) {
      // frame j31, taps 32 kc + 8 u + 4 h + e; 512 = 16 KC2, so a slab never straddles a hop
      const float* ap = as + ALD2 * j31 + kc * KC2 + 4 * (kc >> 4) + 4 * h;
      const float* bre = bs + (64 * w + j31) * BLD2 + 4 * h;
      const float* bim = bre + 32 * BLD2;
#pragma unroll
      for (int u = 0; u < KC2 / 8; ++u) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(ap + 8 * u);
        const f32x4 c = *reinterpret_cast<const f32x4*>(bre + 8 * u);
        const f32x4 s = *reinterpret_cast<const f32x4*>(bim + 8 * u);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          re = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], c[e], re, 0, 0, 0);
          im = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], s[e], im, 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
  if (!live) return;
  // accumulator register q of lane (j31, h): frame (q & 3) + 8 (q >> 2) + 4 h, bin 32 bb + j31 (bins 1025 .. 1055: zeros)
  const int bin = 32 * bb + j31;
  float* row = mag_ws + ((size_t)b * tiles_max * FT2 + f0) * MAG_LD + bin;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int f = (q & 3) + 8 * (q >> 2) + 4 * h;
    const float v = sqrtf(fmaf(re[q], re[q], im[q] * im[q]));
    if (f < fv) row[(size_t)f * MAG_LD] = v;
    if (mag_out && bin < BINS2 && f < fo) mag_out[(size_t)bin * T_max + f] = f < fv ? v : 0.0f;
  }
}

// One wave per frame: lane l owns bins 17 l .. 17 l + 16 in ascending order (double); the lanes' sums are combined in lane order.
__global__ __launch_bounds__(256) void desc_b_frame_kernel(const float* __restrict__ mag_ws, const int32_t* __restrict__ lengths,
                                                           float* __restrict__ cent, float* __restrict__ roll, float* __restrict__ flat,
                                                           float* __restrict__ cent_out, float* __restrict__ roll_out, float* __restrict__ flat_out,
                                                           int n_max, int T_max, int tiles_max) {
  __shared__ double part[4][4][64];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, b = blockIdx.y;
  const int t = 4 * blockIdx.x + w;
  const int Tb = frames_b(clip_len(lengths, b, n_max));
  const bool on = t < Tb;
  const int lo = CHUNK2 * lane, hi = min(lo + CHUNK2, BINS2);
  const float* row = mag_ws + ((size_t)b * tiles_max * FT2 + (on ? t : 0)) * MAG_LD;
  double s = 0.0, fs = 0.0, sl = 0.0, sp = 0.0;
  if (on)
    for (int k = lo; k < hi; ++k) {
      const float v = row[k];
      const double p = power_of(v);
      s += (double)v;
      fs = fma((double)k, (double)v, fs);
      sl += log(p);
      sp += p;
    }
  part[w][0][lane] = s;
  part[w][1][lane] = fs;
  part[w][2][lane] = sl;
  part[w][3][lane] = sp;
  __syncthreads();
  if (!on) {
    if (t < T_max && lane == 0) {
      const size_t at = (size_t)b * T_max + t;
      if (cent_out) cent_out[at] = 0.0f;
      if (roll_out) roll_out[at] = 0.0f;
      if (flat_out) flat_out[at] = 0.0f;
    }
    return;
  }
  double tot = 0.0, tfs = 0.0, tsl = 0.0, tsp = 0.0, before = 0.0;
  for (int l = 0; l < 64; ++l) {
    if (l == lane) before = tot;      // the running sum of S over the bins below this lane's
    tot += part[w][0][l];
    tfs += part[w][1][l];
    tsl += part[w][2][l];
    tsp += part[w][3][l];
  }
  // rolloff: the first bin whose running sum is not below 0.85 of the total
  const double thr = 0.85 * tot;
  int first = INT_MAX;
  double cum = before;
  for (int k = lo; k < hi; ++k) {
    cum += (double)row[k];
    if (first == INT_MAX && cum >= thr) first = k;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o));
  if (lane == 0) {
    const size_t at = (size_t)b * T_max + t;
    const float c = tot < (double)FLT_MIN ? 0.0f : (float)(BIN_HZ2 * tfs / tot);
    const float r = (float)(BIN_HZ2 * (double)min(first, BINS2 - 1));
    const float f = flatness_of(tsl, tsp, BINS2);
    cent[at] = c;
    roll[at] = r;
    flat[at] = f;
    if (cent_out) cent_out[at] = c;
    if (roll_out) roll_out[at] = r;
    if (flat_out) flat_out[at] = f;
  }
}

// ---------------------------------------------------------------------------------------------------------------- zero crossings
// grid (T_max, B): frame t is samples 512 t - 1024 .. 512 t + 1023 of the clip, EDGE-padded; |x| <= 1e-10 counts as +0
__device__ __forceinline__ bool neg_of(float v) { return fabsf(v) <= 1e-10f ? false : (__float_as_uint(v) >> 31) != 0; }

__global__ __launch_bounds__(256) void desc_zcr_kernel(const float* __restrict__ waves, const int32_t* __restrict__ lengths, int32_t* __restrict__ zc,
                                                       float* __restrict__ zcr_out, int n_max, int T_max) {
  __shared__ int red[4];
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int len = clip_len(lengths, b, n_max);
  const size_t at = (size_t)b * T_max + t;
  if (t >= frames_b(len)) {      // (uniform)
    if (zcr_out && tid == 0) zcr_out[at] = 0.0f;
    return;
  }
  const float* x = waves + (size_t)b * n_max;
  const int p0 = t * HOP2 - PAD2;
  int n = 0;
  for (int j = 1 + tid; j < NFFT2; j += 256) {
    const int i = min(max(p0 + j, 0), len - 1), ip = min(max(p0 + j - 1, 0), len - 1);
    n += neg_of(x[i]) != neg_of(x[ip]) ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
  if ((tid & 63) == 0) red[tid >> 6] = n;
  __syncthreads();
  if (tid == 0) {
    const int c = (red[0] + red[1]) + (red[2] + red[3]);
    zc[at] = c;
    if (zcr_out) zcr_out[at] = (float)c / (float)NFFT2;
  }
}

// ---------------------------------------------------------------------------------------------------------------- finish
struct FinishArgs {
  const double* partials;
  const float *peak, *valley, *flat_a, *cent, *roll, *flat_b;
  const int32_t* zc;
  float *descriptors, *features, *contrast, *clone;
  int n_max, TA, TB, tiles_a, dim, do_a, do_b;
};

__device__ __forceinline__ double to_db(float v) { return 10.0 * log10(fmax(1e-10, (double)v)); }

// mean over n floats (double, fixed order: thread t takes t, t + 256, ..., then the tree); n >= 1
__device__ __forceinline__ double block_mean(const float* v, int n, double* red) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += (double)v[i];
  return block_tree(s, red, dadd) / (double)n;
}

// One workgroup per clip: the 11 descriptors in the reference's order, the tiled and normalised features, the clone score.
__global__ __launch_bounds__(256) void desc_finish_kernel(const int32_t* __restrict__ lengths, FinishArgs a) {
  __shared__ double red[256];
  __shared__ float d[DESC];
  __shared__ float inv;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int len = clip_len(lengths, b, a.n_max);
  const int Ta = frames_a(len), Tb = frames_b(len);
  if (tid < DESC) d[tid] = 0.0f;
  __syncthreads();
  if (a.do_a && Ta > 0) {
    if (tid == 0) {      // the tiles in order (Chan's pairwise update)
      double n = 0.0, mean = 0.0, m2 = 0.0, mx = 0.0, mn = 0.0;
      for (int t = 0; t * FT < Ta; ++t) {
        const double* p = a.partials + ((size_t)b * a.tiles_a + t) * PART;
        const double nt = (double)(BINS * min(FT, Ta - t * FT));
        const double delta = p[0] / nt - mean, tot = n + nt;
        mean += delta * (nt / tot);
        m2 += p[1] + delta * delta * (n * nt / tot);
        mx = t ? fmax(mx, p[2]) : p[2];
        mn = t ? fmin(mn, p[3]) : p[3];
        n = tot;
      }
      d[0] = (float)mean;
      d[1] = (float)sqrt(m2 / n);
      d[2] = (float)mx;
      d[3] = (float)mn;
    }
    // contrast = power_to_db(peak) - power_to_db(valley), each clipped from below at its own maximum over the clip - 80 dB
    const float* pk = a.peak + (size_t)b * NBAND * a.TA;
    const float* vl = a.valley + (size_t)b * NBAND * a.TA;
    const int n = NBAND * Ta;
    double mp = -INFINITY, mv = -INFINITY;
    for (int i = tid; i < n; i += 256) {
      const size_t at = (size_t)(i / Ta) * a.TA + i % Ta;
      mp = fmax(mp, (double)pk[at]);
      mv = fmax(mv, (double)vl[at]);
    }
    const double floor_p = to_db((float)block_tree(mp, red, dmax)) - 80.0, floor_v = to_db((float)block_tree(mv, red, dmax)) - 80.0;
    double s = 0.0;
    for (int i = tid; i < n; i += 256) {
      const size_t at = (size_t)(i / Ta) * a.TA + i % Ta;
      const double c = fmax(to_db(pk[at]), floor_p) - fmax(to_db(vl[at]), floor_v);
      s += c;
      if (a.contrast) a.contrast[(size_t)b * NBAND * a.TA + at] = (float)c;
    }
    const double cmean = block_tree(s, red, dadd) / (double)n;
    double q = 0.0;
    for (int i = tid; i < n; i += 256) {
      const size_t at = (size_t)(i / Ta) * a.TA + i % Ta;
      const double e = fmax(to_db(pk[at]), floor_p) - fmax(to_db(vl[at]), floor_v) - cmean;
      q = fma(e, e, q);
    }
    const double cvar = block_tree(q, red, dadd) / (double)n;
    const float* fl = a.flat_a + (size_t)b * a.TA;
    const double fmean = block_mean(fl, Ta, red);
    q = 0.0;
    for (int i = tid; i < Ta; i += 256) {
      const double e = (double)fl[i] - fmean;
      q = fma(e, e, q);
    }
    const double fvar = block_tree(q, red, dadd) / (double)Ta;
    if (tid == 0) {
      d[4] = (float)cmean;
      d[5] = (float)sqrt(cvar);
      d[6] = (float)fmean;
      d[7] = (float)sqrt(fvar);
    }
  }
  if (a.contrast)      // zeros from frame T_b on
    for (size_t i = tid; i < (size_t)NBAND * a.TA; i += 256)
      if ((int)(i % a.TA) >= (a.do_a ? Ta : 0)) a.contrast[(size_t)b * NBAND * a.TA + i] = 0.0f;
  float clone = 0.0f;
  if (a.do_b && Tb > 0) {
    const double c = block_mean(a.cent + (size_t)b * a.TB, Tb, red);
    const double r = block_mean(a.roll + (size_t)b * a.TB, Tb, red);
    const double f = block_mean(a.flat_b + (size_t)b * a.TB, Tb, red);
    double s = 0.0;      // (a sum of integers below 2^53: exact)
    for (int i = tid; i < Tb; i += 256) s += (double)a.zc[(size_t)b * a.TB + i];
    const double z = block_tree(s, red, dadd) / ((double)NFFT2 * (double)Tb);
    if (tid == 0) {
      d[8] = (float)c;
      d[9] = (float)r;
      d[10] = (float)z;
    }
    // the reference mixes the three float32 means in Python floats
    const double sc = 0.4 * (double)(float)f + 0.3 * (double)(float)z + 0.3 * tanh((double)(float)c / 3000.0);
    clone = (float)fmin(fmax(sc, 0.0), 1.0);
  }
  __syncthreads();
  if (tid == 0) {
    double ss = 0.0;      // ||tile(d)[:dim]||^2: descriptor k appears (dim - k + 10) / 11 times
    for (int k = 0; k < DESC; ++k) ss += (double)(a.dim > k ? (a.dim - k + DESC - 1) / DESC : 0) * (double)d[k] * (double)d[k];
    inv = (float)sqrt(ss) + 1e-9f;
    if (a.clone) a.clone[b] = clone;
  }
  __syncthreads();
  if (a.descriptors && tid < DESC) a.descriptors[(size_t)b * DESC + tid] = d[tid];
  if (a.features)
    for (int i = tid; i < a.dim; i += 256) a.features[(size_t)b * a.dim + i] = d[i % DESC] / inv;
}

bool shape_ok(int B, int n_max) { return B >= 1 && B <= 65535 && n_max >= 1 && n_max <= (1 << 30); }

}  // namespace

extern "C" size_t ufnd_spectral_desc_workspace_bytes(int B, int n_max) { return shape_ok(B, n_max) ? layout(B, n_max).bytes : 0; }

extern "C" int ufnd_spectral_descriptors(const float* waves, const int32_t* lengths, const float* basis_a, const float* basis_b, void* workspace,
                                         const ufnd_spectral_desc_out* out, int B, int n_max, int dim, void* stream_) {
  UFND_REQUIRE(waves && basis_a && basis_b && workspace && out, "spectral_descriptors: null argument (waves, basis_a, basis_b, workspace, out)");
  const bool all = out->features || out->descriptors;
  const bool want_a = all || out->contrast || out->flatness || out->magnitude;
  const bool want_b = all || out->clone_score || out->centroid || out->rolloff || out->flatness_y || out->magnitude_y;
  const bool want_z = all || out->clone_score || out->zcr;
  UFND_REQUIRE(want_a || want_b || want_z, "spectral_descriptors: no output asked for");
  UFND_REQUIRE(shape_ok(B, n_max), "spectral_descriptors: B=%d n_max=%d (1 <= B <= 65535 clips of 1 <= n_max <= 2^30 samples)", B, n_max);
  UFND_REQUIRE(!out->features || dim >= 1, "spectral_descriptors: dim=%d (>= 1)", dim);
  UFND_REQUIRE(ufnd_aligned(basis_a, 16) && ufnd_aligned(basis_b, 16) && ufnd_aligned(workspace, 16),
               "spectral_descriptors: alignment (basis_a, basis_b, workspace: 16 bytes)");
  hipStream_t stream = (hipStream_t)stream_;
  const Layout l = layout(B, n_max);
  char* ws = (char*)workspace;
  float *peak = (float*)(ws + l.peak), *valley = (float*)(ws + l.valley), *flat_a = (float*)(ws + l.flat_a);
  float *cent = (float*)(ws + l.cent), *roll = (float*)(ws + l.roll), *flat_b = (float*)(ws + l.flat_b), *mag_b = (float*)(ws + l.mag_b);
  int32_t* zc = (int32_t*)(ws + l.zc);
  if (want_a) {
    hipLaunchKernelGGL(desc_a_kernel, dim3(l.tiles_a, B), dim3(256), 0, stream, waves, lengths, basis_a, (double*)(ws + l.partials), peak, valley, flat_a,
                       out->magnitude, out->flatness, n_max, l.TA, l.tiles_a);
    UFND_CHECK_LAUNCH();
  }
  if (want_b) {
    hipLaunchKernelGGL(desc_b_kernel, dim3(l.tiles_b, GROUPS2, B), dim3(256), 0, stream, waves, lengths, basis_b, mag_b, out->magnitude_y, n_max, l.TB,
                       l.tiles_b);
    UFND_CHECK_LAUNCH();
    hipLaunchKernelGGL(desc_b_frame_kernel, dim3(ufnd_cdiv(l.TB, 4), B), dim3(256), 0, stream, mag_b, lengths, cent, roll, flat_b, out->centroid,
                       out->rolloff, out->flatness_y, n_max, l.TB, l.tiles_b);
    UFND_CHECK_LAUNCH();
  }
  if (want_z) {
    hipLaunchKernelGGL(desc_zcr_kernel, dim3(l.TB, B), dim3(256), 0, stream, waves, lengths, zc, out->zcr, n_max, l.TB);
    UFND_CHECK_LAUNCH();
  }
  if (all || out->contrast || out->clone_score) {
    FinishArgs a = {(const double*)(ws + l.partials), peak, valley, flat_a, cent, roll, flat_b, zc, out->descriptors, out->features, out->contrast,
                    out->clone_score, n_max, l.TA, l.TB, l.tiles_a, dim, want_a ? 1 : 0, (want_b && want_z) ? 1 : 0};
    hipLaunchKernelGGL(desc_finish_kernel, dim3(B), dim3(256), 0, stream, lengths, a);
    UFND_CHECK_LAUNCH();
  }
  return UFND_OK;
}
