// The reference's audio feature layer on the branches it takes without librosa and without a wav2vec2 checkpoint
// (src/core_blocks/audio_blocks.py), SURVEY.md section 2 row 11:
//   SpectralForensics._torch_stft_fallback  :178-188  torch.stft(n_fft=400, hop=160).abs() -> [mean, std, max, min] tiled, L2-normalised
//   MelSpectrogramGenerator.generate        :79-91    the same magnitudes, bins 3m .. 3m + 2 averaged into 64 bands
//   VoiceCloneDetector.score                :255-257  e = mean(x^2), e / (e + 1)
// The STFT is an exact-fp32 GEMM on v_mfma_f32_32x32x2_f32: row t of the A operand is samples 160 t .. 160 t + 399 of the
// reflect-padded clip (overlapping rows of the wave itself, mirrored by index while staging: no padded copy, no frame matrix), the B
// operand is the (402, 400) cos / -sin basis streamed through LDS in K-slabs.  A workgroup owns 64 frames of ONE clip, counted from
// the clip's own first frame, and all 201 bins: the magnitudes of its tile meet in LDS, and the statistics, the 64 bands and the
// optional spectrogram are read from there, so the statistics never need the spectrogram in memory.
//
// One value, one arithmetic: re and im of (frame, bin) are each ONE chain of 400 fmaf from zero, in the tap order
// 8u + e, 8u + 4 + e  (u = 0 .. 49, e = 0 .. 3) -- the two lane halves of an MFMA step feed taps 4 apart -- whatever the tile, the
// batch or the outputs asked for; |S| = sqrtf(fmaf(re, re, im * im)).  No atomics; the tile statistics are fixed trees in double and
// the finish kernel combines a clip's tiles in tile order (Chan).  A clip's outputs are the same bits alone and in any batch.
#include "rowwise.hpp"

namespace {

constexpr int NFFT = 400, HOP = 160, BINS = 201, REFLECT = 200, MIN_LEN = 201, BANDS = 64;
constexpr int FT = UFND_STFT_FRAME_TILE;      // frames of a workgroup: two 32-row MFMA blocks
constexpr int BIN_BLOCKS = 7;                 // 32-bin blocks (224 columns; the basis of bins 201 .. 223 is zero)
constexpr int ROUNDS = 4;                     // per round two bin blocks are live: waves 0, 1 take block 2 r, waves 2, 3 block 2 r + 1
constexpr int KC = 40;                        // taps of a K-slab: 160 = 4 KC, so a slab never straddles a hop
constexpr int SLABS = NFFT / KC;
constexpr int BLD = KC + 4;                   // slab row stride (floats): 11 x 16 B, odd -> 16-B reads of 32 rows spread over all banks
constexpr int ALD = HOP + 4;                  // a hop of samples takes 164 floats in LDS (41 x 16 B, odd): frame i starts at 164 i
constexpr int A_FLOATS = ALD * (FT - 1) + NFFT + 8 + 4;
constexpr int MLD = FT + 1;                   // magnitude tile [bin][frame]
constexpr int PART = 4;                       // doubles per tile partial: sum, centred second moment, max, min
static_assert(FT == 64 && HOP % KC == 0 && NFFT % KC == 0 && KC % 8 == 0 && (128 * KC / 4) % 256 == 0, "tile geometry");

__host__ __device__ inline int frames_of(int len) { return len >= MIN_LEN ? 1 + len / HOP : 0; }
__device__ __forceinline__ int clip_len(const int32_t* lengths, int b, int n_max) {
  const int n = lengths ? lengths[b] : n_max;
  return n < 0 ? 0 : (n > n_max ? n_max : n);
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

__global__ __launch_bounds__(256) void stft_kernel(const float* __restrict__ waves, const int32_t* __restrict__ lengths,
                                                   const float* __restrict__ basis, double* __restrict__ partials,
                                                   float* __restrict__ magnitude, float* __restrict__ mel, int n_max, int T_max, int tiles_max) {
  __shared__ __attribute__((aligned(16))) float as[A_FLOATS];
  __shared__ __attribute__((aligned(16))) float bs[128 * BLD];
  __shared__ float ms[BINS * MLD];
  __shared__ double red[256];
  const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
  const int len = clip_len(lengths, b, n_max);
  const int f0 = tile * FT;
  const int Tb = frames_of(len);
  const int fv = min(max(Tb - f0, 0), FT);      // the clip's frames in this tile
  const int fo = min(T_max - f0, FT);           // output columns of this tile (zeros from fv on)
  float* mag_out = magnitude ? magnitude + (size_t)b * BINS * T_max + f0 : nullptr;
  float* mel_out = mel ? mel + (size_t)b * BANDS * T_max + f0 : nullptr;

  if (fv == 0) {      // (uniform) nothing of the clip here: the outputs' zero padding, no partial (the finish kernel counts tiles from T_b)
    for (int idx = tid; idx < BINS * FT; idx += 256) {
      const int row = idx >> 6, f = idx & 63;
      if (f < fo) {
        if (mag_out) mag_out[(size_t)row * T_max + f] = 0.0f;
        if (mel_out && row < BANDS) mel_out[(size_t)row * T_max + f] = 0.0f;
      }
    }
    return;
  }

  // ---- the A operand: padded samples p0 .. p0 + 63 * 160 + 399 of the clip, mirrored by index; nothing at or past x[len] is read
  {
    const float* x = waves + (size_t)b * n_max;
    const int p0 = f0 * HOP;
    constexpr int SPAN = (FT - 1) * HOP + NFFT, BATCH = 21;      // 41 samples per thread in two batches of independent loads
    for (int s0 = tid; s0 < SPAN; s0 += 256 * BATCH) {
      float v[BATCH];
#pragma unroll
      for (int j = 0; j < BATCH; ++j) {      // branch-free: a sample no frame of the clip reaches loads x[0] and stores zero
        const int p = p0 + s0 + 256 * j;
        const bool ok = s0 + 256 * j < SPAN && p < len + 2 * REFLECT;
        int i = p - REFLECT;
        i = i < 0 ? -i : (i >= len ? 2 * (len - 1) - i : i);      // (len >= 201: both mirrors land inside the clip)
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
  if (mel_out) {
    for (int idx = tid; idx < BANDS * FT; idx += 256) {
      const int m = idx >> 6, f = idx & 63;
      if (f < fo) {
        const float* c = ms + 3 * m * MLD + f;
        mel_out[(size_t)m * T_max + f] = f < fv ? ((c[0] + c[MLD]) + c[2 * MLD]) / 3.0f : 0.0f;
      }
    }
  }
  if (partials) {
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
    auto add = [](double x, double y) { return x + y; };
    const double sum = block_tree(s, red, add);
    const double mean = sum / (double)(BINS * fv);
    double q = 0.0;
    for (int idx = tid; idx < BINS * FT; idx += 256) {
      const int bin = idx >> 6, f = idx & 63;
      if (f < fv) {
        const double d = (double)ms[bin * MLD + f] - mean;
        q = fma(d, d, q);
      }
    }
    const double m2 = block_tree(q, red, add);
    mx = block_tree(mx, red, [](double x, double y) { return fmax(x, y); });
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

// One workgroup per clip: thread 0 walks the clip's tiles in order (Chan's pairwise update, double); then stats and the tiled,
// normalised features.
__global__ __launch_bounds__(256) void stft_finish_kernel(const double* __restrict__ partials, const int32_t* __restrict__ lengths,
                                                          float* __restrict__ stats, float* __restrict__ features, int n_max, int tiles_max,
                                                          int dim) {
  __shared__ float st[4];
  __shared__ float inv;
  const int b = blockIdx.x;
  if (threadIdx.x == 0) {
    const int Tb = frames_of(clip_len(lengths, b, n_max));
    double n = 0.0, mean = 0.0, m2 = 0.0, mx = 0.0, mn = 0.0;
    for (int t = 0; t * FT < Tb; ++t) {
      const double* p = partials + ((size_t)b * tiles_max + t) * PART;
      const double nt = (double)(BINS * min(FT, Tb - t * FT));
      const double delta = p[0] / nt - mean, tot = n + nt;
      mean += delta * (nt / tot);
      m2 += p[1] + delta * delta * (n * nt / tot);
      mx = t ? fmax(mx, p[2]) : p[2];
      mn = t ? fmin(mn, p[3]) : p[3];
      n = tot;
    }
    st[0] = (float)mean;
    st[1] = n > 0.0 ? (float)sqrt(m2 / n) : 0.0f;
    st[2] = (float)mx;
    st[3] = (float)mn;
    double ss = 0.0;      // ||tile(stats)[:dim]||^2: statistic k appears (dim - k + 3) / 4 times
    for (int k = 0; k < 4; ++k) ss += (double)((dim - k + 3) / 4) * (double)st[k] * (double)st[k];
    inv = (float)sqrt(ss) + 1e-9f;
  }
  __syncthreads();
  if (stats && threadIdx.x < 4) stats[(size_t)b * 4 + threadIdx.x] = st[threadIdx.x];
  if (features)
    for (int i = threadIdx.x; i < dim; i += 256) features[(size_t)b * dim + i] = st[i & 3] / inv;
}

__global__ __launch_bounds__(256) void wave_energy_kernel(const float* __restrict__ x, const int32_t* __restrict__ lengths,
                                                          float* __restrict__ energy, float* __restrict__ score, int n_max) {
  __shared__ float red[4];
  const int b = blockIdx.x;
  const int n = clip_len(lengths, b, n_max);
  const float tot = block_square_sum(x + (size_t)b * n_max, n, red);
  if (threadIdx.x == 0) {
    const float e = n > 0 ? tot / (float)n : 0.0f;
    if (energy) energy[b] = e;
    if (score) {      // the reference divides in Python floats: e / (e + 1.0) in double, then clips
      const double r = (double)e / ((double)e + 1.0);
      score[b] = (float)fmin(fmax(r, 0.0), 1.0);
    }
  }
}

int shape_checks(const char* what, int B, int n_max) {
  UFND_REQUIRE(B >= 1 && B <= 65535 && n_max >= 1 && n_max <= (1 << 30), "%s: B=%d n_max=%d (1 <= B <= 65535 clips of 1 <= n_max <= 2^30 samples)", what, B,
               n_max);
  return UFND_OK;
}

}  // namespace

extern "C" size_t ufnd_spectral_workspace_bytes(int B, int n_max) {
  if (B < 1 || B > 65535 || n_max < 1 || n_max > (1 << 30)) return 0;
  return (size_t)B * ufnd_cdiv(1 + n_max / HOP, FT) * PART * sizeof(double);
}

extern "C" int ufnd_stft_forensics(const float* waves, const int32_t* lengths, const float* basis, void* workspace, float* magnitude, float* mel_like,
                                   float* stats, float* features, int B, int n_max, int dim, void* stream_) {
  UFND_REQUIRE(waves && basis, "stft_forensics: null argument (waves, basis)");
  UFND_REQUIRE(magnitude || mel_like || stats || features, "stft_forensics: no output asked for");
  const int rc = shape_checks("stft_forensics", B, n_max);
  if (rc != UFND_OK) return rc;
  const bool want_stats = stats || features;
  UFND_REQUIRE(!want_stats || workspace, "stft_forensics: stats and features need the workspace");
  UFND_REQUIRE(!features || dim >= 1, "stft_forensics: dim=%d (>= 1)", dim);
  UFND_REQUIRE(ufnd_aligned(basis, 16) && ufnd_aligned(workspace, 8), "stft_forensics: alignment (basis 16 bytes, workspace 8)");
  hipStream_t stream = (hipStream_t)stream_;
  const int T_max = 1 + n_max / HOP, tiles_max = ufnd_cdiv(T_max, FT);
  hipLaunchKernelGGL(stft_kernel, dim3(tiles_max, B), dim3(256), 0, stream, waves, lengths, basis, want_stats ? (double*)workspace : nullptr, magnitude,
                     mel_like, n_max, T_max, tiles_max);
  UFND_CHECK_LAUNCH();
  if (want_stats) {
    hipLaunchKernelGGL(stft_finish_kernel, dim3(B), dim3(256), 0, stream, (const double*)workspace, lengths, stats, features, n_max, tiles_max, dim);
    UFND_CHECK_LAUNCH();
  }
  return UFND_OK;
}

extern "C" int ufnd_wave_energy(const float* waves, const int32_t* lengths, float* energy, float* score, int B, int n_max, void* stream_) {
  UFND_REQUIRE(waves && (energy || score), "wave_energy: null argument");
  const int rc = shape_checks("wave_energy", B, n_max);
  if (rc != UFND_OK) return rc;
  hipLaunchKernelGGL(wave_energy_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream_, waves, lengths, energy, score, n_max);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}
