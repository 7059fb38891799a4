// The reference's MelSpectrogramGenerator.generate on a host WITH librosa (src/core_blocks/audio_blocks.py:71-78), batched on the device:
//   S_db = power_to_db(melspectrogram(y, sr=16000, n_fft=400, hop_length=160, n_mels=64, power=2.0), ref=np.max)      (64, T) per clip
// The definitions are restated from librosa's documented algorithms (0.10 defaults; include/ultrafnd_hip.h spells them out) and are
// NOT verified against librosa itself.  Two launches:
//   mel_tile_kernel   grid (frame tiles of 64, B): the zero-padded path-A STFT tile (csrc/stft_tile_a.hpp: the magnitudes of
//                     spectral_descriptors, bit for bit), then the filterbank from the LDS tile: wave w owns filters w, w + 4, ...,
//                     lane f owns frame f, so the tile is read at stride 1 and the filter's support and weights are wave-uniform.
//                     M[i, t] is ONE chain of fmaf from zero over the filter's support in ascending bins; nothing outside the support
//                     is touched.  The tile's mel powers and their maximum (one float per tile) go to the workspace.
//   mel_db_kernel     grid (frame tiles, B): folds the clip's tile maxima (a maximum is order-free; still no atomics), converts its
//                     own tile in double, writes the zero padding, the tiles past the clip's last frame and mel_max.
// A clip is computed as if alone and nothing at or past x[len] is read.
#include <math.h>

#include "stft_tile_a.hpp"

namespace {

namespace T = stft_tile_a;
constexpr int FT = UFND_MEL_FRAME_TILE, MELS = UFND_MEL_FILTERS, NNZ = UFND_MEL_NNZ;
static_assert(FT == T::FT && FT == 64 && MELS == 64, "a lane per frame of the tile, a wave per four filters");

__device__ __forceinline__ int clip_len(const int32_t* lengths, int b, int n_max) {
  const int n = lengths ? lengths[b] : n_max;
  return n < 0 ? 0 : (n > n_max ? n_max : n);
}

// the workspace: offsets in bytes
struct Layout {
  size_t power, tile_max, bytes;
  int T_max, tiles;
};
__host__ inline Layout layout(int B, int n_max) {
  Layout l;
  l.T_max = 1 + n_max / T::HOP;
  l.tiles = ufnd_cdiv(l.T_max, FT);
  size_t o = 0;
  auto take = [&](size_t n) {
    const size_t at = o;
    o += (n + 15) / 16 * 16;
    return at;
  };
  l.power = take((size_t)B * MELS * l.T_max * sizeof(float));
  l.tile_max = take((size_t)B * l.tiles * sizeof(float));
  l.bytes = o;
  return l;
}

__global__ __launch_bounds__(256) void mel_tile_kernel(const float* __restrict__ waves, const int32_t* __restrict__ lengths,
                                                       const float* __restrict__ basis, const float* __restrict__ fb_weights,
                                                       const int32_t* __restrict__ fb_first, const int32_t* __restrict__ fb_count,
                                                       float* __restrict__ power, float* __restrict__ tile_max, int n_max, int T_max, int tiles_max) {
  __shared__ __attribute__((aligned(16))) float as[T::A_FLOATS];
  __shared__ __attribute__((aligned(16))) float bs[T::B_FLOATS];
  __shared__ float ms[T::M_FLOATS];
  __shared__ float wl[NNZ];
  __shared__ int lo_s[MELS], cnt_s[MELS], off_s[MELS];
  __shared__ float wmax[4];
  const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
  const int len = clip_len(lengths, b, n_max);
  const int f0 = tile * FT;
  const int fv = min(max(T::frames(len) - f0, 0), FT);      // the clip's frames in this tile
  if (fv == 0) return;      // (uniform) nothing of the clip here: mel_db_kernel writes these columns and reads nothing of this tile

  // the filter table: the supports are clamped to the tile's bins and to the NNZ packed weights, whatever the arrays hold
  if (tid < MELS) {
    const int lo = min(max(fb_first[tid], 0), T::BINS);
    lo_s[tid] = lo;
    cnt_s[tid] = min(max(fb_count[tid], 0), T::BINS - lo);
  }
  for (int i = tid; i < NNZ; i += 256) wl[i] = fb_weights[i];
  __syncthreads();
  if (tid == 0) {
    int at = 0;
    for (int i = 0; i < MELS; ++i) {
      const int c = min(cnt_s[i], NNZ - at);
      off_s[i] = at;
      cnt_s[i] = c;
      at += c;
    }
  }
  T::magnitudes(waves + (size_t)b * n_max, len, f0, basis, as, bs, ms);      // (its barriers publish the table too)

  // ---- the filterbank: 64 filters x 64 frames, a lane per frame
  const int w = tid >> 6, f = tid & 63;
  float best = 0.0f;      // powers are >= 0
  float* out = power + (size_t)b * MELS * T_max + f0 + f;
  for (int i = w; i < MELS; i += 4) {
    const int lo = lo_s[i], cnt = cnt_s[i];
    const float* wt = wl + off_s[i];
    const float* col = ms + lo * T::MLD + f;
    float m = 0.0f;
    for (int k = 0; k < cnt; ++k) {
      const float s = col[k * T::MLD];
      m = fmaf(wt[k], s * s, m);      // P = S S is one fp32 product of its own
    }
    if (f < fv) {
      out[(size_t)i * T_max] = m;
      best = fmaxf(best, m);
    }
  }
  best = wave_max(best);
  if (f == 0) wmax[w] = best;
  __syncthreads();
  if (tid == 0) tile_max[(size_t)b * tiles_max + tile] = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
}

__device__ __forceinline__ double db_of(float v) { return 10.0 * log10(fmax(1e-10, (double)v)); }

__global__ __launch_bounds__(256) void mel_db_kernel(const int32_t* __restrict__ lengths, const float* __restrict__ power,
                                                     const float* __restrict__ tile_max, float* __restrict__ mel_db, float* __restrict__ mel_power,
                                                     float* __restrict__ mel_max, int n_max, int T_max, int tiles_max) {
  __shared__ float red[256];
  const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y;
  const int Tb = T::frames(clip_len(lengths, b, n_max));
  const int f0 = tile * FT;
  const int fv = min(max(Tb - f0, 0), FT);
  const int fo = min(T_max - f0, FT);      // output columns of this tile (zeros from fv on)
  // the clip's maximum: the maxima of its (Tb + 63) / 64 tiles
  float mx = 0.0f;
  if (fv > 0 || (tile == 0 && mel_max)) {      // (uniform)
    const int nt = (Tb + FT - 1) / FT;
    for (int t = tid; t < nt; t += 256) mx = fmaxf(mx, tile_max[(size_t)b * tiles_max + t]);
    red[tid] = mx;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) red[tid] = fmaxf(red[tid], red[tid + o]);
      __syncthreads();
    }
    mx = red[0];
  }
  if (tile == 0 && tid == 0 && mel_max) mel_max[b] = mx;
  const double ref = db_of(mx);
  for (int idx = tid; idx < MELS * FT; idx += 256) {
    const int i = idx >> 6, f = idx & 63;
    if (f >= fo) continue;
    const size_t at = ((size_t)b * MELS + i) * T_max + f0 + f;
    const bool on = f < fv;
    const float m = on ? power[at] : 0.0f;
    if (mel_power) mel_power[at] = m;
    if (mel_db) mel_db[at] = on ? (float)fmax(db_of(m) - ref, -80.0) : 0.0f;
  }
}

bool shape_ok(int B, int n_max) { return B >= 1 && B <= 65535 && n_max >= 1 && n_max <= (1 << 30); }

}  // namespace

extern "C" size_t ufnd_mel_workspace_bytes(int B, int n_max) { return shape_ok(B, n_max) ? layout(B, n_max).bytes : 0; }

extern "C" int ufnd_mel_spectrogram(const float* waves, const int32_t* lengths, const float* basis_a, const float* fb_weights, const int32_t* fb_first,
                                    const int32_t* fb_count, void* workspace, float* mel_db, float* mel_power, float* mel_max, int B, int n_max,
                                    void* stream_) {
  UFND_REQUIRE(waves && basis_a && fb_weights && fb_first && fb_count && workspace,
               "mel_spectrogram: null argument (waves, basis_a, fb_weights, fb_first, fb_count, workspace)");
  UFND_REQUIRE(mel_db || mel_power || mel_max, "mel_spectrogram: no output asked for (mel_db, mel_power, mel_max)");
  UFND_REQUIRE(shape_ok(B, n_max), "mel_spectrogram: B=%d n_max=%d (1 <= B <= 65535 clips of 1 <= n_max <= 2^30 samples)", B, n_max);
  UFND_REQUIRE(ufnd_aligned(basis_a, 16) && ufnd_aligned(workspace, 16) && ufnd_aligned(fb_weights, 4) && ufnd_aligned(fb_first, 4) &&
                   ufnd_aligned(fb_count, 4),
               "mel_spectrogram: alignment (basis_a, workspace: 16 bytes; fb_weights, fb_first, fb_count: 4 bytes)");
  hipStream_t stream = (hipStream_t)stream_;
  const Layout l = layout(B, n_max);
  float* power = (float*)((char*)workspace + l.power);
  float* tile_max = (float*)((char*)workspace + l.tile_max);
  hipLaunchKernelGGL(mel_tile_kernel, dim3(l.tiles, B), dim3(256), 0, stream, waves, lengths, basis_a, fb_weights, fb_first, fb_count, power, tile_max,
                     n_max, l.T_max, l.tiles);
  UFND_CHECK_LAUNCH();
  hipLaunchKernelGGL(mel_db_kernel, dim3(l.tiles, B), dim3(256), 0, stream, lengths, power, tile_max, mel_db, mel_power, mel_max, n_max, l.T_max, l.tiles);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}
