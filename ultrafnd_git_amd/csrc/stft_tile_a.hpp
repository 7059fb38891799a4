// The zero-padded STFT tile of path A (n_fft 400, hop 160, 201 bins; periodic Hann window folded into the basis): 64 frames of ONE
// clip as a 64-frame x 201-bin magnitude tile in LDS.  The arithmetic is that of desc_a_kernel (csrc/spectral_desc.hip), value for
// value: re and im of a (frame, bin) are each ONE chain of 400 fmaf from zero in the tap order 8u + e, 8u + 4 + e, and
// |S| = sqrtf(fmaf(re, re, im * im)), so a magnitude has the same bits in both kernels (tests/test_gpu_mel.py holds them to it).
// csrc/mel_db.hip is the user; csrc/spectral_desc.hip keeps its own copy of this body (DESIGN.md says why).
#pragma once
#include "common.hpp"

namespace stft_tile_a {

constexpr int NFFT = 400, HOP = 160, BINS = 201, PAD = 200;
constexpr int FT = 64;                                  // frames of a tile
constexpr int BIN_BLOCKS = 7, ROUNDS = 4, KC = 40, SLABS = NFFT / KC, BLD = KC + 4, ALD = HOP + 4;
constexpr int A_FLOATS = ALD * (FT - 1) + NFFT + 8 + 4;      // the tile's samples: frame i starts at 164 i
constexpr int B_FLOATS = 128 * BLD;                          // one slab of the basis: 128 columns x 40 taps
constexpr int MLD = FT + 1;
constexpr int M_FLOATS = BINS * MLD;                         // the magnitudes: bin k, frame f at k MLD + f
static_assert(HOP % KC == 0 && NFFT % KC == 0 && KC % 8 == 0 && (128 * KC / 4) % 256 == 0, "tile geometry");

__host__ __device__ inline int frames(int len) { return len >= 1 ? 1 + len / HOP : 0; }

// 256 threads, all of them.  x: the clip's samples (len >= 1 of them; nothing at or past x[len] is read); f0: the tile's first
// frame; basis: (402, 400), 16-byte aligned; as, bs (16-byte aligned), ms: LDS of A_FLOATS, B_FLOATS, M_FLOATS floats.  On return
// ms holds the magnitudes of frames f0 .. f0 + 63 (zeros for frames past the clip's last: their samples are all padding) and the
// workgroup is synchronised.
__device__ __forceinline__ void magnitudes(const float* __restrict__ x, int len, int f0, const float* __restrict__ basis, float* as, float* bs,
                                           float* ms) {
  const int tid = threadIdx.x;
  // ---- the A operand: padded samples p0 .. p0 + 63 * 160 + 399 of the clip, zeros outside [0, len)
  {
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
}

}  // namespace stft_tile_a
