// What the frame-reading kernels share (csrc/motion.hip, csrc/forgery.hip): the clamped clip length, the reference's float64 luma, wave-wide
// integer and double sums, and the tile-and-normalise finish of every evidence vector.  Both files are compiled with -ffp-contract=off
// (build.py), which the luma and the norm rely on.
#pragma once
#include "common.hpp"

namespace {

__device__ __forceinline__ int clip_len(const int32_t* lengths, int b, int T) {
  const int n = lengths ? lengths[b] : T;
  return n < 0 ? 0 : (n > T ? T : n);
}

// wave-wide integer sum by DPP, the association order of wave_sum (common.hpp); integer adds are order-independent anyway
#define FRAMES_DPP_I(v, ctrl, rmask) __builtin_amdgcn_update_dpp(0, (v), ctrl, rmask, 0xF, false)
__device__ __forceinline__ int wave_sum_i(int v) {
  v += FRAMES_DPP_I(v, 0xB1, 0xF);
  v += FRAMES_DPP_I(v, 0x4E, 0xF);
  v += FRAMES_DPP_I(v, 0x141, 0xF);
  v += FRAMES_DPP_I(v, 0x140, 0xF);
  v += FRAMES_DPP_I(v, 0x142, 0xA);
  v += FRAMES_DPP_I(v, 0x143, 0xC);
  return __builtin_amdgcn_readlane(v, 63);
}
#undef FRAMES_DPP_I
// wave-wide double sum: the xor butterfly, every lane ends with the same bits
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// (0.2989 r + 0.587 g + 0.114 b) in double, each operation rounded on its own, truncated.  A fused multiply-add changes 224 of the 2^24
// triples.  HIP's __dmul_rn / __dadd_rn are plain operators compiled with the header's contraction setting and were fused here; plain
// operators under the pragma are not (and build.py compiles this file with -ffp-contract=off).
__device__ __forceinline__ uint32_t luma_u8(uint32_t r, uint32_t g, uint32_t b) {
#pragma clang fp contract(off)
  const double pr = 0.2989 * (double)r;
  const double pg = 0.587 * (double)g;
  const double pb = 0.114 * (double)b;
  const double rg = pr + pg;
  const double y = rg + pb;
  return (uint32_t)(int)y;
}

// tile v (nv values, in LDS) to `dim` entries and divide by fl32(||.||) + 1e-9 (fp32, as np.linalg.norm(v) + 1e-9 is under NumPy 2)
__device__ __forceinline__ void tile_normalise(const float* v, int nv, float* out, int dim, float* nrm_slot) {
  if (threadIdx.x == 0) {
    double q = 0.0;
    for (int k = 0; k < nv && k < dim; ++k) q += (double)((dim - k + nv - 1) / nv) * ((double)v[k] * (double)v[k]);      // entry k occurs ceil((dim - k) / nv) times
    *nrm_slot = (float)sqrt(q) + 1e-9f;
  }
  __syncthreads();
  const float nrm = *nrm_slot;
  for (int j = threadIdx.x; j < dim; j += blockDim.x) out[j] = __fdiv_rn(v[j % nv], nrm);
}

}  // namespace
