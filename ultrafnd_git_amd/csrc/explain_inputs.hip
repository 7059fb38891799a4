// Token and image-patch attributions (explain.input_attribution): the row kernels around the encoders' data-gradient pass.
// The reference explains its classifier's input row only (src/models/fusion/deep_truth_classifier.py:189-272); carrying the
// gradient on through the encoders to tokens and pixels has no counterpart there.  All HBM-bound: 16-B accesses, DPP wave
// reductions, block sums added in a fixed order -- no atomics, a rerun gives the same bits.
#include <hip/hip_runtime.h>

#include "rowwise.hpp"

namespace {

__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

struct PathAlphas {
  float a[UFND_PATH_MAX_POINTS];
};

// out[k][w] = base[w] + a_k (x[w] - base[w]) over the panel's 16-byte words w; x and base are read once for all points
__global__ __launch_bounds__(256) void path_points_kernel(const float* __restrict__ x, const float* __restrict__ base, const PathAlphas al, int n,
                                                          size_t words, float* __restrict__ out) {
  for (size_t w = blockIdx.x * (size_t)256 + threadIdx.x; w < words; w += (size_t)gridDim.x * 256) {
    const f32x4 xv = ld4(x + 4 * w);
    const f32x4 bv = base ? ld4(base + 4 * w) : f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4 d = xv - bv;
    for (int k = 0; k < n; ++k) st4(out + 4 * ((size_t)k * words + w), bv + al.a[k] * d);
  }
}

// one wave per row: score[r] = sum_h g (s - base), norm[r] = ||g||_2; rows with mask 0 are written as exactly 0
__global__ __launch_bounds__(256) void token_attribution_kernel(const float* __restrict__ g, int ldg, const float* __restrict__ s, int lds,
                                                                const float* __restrict__ base, int ldb, const int32_t* __restrict__ mask,
                                                                int R, int H, float* __restrict__ score, float* __restrict__ norm) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  if (mask && mask[row] == 0) {      // (wave-uniform)
    if (lane == 0) {
      score[row] = 0.0f;
      norm[row] = 0.0f;
    }
    return;
  }
  float dot = 0.0f, sq = 0.0f;
  for (int c = 4 * lane; c < H; c += 256) {
    const f32x4 gv = ld4(g + (size_t)row * ldg + c);
    const f32x4 d = ld4(s + (size_t)row * lds + c) - ld4(base + (size_t)row * ldb + c);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      dot += gv[q] * d[q];
      sq += gv[q] * gv[q];
    }
  }
  dot = wave_sum(dot);
  sq = wave_sum(sq);
  if (lane == 0) {
    score[row] = dot;
    norm[row] = sqrtf(sq);
  }
}

// One workgroup per patch: the patch's 3 p^2 gradients (conv-weight order (c, ky, kx): a row of ufnd_vit_patchify's panel) go
// back to their pixels.  grad / pix (N, 3, S, S), psum (N, P): any subset.  pix = g (x - base); psum = the patch's sum of pix:
// per-thread strided sums, a DPP wave sum, the four waves added in wave order.
__global__ __launch_bounds__(256) void unpatchify_kernel(const float* __restrict__ dp, const float* __restrict__ x, const float* __restrict__ base,
                                                         float* __restrict__ grad, float* __restrict__ pix, float* __restrict__ psum, int S, int P) {
  __shared__ float sh[4];
  const int G = S / P, K = 3 * P * P;
  const int patch = blockIdx.x, n = patch / (G * G), rem = patch - n * G * G, py = rem / G, px = rem - py * G;
  const float* src = dp + (size_t)patch * K;
  const size_t img = (size_t)n * 3 * S * S;
  float acc = 0.0f;
  for (int e = 4 * threadIdx.x; e < K; e += 1024) {
    const int c = e / (P * P), r = e - c * P * P, ky = r / P, kx = r - ky * P;
    const size_t at = img + ((size_t)c * S + (size_t)py * P + ky) * S + (size_t)px * P + kx;
    const f32x4 gv = ld4(src + e);
    if (grad) st4(grad + at, gv);
    if (x) {
      f32x4 d = ld4(x + at);
      if (base) d -= ld4(base + at);
      const f32x4 a = gv * d;
      if (pix) st4(pix + at, a);
      acc += (a[0] + a[1]) + (a[2] + a[3]);
    }
  }
  if (psum) {
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) psum[patch] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
  }
}

}  // namespace

extern "C" int ufnd_path_points(const float* x, const float* base, const float* alphas, int n_points, size_t rows, int width, float* out,
                                void* stream_) {
  UFND_REQUIRE(x && alphas && out && rows >= 1, "path_points: null argument");
  UFND_REQUIRE(n_points >= 1 && n_points <= UFND_PATH_MAX_POINTS, "path_points: %d points (1 .. %d per call)", n_points, UFND_PATH_MAX_POINTS);
  UFND_REQUIRE(width >= 4 && width % 4 == 0, "path_points: width=%d (a multiple of 4)", width);
  UFND_REQUIRE(ufnd_aligned(x, 16) && (!base || ufnd_aligned(base, 16)) && ufnd_aligned(out, 16), "path_points: 16-B alignment");
  PathAlphas al;
  for (int k = 0; k < UFND_PATH_MAX_POINTS; ++k) al.a[k] = k < n_points ? alphas[k] : 0.0f;
  const size_t words = rows * (size_t)width / 4, want = (words + 255) / 256;
  hipLaunchKernelGGL(path_points_kernel, dim3((unsigned)(want > 8192 ? 8192 : want)), dim3(256), 0, (hipStream_t)stream_, x, base, al, n_points, words,
                     out);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_token_attribution(const float* g, int ldg, const float* s, int lds, const float* base, int ldb, const int32_t* mask, int R, int H,
                                      float* score, float* grad_norm, void* stream_) {
  UFND_REQUIRE(g && s && base && score && grad_norm && R >= 1, "token_attribution: null argument");
  UFND_REQUIRE(H >= 4 && H % 4 == 0 && ldg % 4 == 0 && ldg >= H && lds % 4 == 0 && lds >= H && ldb % 4 == 0 && ldb >= H,
               "token_attribution: H=%d ldg=%d lds=%d ldb=%d (multiples of 4, strides >= H)", H, ldg, lds, ldb);
  UFND_REQUIRE(ufnd_aligned(g, 16) && ufnd_aligned(s, 16) && ufnd_aligned(base, 16), "token_attribution: 16-B alignment");
  hipLaunchKernelGGL(token_attribution_kernel, dim3(ufnd_cdiv(R, 4)), dim3(256), 0, (hipStream_t)stream_, g, ldg, s, lds, base, ldb, mask, R, H, score,
                     grad_norm);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_vit_unpatchify_attribution(const float* dpatches, const float* x, const float* base, float* grad, float* pixels, float* patch_sums,
                                               int N, int image, int patch, void* stream_) {
  UFND_REQUIRE(dpatches && (grad || pixels || patch_sums) && N >= 1, "vit_unpatchify_attribution: null argument");
  UFND_REQUIRE(x || (!pixels && !patch_sums && !base), "vit_unpatchify_attribution: pixels / patch_sums / base need x");
  UFND_REQUIRE(patch >= 4 && patch % 4 == 0 && image >= patch && image % patch == 0, "vit_unpatchify_attribution: image=%d patch=%d (patch a multiple of 4)",
               image, patch);
  UFND_REQUIRE(ufnd_aligned(dpatches, 16) && (!x || ufnd_aligned(x, 16)) && (!base || ufnd_aligned(base, 16)) && (!grad || ufnd_aligned(grad, 16)) &&
                   (!pixels || ufnd_aligned(pixels, 16)), "vit_unpatchify_attribution: 16-B alignment");
  const long long blocks = (long long)N * (image / patch) * (image / patch);
  UFND_REQUIRE(blocks < (1ll << 31), "vit_unpatchify_attribution: N=%d", N);
  hipLaunchKernelGGL(unpatchify_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream_, dpatches, x, base, grad, pixels, patch_sums, image, patch);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}
