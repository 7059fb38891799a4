// Audio encoder (wav2vec2-base geometry), the pieces that are not a GEMM, an attention or a LayerNorm launch:
//   utterance normalisation, conv layer 0 + GroupNorm + GELU, the positional conv's pack / add kernels, the frame counts.
// Frames are rows, channel-last, in per-clip slabs (include/ultrafnd_hip.h).  Every reduction is a fixed tree over the clip's own
// samples / frames: fp32 partials per fixed-size chunk about the chunk's own fp32 mean (formed inside the workgroup first: a chunk
// whose first value is a click is as accurate as any other), combined in chunk order in float64 (Chan's update).  No atomics; a
// clip's results are the same bits alone and inside any batch, on every run.
#include "rowwise.hpp"
#include "gemm_f32.hpp"

// (the statistics below are sums of exactly the values the apply passes recompute: no contraction may differ between the passes)
#pragma clang fp contract(off)

namespace {

constexpr int WCH = UFND_WAVE_CHUNK;       // samples per wave partial
constexpr int FCH = UFND_CONV0_CHUNK;      // frames per conv0 partial
constexpr int C0 = 512;                    // conv channels
constexpr int HID = 768, POS_G = 16, POS_C = 48, POS_K = 128;

__device__ __forceinline__ int w2v2_frames(int n) {
  int t = (n - 10) / 5 + 1;                 // k 10, s 5
#pragma unroll
  for (int l = 0; l < 4; ++l) t = (t - 3) / 2 + 1;      // k 3, s 2
#pragma unroll
  for (int l = 0; l < 2; ++l) t = (t - 2) / 2 + 1;      // k 2, s 2
  return t;
}

// a clip's sample count, never past the row it lives in (the host checks the range; this keeps a bad count inside the buffer)
__device__ __forceinline__ int clip_len(const int32_t* lengths, int b, int n_max) {
  const int n = lengths[b];
  return n < n_max ? n : n_max;
}

// ---- utterance normalisation.  Partials: grid (chunks, B); chunk c of clip b -> ws[(b nch + c) 3 ..] = {centre, s, q}
__global__ __launch_bounds__(256) void wave_partials_kernel(const float* wave, const int32_t* lengths, float* ws, int n_max, int nch) {
  __shared__ float red[4];
  const int b = blockIdx.y, c = blockIdx.x, n = clip_len(lengths, b, n_max), i0 = c * WCH;
  if (i0 >= n) return;
  const float* x = wave + (size_t)b * n_max;
  const int i1 = i0 + WCH < n ? i0 + WCH : n;
  // the thread's 16 samples stay in registers (past the chunk's end: its first sample, whose difference from itself is 0)
  static_assert(WCH == 16 * 256, "one workgroup of 256 threads holds a chunk in 16 registers per thread");
  const float first = x[i0];
  float v[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int i = i0 + threadIdx.x + 256 * j;
    v[j] = i < i1 ? x[i] : first;
  }
  // pass 1: the chunk's own fp32 mean, from a sum about its first sample.  It only has to lie NEAR the mean: whatever it is, the
  // {centre, s, q} below describe the chunk exactly up to the rounding of s and q
  float s = 0.0f, q = 0.0f;
#pragma unroll
  for (int j = 0; j < 16; ++j) s += v[j] - first;
  const float p = first + block_sum4(s, red) / (float)(i1 - i0);
  // pass 2: the sums about that centre
  s = 0.0f;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if (i0 + threadIdx.x + 256 * j < i1) {
      const float d = v[j] - p;
      s += d;
      q += d * d;
    }
  }
  s = block_sum4(s, red);
  q = block_sum4(q, red);
  if (threadIdx.x == 0) {
    float* o = ws + ((size_t)b * nch + c) * 3;
    o[0] = p; o[1] = s; o[2] = q;
  }
}

// Chan's combination of chunk partials {centre, s, q} with counts cnt(c), in chunk order, float64: mean and M2 of the whole
struct MeanM2 { double mean, m2; };
template <typename Get, typename Cnt>
__device__ __forceinline__ MeanM2 combine_chunks(int nchunks, Get get, Cnt cnt) {
  double n_a = 0.0, mean_a = 0.0, m2_a = 0.0;
  for (int c = 0; c < nchunks; ++c) {
    float p, s, q;
    get(c, p, s, q);
    const double n_b = (double)cnt(c);
    const double mean_b = (double)p + (double)s / n_b;
    double m2_b = (double)q - (double)s * (double)s / n_b;
    m2_b = m2_b > 0.0 ? m2_b : 0.0;
    const double n_ab = n_a + n_b, delta = mean_b - mean_a;
    mean_a += delta * (n_b / n_ab);
    m2_a += m2_b + delta * delta * (n_a * n_b / n_ab);
    n_a = n_ab;
  }
  return MeanM2{mean_a, m2_a};
}

__global__ __launch_bounds__(256) void wave_apply_kernel(const float* wave, const int32_t* lengths, const float* ws, float* out, int n_max, int nch) {
  const int b = blockIdx.y, n = clip_len(lengths, b, n_max), i0 = blockIdx.x * WCH;
  if (i0 >= n) return;
  const float* part = ws + (size_t)b * nch * 3;
  const int used = (n + WCH - 1) / WCH;
  const MeanM2 st = combine_chunks(used, [&](int c, float& p, float& s, float& q) { p = part[3 * c]; s = part[3 * c + 1]; q = part[3 * c + 2]; },
                                   [&](int c) { return n - c * WCH < WCH ? n - c * WCH : WCH; });
  const float mean = (float)st.mean;
  const float inv = (float)(1.0 / sqrt(st.m2 / (double)n + 1e-7));
  const float* x = wave + (size_t)b * n_max;
  float* o = out + (size_t)b * n_max;
  for (int i = i0 + threadIdx.x; i < i0 + WCH && i < n; i += 256) o[i] = (x[i] - mean) * inv;
}

// ---- conv layer 0.  Thread (fq = tid >> 6, cg = tid & 63) owns channels 8 cg .. 8 cg + 7 and the frames t = fq (mod 4) of its block.
__device__ __forceinline__ void conv0_load_w(const float* w, int cg, float (&wr)[8][10]) {
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int k = 0; k < 10; ++k) wr[j][k] = w[(8 * cg + j) * 10 + k];
}
// the 10-tap dot of a window: one fixed fma chain per channel, the same in both passes
__device__ __forceinline__ void conv0_dot(const float (&xv)[10], const float (&wr)[8][10], float (&y)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float a = 0.0f;
#pragma unroll
    for (int k = 0; k < 10; ++k) a = __fmaf_rn(wr[j][k], xv[k], a);
    y[j] = a;
  }
}
__device__ __forceinline__ void conv0_frame(const float* x, int t, const float (&wr)[8][10], float (&y)[8]) {
  float xv[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) xv[k] = x[5 * t + k];
  conv0_dot(xv, wr, y);
}

// partials: grid (frame chunks, B); ws[((b nch + c) 3 + {0,1,2}) 512 + channel] = {centre, s, q} of the chunk's frames
__global__ __launch_bounds__(256) void conv0_partials_kernel(const float* wave, const int32_t* lengths, const float* w, float* ws, int n_max, int nch) {
  __shared__ float red[2][4][C0];
  const int b = blockIdx.y, c = blockIdx.x, T1 = (clip_len(lengths, b, n_max) - 10) / 5 + 1, t0 = c * FCH;
  if (t0 >= T1) return;
  const int fq = threadIdx.x >> 6, cg = threadIdx.x & 63;
  const float* x = wave + (size_t)b * n_max;
  float wr[8][10], piv[8], y[8], s[8], q[8];
  conv0_load_w(w, cg, wr);
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = q[j] = 0.0f;
  const int t1 = t0 + FCH < T1 ? t0 + FCH : T1;
  // the centre of a channel's sums: the conv is linear, so its mean over the chunk's frames is the conv of the MEAN WINDOW -- ten
  // sample means over the chunk (thread i holds frame t0 + i; one fixed tree), the same for all 512 channels.  A centre only has
  // to lie near the mean: whatever it is, {centre, s, q} describe the chunk exactly up to the rounding of s and q.
  static_assert(FCH == 256, "one frame of the chunk per thread");
  {
    float xm[10];
    const int tf = t0 + threadIdx.x;
#pragma unroll
    for (int k = 0; k < 10; ++k) xm[k] = wave_sum(tf < t1 ? x[5 * tf + k] : 0.0f);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int k = 0; k < 10; ++k) red[0][fq][k] = xm[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 10; ++k) xm[k] = ((red[0][0][k] + red[0][1][k]) + (red[0][2][k] + red[0][3][k])) / (float)(t1 - t0);
    __syncthreads();
    conv0_dot(xm, wr, piv);
  }
  // pass 2: the sums about that centre
  for (int t = t0 + fq; t < t1; t += 4) {
    conv0_frame(x, t, wr, y);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float d = y[j] - piv[j];
      s[j] += d;
      q[j] += d * d;
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    red[0][fq][8 * cg + j] = s[j];
    red[1][fq][8 * cg + j] = q[j];
  }
  __syncthreads();
  float* o = ws + ((size_t)b * nch + c) * 3 * C0;
  for (int ch = threadIdx.x; ch < C0; ch += 256) {
    o[2 * C0 + ch] = (red[1][0][ch] + red[1][1][ch]) + (red[1][2][ch] + red[1][3][ch]);
    o[C0 + ch] = (red[0][0][ch] + red[0][1][ch]) + (red[0][2][ch] + red[0][3][ch]);
  }
  if (fq == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) o[8 * cg + j] = piv[j];
  }
}

// statistics: grid (B), 512 threads; stats[(b 512 + ch) 2 ..] = {mean, rstd}
__global__ __launch_bounds__(512) void conv0_stats_kernel(const int32_t* lengths, const float* ws, float* stats, int n_max, int nch, float eps) {
  const int b = blockIdx.x, ch = threadIdx.x, T1 = (clip_len(lengths, b, n_max) - 10) / 5 + 1;
  const float* part = ws + (size_t)b * nch * 3 * C0;
  const int used = (T1 + FCH - 1) / FCH;
  const MeanM2 st = combine_chunks(used, [&](int c, float& p, float& s, float& q) {
                                     const float* o = part + (size_t)c * 3 * C0;
                                     p = o[ch]; s = o[C0 + ch]; q = o[2 * C0 + ch];
                                   },
                                   [&](int c) { return T1 - c * FCH < FCH ? T1 - c * FCH : FCH; });
  stats[((size_t)b * C0 + ch) * 2] = (float)st.mean;
  stats[((size_t)b * C0 + ch) * 2 + 1] = (float)(1.0 / sqrt(st.m2 / (double)T1 + (double)eps));
}

// apply: grid (frame blocks of 64, B): recompute the conv, normalise, GELU, 16-B bf16 stores
__global__ __launch_bounds__(256) void conv0_apply_kernel(const float* wave, const int32_t* lengths, const float* w, const float* gamma, const float* beta,
                                                          const float* stats, __bf16* ob, float* of, int n_max, int S1) {
  const int b = blockIdx.y, T1 = (clip_len(lengths, b, n_max) - 10) / 5 + 1, t0 = blockIdx.x * 64;
  if (t0 >= T1) return;
  const int fq = threadIdx.x >> 6, cg = threadIdx.x & 63;
  const float* x = wave + (size_t)b * n_max;
  float wr[8][10], mean[8], sc[8], bt[8], y[8];
  conv0_load_w(w, cg, wr);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int ch = 8 * cg + j;
    mean[j] = stats[((size_t)b * C0 + ch) * 2];
    sc[j] = stats[((size_t)b * C0 + ch) * 2 + 1];
    bt[j] = beta[ch];
  }
  const int t1 = t0 + 64 < T1 ? t0 + 64 : T1;
  for (int t = t0 + fq; t < t1; t += 4) {
    conv0_frame(x, t, wr, y);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = gelu_fast_f(__fmaf_rn(__fmul_rn(__fsub_rn(y[j], mean[j]), sc[j]), gamma[8 * cg + j], bt[j]));
    const size_t row = (size_t)b * S1 + t;
    bf16x8 o = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3], (__bf16)v[4], (__bf16)v[5], (__bf16)v[6], (__bf16)v[7]};
    *reinterpret_cast<bf16x8*>(ob + row * C0 + 8 * cg) = o;
    if (of) {
      *reinterpret_cast<f32x4*>(of + row * C0 + 8 * cg) = f32x4{v[0], v[1], v[2], v[3]};
      *reinterpret_cast<f32x4*>(of + row * C0 + 8 * cg + 4) = f32x4{v[4], v[5], v[6], v[7]};
    }
  }
}

// ---- positional conv: pack / add.  One thread per 16 bytes.
__global__ __launch_bounds__(256) void pos_pack_kernel(const __bf16* x, const int32_t* frames, __bf16* packed, int B, int S, int Sp, size_t Mp) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x, total = Mp * (HID / 8);
  if (idx >= total) return;
  const int piece = (int)(idx % (HID / 8));
  const size_t prow = idx / (HID / 8);                 // b Sp + tp; the POS_K spare rows behind the last clip (b == B) are zeroed too
  const int b = (int)(prow / Sp), t = (int)(prow % Sp) - POS_K / 2;
  const int g = piece / (POS_C / 8), j = piece % (POS_C / 8);
  bf16x8 v = {};
  if (b < B && t >= 0 && t < S && t < frames[b]) v = *reinterpret_cast<const bf16x8*>(x + ((size_t)b * S + t) * HID + 8 * piece);
  *reinterpret_cast<bf16x8*>(packed + ((size_t)g * Mp + prow) * POS_C + 8 * j) = v;
}

__global__ __launch_bounds__(256) void pos_add_kernel(const float* x, const float* conv, const int32_t* frames, float* y, int B, int S, int Sp) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)B * S * (HID / 4);
  if (idx >= total) return;
  const int piece = (int)(idx % (HID / 4));
  const size_t row = idx / (HID / 4);
  const int b = (int)(row / S), t = (int)(row % S);
  const int g = piece / (POS_C / 4), o4 = piece % (POS_C / 4);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (t < frames[b]) {
    const f32x4 xv = *reinterpret_cast<const f32x4*>(x + row * HID + 4 * piece);
    const f32x4 cv = *reinterpret_cast<const f32x4*>(conv + ((size_t)g * B * Sp + (size_t)b * Sp + t) * 64 + 4 * o4);
    v = xv + cv;
  }
  *reinterpret_cast<f32x4*>(y + row * HID + 4 * piece) = v;
}

__global__ __launch_bounds__(256) void frames_kernel(const int32_t* lengths, int32_t* frames, int32_t* key_mask, int B, int S) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= B * S) return;
  const int b = idx / S, t = idx % S, T = w2v2_frames(lengths[b]);
  key_mask[idx] = t < T ? 1 : 0;
  if (t == 0) frames[b] = T;
}

}  // namespace

extern "C" int ufnd_wave_normalize(const float* wave, const int32_t* lengths, float* out, float* ws, int B, int n_max, void* stream_) {
  UFND_REQUIRE(wave && lengths && out && ws, "wave_normalize: null argument");
  UFND_REQUIRE(B >= 1 && B <= 65535 && n_max >= UFND_AUDIO_MIN_SAMPLES && (long long)B * n_max < (1ll << 40),
               "wave_normalize: B=%d n_max=%d (a clip has at least %d samples: one output frame)", B, n_max, UFND_AUDIO_MIN_SAMPLES);
  const int nch = ufnd_cdiv(n_max, WCH);
  hipLaunchKernelGGL(wave_partials_kernel, dim3(nch, B), dim3(256), 0, (hipStream_t)stream_, wave, lengths, ws, n_max, nch);
  hipLaunchKernelGGL(wave_apply_kernel, dim3(nch, B), dim3(256), 0, (hipStream_t)stream_, wave, lengths, (const float*)ws, out, n_max, nch);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_w2v2_conv0(const float* wave, const int32_t* lengths, const float* w, const float* gamma, const float* beta, void* out_bf16,
                               float* out_f32, float* ws, int B, int n_max, int S1, float eps, void* stream_) {
  UFND_REQUIRE(wave && lengths && w && gamma && beta && out_bf16 && ws, "w2v2_conv0: null argument");
  UFND_REQUIRE(B >= 1 && B <= 65535 && n_max >= UFND_AUDIO_MIN_SAMPLES, "w2v2_conv0: B=%d n_max=%d (a clip has at least %d samples)", B, n_max,
               UFND_AUDIO_MIN_SAMPLES);
  UFND_REQUIRE(S1 % 64 == 0 && S1 >= (n_max - 10) / 5 + 1, "w2v2_conv0: S1=%d (a multiple of 64, at least the %d frames of n_max=%d samples)", S1,
               (n_max - 10) / 5 + 1, n_max);
  UFND_REQUIRE(ufnd_aligned(out_bf16, 16) && (!out_f32 || ufnd_aligned(out_f32, 16)), "w2v2_conv0: 16-B alignment required");
  const int nch = ufnd_cdiv(S1, FCH);
  float* stats = ws + (size_t)3 * B * C0 * nch;
  hipStream_t st = (hipStream_t)stream_;
  hipLaunchKernelGGL(conv0_partials_kernel, dim3(nch, B), dim3(256), 0, st, wave, lengths, w, ws, n_max, nch);
  hipLaunchKernelGGL(conv0_stats_kernel, dim3(B), dim3(512), 0, st, lengths, (const float*)ws, stats, n_max, nch, eps);
  hipLaunchKernelGGL(conv0_apply_kernel, dim3(S1 / 64, B), dim3(256), 0, st, wave, lengths, w, gamma, beta, (const float*)stats, (__bf16*)out_bf16,
                     out_f32, n_max, S1);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_w2v2_pos_pack(const void* x_bf16, const int32_t* frames, void* packed, int B, int S, void* stream_) {
  UFND_REQUIRE(x_bf16 && frames && packed, "w2v2_pos_pack: null argument");
  UFND_REQUIRE(B >= 1 && S >= 1 && (long long)B * (S + POS_K) < (1ll << 24), "w2v2_pos_pack: B=%d S=%d", B, S);
  UFND_REQUIRE(ufnd_aligned(x_bf16, 16) && ufnd_aligned(packed, 16), "w2v2_pos_pack: 16-B alignment required");
  const int Sp = S + POS_K;
  const size_t Mp = (size_t)B * Sp + POS_K, total = Mp * (HID / 8);
  hipLaunchKernelGGL(pos_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, (const __bf16*)x_bf16, frames,
                     (__bf16*)packed, B, S, Sp, Mp);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_w2v2_pos_add(const float* x, const float* conv, const int32_t* frames, float* y, int B, int S, void* stream_) {
  UFND_REQUIRE(x && conv && frames && y, "w2v2_pos_add: null argument");
  UFND_REQUIRE(B >= 1 && S >= 1 && (long long)B * (S + POS_K) < (1ll << 24), "w2v2_pos_add: B=%d S=%d", B, S);
  UFND_REQUIRE(ufnd_aligned(x, 16) && ufnd_aligned(conv, 16) && ufnd_aligned(y, 16), "w2v2_pos_add: 16-B alignment required");
  const size_t total = (size_t)B * S * (HID / 4);
  hipLaunchKernelGGL(pos_add_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, x, conv, frames, y, B, S, S + POS_K);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_w2v2_frames(const int32_t* lengths, int32_t* frames, int32_t* key_mask, int B, int S, void* stream_) {
  UFND_REQUIRE(lengths && frames && key_mask, "w2v2_frames: null argument");
  UFND_REQUIRE(B >= 1 && S >= 1 && (long long)B * S < (1ll << 30), "w2v2_frames: B=%d S=%d", B, S);
  hipLaunchKernelGGL(frames_kernel, dim3(ufnd_cdiv(B * S, 256)), dim3(256), 0, (hipStream_t)stream_, lengths, frames, key_mask, B, S);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_linear_f32(const float* X, const float* W, const float* bias, float* Y, int M, int N, int K, void* stream_) {
  UFND_REQUIRE(X && W && Y && M >= 1 && N >= 32 && K >= 4 && K % 4 == 0, "linear_f32: M=%d N=%d K=%d", M, N, K);
  const NtProb p = nt_linear(X, K, W, K, bias, Y, N, M, N, K);
  return launch_nt(&p, 1, nullptr, (hipStream_t)stream_);
}
