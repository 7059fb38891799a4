// RobertaForSequenceClassification (the emotion classifier of src/models/affective_forensics.py) and AffectiveForensics: the pieces
// that are not a GEMM, an attention or a LayerNorm launch.
//   pack     position ids by HF's rule (create_position_ids_from_input_ids: cumsum(ids != pad) * (ids != pad) + pad, over the ids, not
//            the mask), a per-sample "has a kept token" flag and, on request, ufnd_text_pack's cu_seqlens / row_src
//   embed    LayerNorm(word[id] + position[pos_id] + token_type[0]) -> bf16 and/or fp32 rows (bert_embed with looked-up positions)
//   gather   the class (<s>) row of each sample -> compact B-row buffers: what the last layer runs over past its attention
//   head     tanh(x Wd^T + bd) -> out_proj -> softmax -> fear / anger / joy group sums -> intensity and valence, all fp32
//   arousal  clip(sigmoid(5 mean(x^2))) per clip, the reference's RMS-energy branch
// A wave or a workgroup per sample, fixed reduction trees, no atomics: a sample's results are the same bits alone and inside any batch.
#include "rowwise.hpp"
#include "gemm_f32.hpp"

namespace {

// ---- pack: one workgroup, a wave per sample.  64 tokens per step: an inclusive wave scan of (id != pad) on top of the running count.
__global__ __launch_bounds__(PACK_THREADS) void roberta_pack_kernel(const int64_t* ids, const int32_t* mask, int B, int L, long long pad, int32_t* cu,
                                                                    int32_t* row_src, int32_t* pos_ids, int32_t* valid) {
  __shared__ int lens[PACK_MAX_B];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int b = wave; b < B; b += PACK_THREADS / 64) {
    int last = 0, carry = 0;
    for (int l0 = 0; l0 < L; l0 += 64) {      // (wave-uniform trip count: every lane takes part in the shuffles)
      const int l = l0 + lane;
      int f = 0;
      if (l < L) {
        f = ids[(size_t)b * L + l] != pad ? 1 : 0;
        last = mask[(size_t)b * L + l] != 0 ? l + 1 : last;
      }
      int inc = f;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(inc, o, 64);
        if (lane >= o) inc += y;
      }
      if (l < L) pos_ids[(size_t)b * L + l] = (carry + inc) * f + (int)pad;
      carry += __shfl(inc, 63, 64);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) last = max(last, __shfl_xor(last, o, 64));
    if (lane == 0) {
      lens[b] = last;      // ufnd_text_pack's n_b: the largest kept position + 1
      if (valid) valid[b] = last > 0 ? 1 : 0;
    }
  }
  if (cu) pack_scan_rows(lens, B, L, cu, row_src);      // (rowwise.hpp: the scan ufnd_text_pack runs)
}

// ---- embed: one wave per row of H = 256 NI columns
template <int NI>
__global__ __launch_bounds__(256) void roberta_embed_kernel(const int64_t* ids, const int32_t* pos_ids, const float* word, const float* pos, const float* type0,
                                                            const float* gamma, const float* beta, __bf16* ob, float* of, int M, int H, int vocab,
                                                            int max_pos, float eps, const int32_t* row_src, const int* m_live) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M || (m_live && row >= *m_live)) return;
  int src = row_src ? row_src[row] : row;      // packed rows: the (B, L) index of the token
  src = src < 0 ? 0 : (src >= M ? M - 1 : src);
  long long id = ids[src];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);      // never read outside the tables
  int p = pos_ids[src];
  p = p < 0 ? 0 : (p >= max_pos ? max_pos - 1 : p);
  f32x4 v[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int col = 4 * lane + 256 * i;
    v[i] = ld4(word + (size_t)id * H + col) + ld4(pos + (size_t)p * H + col) + ld4(type0 + col);
  }
  ln_row<NI>(v, H, eps, gamma, beta, lane);
  store_row<NI>(v, ob, of, row, H, lane);
}

// ---- gather: one wave per sample.  Row cu[b] of the packed stream (b L of the padded one); a sample without rows gets zeros.
__global__ __launch_bounds__(256) void gather_class_rows_kernel(const int32_t* cu, const __bf16* ctx_s, __bf16* ctx_d, const __bf16* rb_s, __bf16* rb_d,
                                                                const float* rf_s, float* rf_d, const float* st_s, float* st_d, int B, int L, int H,
                                                                int st_floats, int capacity) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  long long row = cu ? (long long)cu[b] : (long long)b * L;
  const bool live = (!cu || cu[b + 1] > cu[b]) && row >= 0 && row < capacity;
  if (!live) row = 0;
  for (int col = 4 * lane; col < H; col += 256) {
    const bf16x4 zb = {(__bf16)0.0f, (__bf16)0.0f, (__bf16)0.0f, (__bf16)0.0f};
    if (ctx_s) *reinterpret_cast<bf16x4*>(ctx_d + (size_t)b * H + col) = live ? *reinterpret_cast<const bf16x4*>(ctx_s + (size_t)row * H + col) : zb;
    if (rb_s) *reinterpret_cast<bf16x4*>(rb_d + (size_t)b * H + col) = live ? *reinterpret_cast<const bf16x4*>(rb_s + (size_t)row * H + col) : zb;
    if (rf_s) *reinterpret_cast<f32x4*>(rf_d + (size_t)b * H + col) = live ? ld4(rf_s + (size_t)row * H + col) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }
  if (st_s)
    for (int k = lane; k < st_floats; k += 64) st_d[(size_t)b * st_floats + k] = live ? st_s[(size_t)row * st_floats + k] : 0.0f;
}

// ---- head epilogue: one workgroup per sample.  z (B, H): the dense Linear's pre-activations.  A label's group entry: -1 none, 0 fear,
// 1 anger, 2 joy, 4 + m for several groups at once (m: bit 0 fear, bit 1 anger, bit 2 joy).
constexpr int HEAD_MAX_H = 1024, HEAD_MAX_C = 32;
__device__ __forceinline__ float clip01(float x) { return fminf(1.0f, fmaxf(0.0f, x)); }

__global__ __launch_bounds__(256) void emotion_head_kernel(const float* z, const float* bd, const float* wo, const float* bo, const int32_t* group,
                                                           const int32_t* valid, const float* arousal, float* logits, float* class_probs, float* probs,
                                                           float* text_intensity, float* intensity, float* valence, int H, int C) {
  __shared__ float t[HEAD_MAX_H];
  __shared__ float lg[HEAD_MAX_C];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const bool ok = !valid || valid[b] != 0;      // a sample without a kept token: its features count as zero, the dense output is its bias
  for (int c = tid; c < H; c += 256) t[c] = tanhf(ok ? z[(size_t)b * H + c] : bd[c]);
  __syncthreads();
  for (int c = wave; c < C; c += 4) {      // a wave per label: lane-strided products in column order, then the wave tree
    float acc = 0.0f;
    for (int k = lane; k < H; k += 64) acc = fmaf(t[k], wo[(size_t)c * H + k], acc);
    acc = wave_sum(acc);
    if (lane == 0) lg[c] = acc + bo[c];
  }
  __syncthreads();
  if (tid != 0) return;
  float mx = lg[0];
  for (int c = 1; c < C; ++c) mx = fmaxf(mx, lg[c]);
  float s = 0.0f;
  for (int c = 0; c < C; ++c) {      // (one thread, label order: C <= 32)
    logits[(size_t)b * C + c] = lg[c];
    lg[c] = expf(lg[c] - mx);
    s += lg[c];
  }
  float g3[3] = {0.0f, 0.0f, 0.0f};
  for (int c = 0; c < C; ++c) {
    const float p = lg[c] / s;
    class_probs[(size_t)b * C + c] = p;
    if (group) {
      const int g = group[c];
      const int m = g < 0 ? 0 : (g < 3 ? 1 << g : (g - 4) & 7);
      if (m & 1) g3[0] += p;
      if (m & 2) g3[1] += p;
      if (m & 4) g3[2] += p;
    }
  }
  if (!probs) return;
  const float tot = g3[0] + g3[1] + g3[2] + 1e-9f;
  const float f = ok ? g3[0] / tot : 0.0f, a = ok ? g3[1] / tot : 0.0f, j = ok ? g3[2] / tot : 0.0f;
  probs[(size_t)b * 3 + 0] = f;
  probs[(size_t)b * 3 + 1] = a;
  probs[(size_t)b * 3 + 2] = j;
  const float raw = f + a - 0.5f * j;
  const float ti = clip01(1.0f / (1.0f + expf(-2.5f * raw)));
  const float ar = arousal ? arousal[b] : 0.5f;
  text_intensity[b] = ti;
  intensity[b] = clip01(0.6f * ti + 0.4f * ar);
  valence[b] = clip01(0.5f + 0.5f * (j - 0.5f * (f + a)));
}

// ---- arousal: one workgroup per clip.  Thread t adds the squares of samples t, t + 256, ... in order; then block_sum4's fixed tree.
__global__ __launch_bounds__(256) void audio_arousal_kernel(const float* x, const int32_t* lengths, float* out, int T) {
  __shared__ float red[4];
  const int b = blockIdx.x;
  int n = lengths ? lengths[b] : T;
  n = n < 0 ? 0 : (n > T ? T : n);
  const float tot = block_square_sum(x + (size_t)b * T, n, red);
  if (threadIdx.x == 0) {
    const float en = n > 0 ? tot / (float)n : 0.0f;
    out[b] = clip01(1.0f / (1.0f + expf(-5.0f * en)));
  }
}

int embed_checks(const char* what, const int64_t* ids, const int32_t* pos_ids, const float* word, const float* pos, const float* type0, const float* gamma,
                 const float* beta, void* x_bf16, float* x_f32, int rows, int L, int H, int vocab, int max_pos, int pad) {
  UFND_REQUIRE(ids && pos_ids && word && pos && type0 && gamma && beta && (x_bf16 || x_f32), "%s: null argument", what);
  UFND_REQUIRE(h_ok(H) && rows >= 1 && L >= 1 && vocab >= 1 && pad >= 0 && max_pos >= 1, "%s: rows=%d L=%d H=%d vocab=%d max_position=%d pad=%d", what, rows,
               L, H, vocab, max_pos, pad);
  UFND_REQUIRE(L <= max_pos - pad - 1, "%s: L=%d exceeds max_position - pad_token_id - 1 = %d (position ids run to L + pad)", what, L, max_pos - pad - 1);
  UFND_REQUIRE(ufnd_aligned(word, 16) && ufnd_aligned(pos, 16) && ufnd_aligned(type0, 16) && ufnd_aligned(gamma, 16) && ufnd_aligned(beta, 16) &&
                   (!x_f32 || ufnd_aligned(x_f32, 16)) && (!x_bf16 || ufnd_aligned(x_bf16, 8)), "%s: alignment", what);
  return UFND_OK;
}

}  // namespace

extern "C" int ufnd_roberta_pack(const int64_t* ids, const int32_t* mask, int B, int L, int pad_token_id, int32_t* cu_seqlens, int32_t* row_src,
                                 int32_t* pos_ids, int32_t* valid, void* stream_) {
  UFND_REQUIRE(ids && mask && pos_ids && !cu_seqlens == !row_src, "roberta_pack: null argument");
  UFND_REQUIRE(B >= 1 && B <= PACK_MAX_B && L >= 1 && pad_token_id >= 0 && (long long)B * L < (1ll << 31) && (long long)L + pad_token_id < (1ll << 31),
               "roberta_pack: B=%d L=%d pad=%d (B <= %d)", B, L, pad_token_id, PACK_MAX_B);
  hipLaunchKernelGGL(roberta_pack_kernel, dim3(1), dim3(PACK_THREADS), 0, (hipStream_t)stream_, ids, mask, B, L, (long long)pad_token_id, cu_seqlens, row_src,
                     pos_ids, valid);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_roberta_embed(const int64_t* ids, const int32_t* pos_ids, const float* word, const float* pos, const float* type0, const float* gamma,
                                  const float* beta, void* x_bf16, float* x_f32, int B, int L, int H, int vocab, int max_position, int pad_token_id,
                                  float eps, void* stream_) {
  UFND_REQUIRE(B >= 1 && L >= 1 && (long long)B * L < (1ll << 31), "roberta_embed: B=%d L=%d", B, L);
  const int rc = embed_checks("roberta_embed", ids, pos_ids, word, pos, type0, gamma, beta, x_bf16, x_f32, B * L, L, H, vocab, max_position, pad_token_id);
  if (rc != UFND_OK) return rc;
  NI_LAUNCH(H, roberta_embed_kernel, dim3(ufnd_cdiv(B * L, 4)), (hipStream_t)stream_, ids, pos_ids, word, pos, type0, gamma, beta, (__bf16*)x_bf16, x_f32,
            B * L, H, vocab, max_position, eps, (const int32_t*)nullptr, (const int*)nullptr);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_roberta_embed_live(const int64_t* ids, const int32_t* pos_ids, const int32_t* row_src, const int* m_live, const float* word,
                                       const float* pos, const float* type0, const float* gamma, const float* beta, void* x_bf16, float* x_f32,
                                       int capacity, int L, int H, int vocab, int max_position, int pad_token_id, float eps, void* stream_) {
  UFND_REQUIRE(row_src && m_live, "roberta_embed_live: null argument");
  const int rc = embed_checks("roberta_embed_live", ids, pos_ids, word, pos, type0, gamma, beta, x_bf16, x_f32, capacity, L, H, vocab, max_position,
                              pad_token_id);
  if (rc != UFND_OK) return rc;
  NI_LAUNCH(H, roberta_embed_kernel, dim3(ufnd_cdiv(capacity, 4)), (hipStream_t)stream_, ids, pos_ids, word, pos, type0, gamma, beta, (__bf16*)x_bf16, x_f32,
            capacity, H, vocab, max_position, eps, row_src, m_live);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_gather_class_rows(const int32_t* cu_seqlens, const void* ctx, void* ctx_out, const void* res_bf16, void* res_bf16_out,
                                      const float* res_f32, float* res_f32_out, const float* stats, float* stats_out, int B, int L, int H, int stat_floats,
                                      int capacity, void* stream_) {
  UFND_REQUIRE(!ctx == !ctx_out && !res_bf16 == !res_bf16_out && !res_f32 == !res_f32_out && !stats == !stats_out && (ctx || res_bf16 || res_f32 || stats),
               "gather_class_rows: null argument (a source and its destination go together, at least one pair)");
  UFND_REQUIRE(B >= 1 && L >= 1 && H >= 4 && H % 4 == 0 && (long long)B * L < (1ll << 31) && capacity >= 1 && (cu_seqlens || (long long)B * L <= capacity) &&
                   (!stats || stat_floats >= 1), "gather_class_rows: B=%d L=%d H=%d stat_floats=%d capacity=%d (H a multiple of 4)", B, L, H, stat_floats,
               capacity);
  UFND_REQUIRE(ufnd_aligned(ctx, 8) && ufnd_aligned(ctx_out, 8) && ufnd_aligned(res_bf16, 8) && ufnd_aligned(res_bf16_out, 8) && ufnd_aligned(res_f32, 16) &&
                   ufnd_aligned(res_f32_out, 16), "gather_class_rows: alignment");
  hipLaunchKernelGGL(gather_class_rows_kernel, dim3(ufnd_cdiv(B, 4)), dim3(256), 0, (hipStream_t)stream_, cu_seqlens, (const __bf16*)ctx, (__bf16*)ctx_out,
                     (const __bf16*)res_bf16, (__bf16*)res_bf16_out, res_f32, res_f32_out, stats, stats_out, B, L, H, stat_floats, capacity);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_emotion_head(const float* x, const float* wd, const float* bd, const float* wo, const float* bo, const int32_t* group,
                                 const int32_t* text_valid, const float* arousal, float* workspace, float* logits, float* class_probs, float* probs,
                                 float* text_intensity, float* intensity, float* valence, int B, int H, int C, void* stream_) {
  UFND_REQUIRE(x && wd && bd && wo && bo && workspace && logits && class_probs, "emotion_head: null argument");
  UFND_REQUIRE((probs && text_intensity && intensity && valence && group) || (!probs && !text_intensity && !intensity && !valence),
               "emotion_head: probs, text_intensity, intensity and valence go together, with the group table");
  UFND_REQUIRE(B >= 1 && B <= 65535 && H >= 32 && H % 32 == 0 && H <= HEAD_MAX_H && C >= 1 && C <= HEAD_MAX_C,
               "emotion_head: B=%d H=%d C=%d (B <= 65535, H a multiple of 32 up to %d, C <= %d)", B, H, C, HEAD_MAX_H, HEAD_MAX_C);
  const NtProb p = nt_linear(x, H, wd, H, bd, workspace, H, B, H, H);
  const int rc = launch_nt(&p, 1, nullptr, (hipStream_t)stream_);      // (the exact-fp32 skinny GEMM: ufnd_linear_f32's kernels)
  if (rc != UFND_OK) return rc;
  hipLaunchKernelGGL(emotion_head_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream_, (const float*)workspace, bd, wo, bo, group, text_valid, arousal,
                     logits, class_probs, probs, text_intensity, intensity, valence, H, C);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_audio_arousal(const float* waves, const int32_t* lengths, float* arousal, int B, int T, void* stream_) {
  UFND_REQUIRE(waves && arousal, "audio_arousal: null argument");
  UFND_REQUIRE(B >= 1 && B <= 65535 && T >= 1, "audio_arousal: B=%d T=%d (1 <= B <= 65535 clips of T >= 1 samples; lengths may be 0)", B, T);
  hipLaunchKernelGGL(audio_arousal_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream_, waves, lengths, arousal, T);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}
