// CLIP text tower (CLIPTextModelWithProjection, ViT-B/32 geometry) and the text-image semantic analyzer: the pieces that are not a
// GEMM, an attention or a LayerNorm launch.
//   pack     the pooled position e(b) by HF's rule, and the packed pass's cu_seqlens / row_src over rows 0 .. e(b) of each sample:
//            under the causal mask no row past e(b) can reach row e(b), so the tower needs nothing else
//   embed    token row + position row -> the fp32 residual stream and its bf16 rounding (no LayerNorm, no token types)
//   pool     final_layer_norm on row e(b) alone -> bf16, the A operand of the text_projection GEMM
//   head     exact-erf GELU of the two projections and l2n(t), l2n(i), l2n(t - i), all fp32
//   similarity  the row-wise cosine of text and image embeddings and the conflict score 1 - (cos + 1) / 2
// One wave per row or sample, fixed reduction trees, no atomics: a sample's results are the same bits alone and inside any batch.
#include "rowwise.hpp"
#include "gemm_f32.hpp"

namespace {

// ---- pack: one workgroup, a wave per sample, then the fixed-order scan ufnd_text_pack runs (pack_scan_rows)
__global__ __launch_bounds__(PACK_THREADS) void clip_text_pack_kernel(const int64_t* ids, int B, int L, int eos, int32_t* e, int32_t* cu,
                                                                      int32_t* row_src) {
  __shared__ int lens[PACK_MAX_B];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int b = wave; b < B; b += PACK_THREADS / 64) {
    // eos == 2 (the legacy configs): the first position of the largest id; otherwise the first position equal to eos, 0 if there is
    // none (HF: the argmax of an all-zero row)
    long long best = eos == 2 ? INT64_MIN : 0;
    int pos = eos == 2 ? 0 : L;
    for (int l = lane; l < L; l += 64) {
      const long long id = ids[(size_t)b * L + l];
      if (eos == 2) {
        if (id > best) { best = id; pos = l; }
      } else if (id == eos && l < pos) {
        pos = l;
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const long long ob = __shfl_xor(best, o, 64);
      const int op = __shfl_xor(pos, o, 64);
      if (ob > best || (ob == best && op < pos)) { best = ob; pos = op; }
    }
    if (pos >= L) pos = 0;
    if (lane == 0) {
      lens[b] = pos + 1;
      e[b] = pos;
    }
  }
  pack_scan_rows(lens, B, L, cu, row_src);
}

// ---- embed: one wave per row of H = 256 NI columns
template <int NI>
__global__ __launch_bounds__(256) void clip_text_embed_kernel(const int64_t* ids, const float* tok, const float* pos, __bf16* ob, float* of, int M,
                                                              int L, int H, int vocab, const int32_t* row_src, const int* m_live) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M || (m_live && row >= *m_live)) return;
  const int src = row_src ? row_src[row] : row;      // packed rows of ufnd_clip_text_pack: the (B, L) index of the token
  long long id = ids[src];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);      // never read outside the table
  int l = src % L;
  l = l < 0 ? 0 : l;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int col = 4 * lane + 256 * i;
    const f32x4 v = ld4(tok + (size_t)id * H + col) + ld4(pos + (size_t)l * H + col);
    *reinterpret_cast<f32x4*>(of + (size_t)row * H + col) = v;
    bf16x4 o = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
    *reinterpret_cast<bf16x4*>(ob + (size_t)row * H + col) = o;
  }
}

// ---- pool: LayerNorm of row e(b) (padded: b L + e[b]; packed: cu[b + 1] - 1), ufnd_layernorm's arithmetic (ln_row), bf16 out
template <int NI>
__global__ __launch_bounds__(256) void clip_text_pool_kernel(const float* x, const int32_t* e, const int32_t* cu, const float* gamma, const float* beta,
                                                             __bf16* out, int B, int L, int H, float eps) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  int eb = e[b];
  eb = eb < 0 ? 0 : (eb >= L ? L - 1 : eb);      // (the pack kernel's own output; this keeps a foreign e inside the sample)
  const size_t row = cu ? (size_t)cu[b + 1] - 1 : (size_t)b * L + eb;
  f32x4 v[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) v[i] = ld4(x + row * H + 4 * lane + 256 * i);
  ln_row<NI>(v, H, eps, gamma, beta, lane);
  store_row<NI>(v, out, nullptr, b, H, lane);
}

// ---- head epilogue: one workgroup per sample.  z (2, B, D): the two Linears' pre-activations (text, image).
__global__ __launch_bounds__(256) void semantic_head_kernel(const float* z, float* out_t, float* out_i, float* out_g, int B, int D) {
  __shared__ float red[4];
  const size_t r = (size_t)blockIdx.x * D;
  const float* zt = z + r;
  const float* zi = z + (size_t)B * D + r;
  float qt = 0.0f, qi = 0.0f, qg = 0.0f;
  for (int c = threadIdx.x; c < D; c += 256) {
    const float t = gelu_f(zt[c]), i = gelu_f(zi[c]), g = t - i;
    out_t[r + c] = t; out_i[r + c] = i; out_g[r + c] = g;      // (each thread rereads its own elements below)
    qt += t * t; qi += i * i; qg += g * g;
  }
  const float nt = sqrtf(block_sum4(qt, red)) + 1e-9f;
  const float ni = sqrtf(block_sum4(qi, red)) + 1e-9f;
  const float ng = sqrtf(block_sum4(qg, red)) + 1e-9f;
  for (int c = threadIdx.x; c < D; c += 256) {
    out_t[r + c] = out_t[r + c] / nt;
    out_i[r + c] = out_i[r + c] / ni;
    out_g[r + c] = out_g[r + c] / ng;
  }
}

// ---- similarity: one wave per sample
__global__ __launch_bounds__(256) void clip_similarity_kernel(const float* t, const float* im, float* sim, float* conflict, int B, int D) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  float d = 0.0f, qt = 0.0f, qi = 0.0f;
  for (int c = 4 * lane; c < D; c += 256) {
    const f32x4 a = ld4(t + (size_t)b * D + c), v = ld4(im + (size_t)b * D + c);
#pragma unroll
    for (int k = 0; k < 4; ++k) { d += a[k] * v[k]; qt += a[k] * a[k]; qi += v[k] * v[k]; }
  }
  d = wave_sum(d);
  qt = wave_sum(qt);
  qi = wave_sum(qi);
  if (lane == 0) {
    float c = d / ((sqrtf(qt) + 1e-9f) * (sqrtf(qi) + 1e-9f));
    c = fminf(1.0f, fmaxf(-1.0f, c));      // (rounding can leave a parallel pair an ulp outside; the conflict score stays in [0, 1])
    sim[b] = c;
    conflict[b] = 1.0f - (c + 1.0f) * 0.5f;
  }
}

int embed_checks(const char* what, const int64_t* ids, const float* tok, const float* pos, void* x_bf16, float* x_f32, int rows, int L, int H, int vocab,
                 int max_pos) {
  UFND_REQUIRE(ids && tok && pos && x_bf16 && x_f32, "%s: null argument", what);
  UFND_REQUIRE(h_ok(H) && rows >= 1 && L >= 1 && L <= max_pos && vocab >= 1, "%s: rows=%d L=%d H=%d vocab=%d max_position=%d (L <= max_position)", what,
               rows, L, H, vocab, max_pos);
  UFND_REQUIRE(ufnd_aligned(tok, 16) && ufnd_aligned(pos, 16) && ufnd_aligned(x_f32, 16) && ufnd_aligned(x_bf16, 8), "%s: alignment", what);
  return UFND_OK;
}

}  // namespace

extern "C" int ufnd_clip_text_pack(const int64_t* ids, int B, int L, int eos_token_id, int32_t* e, int32_t* cu_seqlens, int32_t* row_src,
                                   void* stream_) {
  UFND_REQUIRE(ids && e && cu_seqlens && row_src, "clip_text_pack: null argument");
  UFND_REQUIRE(B >= 1 && B <= PACK_MAX_B && L >= 1 && (long long)B * L < (1ll << 31), "clip_text_pack: B=%d L=%d (B <= %d)", B, L, PACK_MAX_B);
  hipLaunchKernelGGL(clip_text_pack_kernel, dim3(1), dim3(PACK_THREADS), 0, (hipStream_t)stream_, ids, B, L, eos_token_id, e, cu_seqlens, row_src);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_clip_text_embed(const int64_t* ids, const float* tok, const float* pos, void* x_bf16, float* x_f32, int B, int L, int H, int vocab,
                                    int max_position, void* stream_) {
  UFND_REQUIRE(B >= 1 && (long long)B * L < (1ll << 31), "clip_text_embed: B=%d L=%d", B, L);
  const int rc = embed_checks("clip_text_embed", ids, tok, pos, x_bf16, x_f32, B * L, L, H, vocab, max_position);
  if (rc != UFND_OK) return rc;
  NI_LAUNCH(H, clip_text_embed_kernel, dim3(ufnd_cdiv(B * L, 4)), (hipStream_t)stream_, ids, tok, pos, (__bf16*)x_bf16, x_f32, B * L, L, H, vocab,
            (const int32_t*)nullptr, (const int*)nullptr);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_clip_text_embed_live(const int64_t* ids, const int32_t* row_src, const int* m_live, const float* tok, const float* pos, void* x_bf16,
                                         float* x_f32, int capacity, int L, int H, int vocab, int max_position, void* stream_) {
  UFND_REQUIRE(row_src && m_live, "clip_text_embed_live: null argument");
  const int rc = embed_checks("clip_text_embed_live", ids, tok, pos, x_bf16, x_f32, capacity, L, H, vocab, max_position);
  if (rc != UFND_OK) return rc;
  NI_LAUNCH(H, clip_text_embed_kernel, dim3(ufnd_cdiv(capacity, 4)), (hipStream_t)stream_, ids, tok, pos, (__bf16*)x_bf16, x_f32, capacity, L, H, vocab,
            row_src, m_live);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_clip_text_pool(const float* x, const int32_t* e, const int32_t* cu_seqlens, const float* gamma, const float* beta, void* out_bf16,
                                   int B, int L, int H, float eps, void* stream_) {
  UFND_REQUIRE(x && e && gamma && beta && out_bf16, "clip_text_pool: null argument");
  UFND_REQUIRE(h_ok(H) && B >= 1 && L >= 1 && (long long)B * L < (1ll << 31), "clip_text_pool: B=%d L=%d H=%d (H: 256/512/768/1024)", B, L, H);
  UFND_REQUIRE(ufnd_aligned(x, 16) && ufnd_aligned(gamma, 16) && ufnd_aligned(beta, 16) && ufnd_aligned(out_bf16, 8), "clip_text_pool: alignment");
  NI_LAUNCH(H, clip_text_pool_kernel, dim3(ufnd_cdiv(B, 4)), (hipStream_t)stream_, x, e, cu_seqlens, gamma, beta, (__bf16*)out_bf16, B, L, H, eps);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_semantic_head(const float* text, const float* image, const float* wt, const float* bt, const float* wi, const float* bi,
                                  float* workspace, float* out_text, float* out_image, float* out_gap, int B, int D, int K, void* stream_) {
  UFND_REQUIRE(text && image && wt && bt && wi && bi && workspace && out_text && out_image && out_gap, "semantic_head: null argument");
  UFND_REQUIRE(B >= 1 && B <= 65535 && D >= 32 && D % 32 == 0 && K >= 4 && K % 4 == 0 && (long long)B * D < (1ll << 30), "semantic_head: B=%d D=%d K=%d", B,
               D, K);
  const NtProb p[2] = {nt_linear(text, K, wt, K, bt, workspace, D, B, D, K), nt_linear(image, K, wi, K, bi, workspace + (size_t)B * D, D, B, D, K)};
  const int rc = launch_nt(p, 2, nullptr, (hipStream_t)stream_);      // (the exact-fp32 skinny GEMM: both products in one launch)
  if (rc != UFND_OK) return rc;
  hipLaunchKernelGGL(semantic_head_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream_, (const float*)workspace, out_text, out_image, out_gap, B, D);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_clip_similarity(const float* text, const float* image, float* similarity, float* conflict, int B, int D, void* stream_) {
  UFND_REQUIRE(text && image && similarity && conflict, "clip_similarity: null argument");
  UFND_REQUIRE(B >= 1 && D >= 4 && D % 4 == 0 && (long long)B * D < (1ll << 31), "clip_similarity: B=%d D=%d (D a multiple of 4)", B, D);
  UFND_REQUIRE(ufnd_aligned(text, 16) && ufnd_aligned(image, 16), "clip_similarity: 16-B alignment required");
  hipLaunchKernelGGL(clip_similarity_kernel, dim3(ufnd_cdiv(B, 4)), dim3(256), 0, (hipStream_t)stream_, text, image, similarity, conflict, B, D);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}
