// The forward attention block body, written once: attention_kernel (attention.hip) and the three fused projection + attention branches
// of gemm_bf16_kernel.hpp (short samples, sample tiles, padded samples / slot bins) are loops over their own geometry -- which LDS row a
// key is, where the block's bias words lie, how many key blocks there are, where a query row goes -- around the pieces below.  That
// the fused launches produce the bits of the two-launch form follows from the source: there is one copy of every operation.
//
// A wave owns 32 queries (two 16-query tile columns qt) of one head and walks the keys in blocks of 16 KT (KT = 4: 64 keys):
//   attn_init             o = 0, m_run = -inf, l_run = 0
//   attn_q_frags          the wave's Q fragments from an LDS image (attention.hip loads them from global memory)
//   attn_scores           S^T = K Q^T of the block            (A = K rows from the swizzled LDS image, B = Q from registers)
//   attn_softmax_rescale  online_softmax_block of one tile column + the rescale of its running output
//   attn_pv               O^T += V^T P^T of the block         (A = V^T by transposed LDS reads, B = P^T: the score accumulators in place)
//   attn_finish           a query's row sum over its four lanes and the reciprocal
//   attn_store_ctx        the normalised output row, rounded to bf16
//   attn_unit             the loop of the fused kernels around all of these: one unit of 32 queries against the key blocks of its sample,
//                         all operands in LDS images (attention.hip stages K / V through LDS block by block and keeps its own loop)
// Lane (fr, g) = (lane & 15, lane >> 4).  `key_row` maps a key index of the block to its row in the K / V image.
//
// online_softmax_block: one 64-key block of the online softmax, for one 16-query tile column of a wave.
// Scores arrive as the S^T accumulators s[kt][qt] (row = key 16 kt + 4 g + r, column = the lane's query); on return pf holds
// exp2(score - m_new) rounded to bf16 in the B-operand order of the P V product, m_run / l_run are updated, and the factor the
// running output must be multiplied by is returned.
//
// The softmax is VALU-bound (32 scores per lane per block against 32 MFMAs per wave), so the common case -- a block WITHOUT a
// masked or out-of-range key (`any_masked` false: wave-uniform, from the block's key-bias words) -- takes the short path: the maximum
// over the raw accumulators, then ONE fused multiply-add and ONE v_exp_f32 per score (exp2(s * scale - m), scale > 0 commutes with
// the maximum).  Blocks with a masked key keep HF's semantics (masked score = the finfo.min-like constant, so a fully masked row
// degenerates to a uniform average) at three more instructions per score.
#pragma once
#include "common.hpp"

// No implicit contraction in any piece of this file: the fused multiply-adds are spelled out.
#pragma clang fp contract(off)

// One 16-B fragment of a 128-B row of an LDS image whose chunks are swizzled by the row (chunk ^= (row >> 1) & 7)
__device__ __forceinline__ bf16x8 lds_frag(const char* tile, int row, int chunk) {
  return *reinterpret_cast<const bf16x8*>(tile + row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4));
}

// A 64-key block whose keys are ALL masked (or beyond L) changes nothing once every query of the wave has seen a live key: its scores
// are the -3e38 constant (or -inf), so m_new = m_run, alpha = 1, every p = exp2(-3e38 - m_run) = +0 exactly, l and O stay as they are.
// Wave-uniform test for that case (kb = the block's 64 key-bias words, one per lane): the wave then skips the block's 32 + 32 MFMAs
// and its softmax -- bit-identical output.  Padding is a suffix of masked keys, so for a batch of ragged lengths this is most of
// the key blocks of the short samples.  A wave whose queries have seen only masked keys so far (m_run still at the mask constant:
// HF's uniform-average degenerate case) does NOT skip.
__device__ __forceinline__ bool masked_block_is_noop(const float* kb, int lane, const float (&m_run)[2]) {
  return __all(kb[lane] != 0.0f) && __all(m_run[0] > -1.0e30f && m_run[1] > -1.0e30f);
}

// DROP (attention.hip's training forward with dropout): pf gets exp2(score - m_new) * dm[kt][r] -- the dropout multiplier applied in fp32
// just before the bf16 rounding -- while l_run keeps summing the UNDROPPED probabilities (HF: dropout after the softmax).
// CAUSAL (attention.hip's causal entries; the caller passes any_masked = true for a block that crosses the diagonal): key 16 kt + r
// of this lane's four-key groups is visible iff 16 kt + r <= qk (qk = the lane's query - the block's first key - 4 g); a live key
// above the diagonal scores causal_neg, the key mask's own constant.
template <int KT, bool DROP = false, bool CAUSAL = false>
__device__ __forceinline__ float online_softmax_block(f32x4 (&s)[KT][2], const int qt, const float* kbias, const bool any_masked, const int g,
                                                      const float scale_log2e, float& m_run, float& l_run, bf16x8 (&pf)[KT / 2][2],
                                                      const f32x4* dm = nullptr, const int qk = 0, const float causal_neg = 0.0f) {
  float mx = -INFINITY, lsum = 0.0f, m_new, alpha;
  if (any_masked) {
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      const f32x4 kbv = *reinterpret_cast<const f32x4*>(kbias + kt * 16 + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = (kbv[r] == 0.0f) ? s[kt][qt][r] * scale_log2e : kbv[r];
        if constexpr (CAUSAL) {
          if (kbv[r] == 0.0f && 16 * kt + r > qk) v = causal_neg;
        }
        s[kt][qt][r] = v;
        mx = fmaxf(mx, v);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    m_new = fmaxf(m_run, mx);                    // finite: every block holds a key < L
    alpha = fast_exp2(m_run - m_new);            // first block: exp2(-inf) = 0
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = fast_exp2(s[kt][qt][r] - m_new);
        lsum += p;
        if constexpr (DROP) pf[kt >> 1][qt][(kt & 1) * 4 + r] = (__bf16)(p * dm[kt][r]);
        else pf[kt >> 1][qt][(kt & 1) * 4 + r] = (__bf16)p;
      }
  } else {
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[kt][qt][r]);
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    m_new = fmaxf(m_run, mx * scale_log2e);
    alpha = fast_exp2(m_run - m_new);
    const float neg_m = -m_new;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = fast_exp2(__builtin_fmaf(s[kt][qt][r], scale_log2e, neg_m));
        lsum += p;
        if constexpr (DROP) pf[kt >> 1][qt][(kt & 1) * 4 + r] = (__bf16)(p * dm[kt][r]);
        else pf[kt >> 1][qt][(kt & 1) * 4 + r] = (__bf16)p;
      }
  }
  l_run = __builtin_fmaf(l_run, alpha, lsum);
  m_run = m_new;
  return alpha;
}

__device__ __forceinline__ void attn_init(f32x4 (&o)[4][2], float (&m_run)[2], float (&l_run)[2]) {
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) o[dt][qt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) m_run[qt] = -INFINITY, l_run[qt] = 0.f;
}

// Q fragments (B operand) from the Q image: lane (fr, g) holds Q[query][8g + 32kk .. +7] of query 16 qt + fr, at image row q_row(16 qt + fr)
template <class QRow>
__device__ __forceinline__ void attn_q_frags(const char* qimg, QRow q_row, int fr, int g, bf16x8 (&qf)[2][2]) {
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int row = q_row(qt * 16 + fr);
    qf[qt][0] = lds_frag(qimg, row, g);
    qf[qt][1] = lds_frag(qimg, row, g + 4);
  }
}

// S^T = K Q^T : KT key tiles x 2 query tiles, contraction over the 64 head columns in two steps of 32 (kk outer, kt inner)
template <int KT, class KeyRow>
__device__ __forceinline__ void attn_scores(const char* kimg, KeyRow key_row, const bf16x8 (&qf)[2][2], int fr, int g, f32x4 (&s)[KT][2]) {
#pragma unroll
  for (int kt = 0; kt < KT; ++kt)
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) s[kt][qt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kk = 0; kk < 2; ++kk)
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      const bf16x8 kf = lds_frag(kimg, key_row(kt * 16 + fr), g + 4 * kk);
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) s[kt][qt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[qt][kk], s[kt][qt], 0, 0, 0);
    }
}

// The softmax of tile column qt over the block (scores kept in the log2 domain: exp(x) = exp2(x * log2 e)) and the rescale of its
// running output (the running maximum rarely moves after the first blocks: the rescale is skipped then)
template <int KT, bool DROP = false, bool CAUSAL = false>
__device__ __forceinline__ void attn_softmax_rescale(f32x4 (&s)[KT][2], const int qt, const float* kbias, const bool any_masked, const int g,
                                                     const float scale_log2e, float (&m_run)[2], float (&l_run)[2], bf16x8 (&pf)[KT / 2][2],
                                                     f32x4 (&o)[4][2], const f32x4* dm = nullptr, const int qk = 0, const float causal_neg = 0.0f) {
  const float alpha = online_softmax_block<KT, DROP, CAUSAL>(s, qt, kbias, any_masked, g, scale_log2e, m_run[qt], l_run[qt], pf, dm, qk, causal_neg);
  if (!__all(alpha == 1.0f)) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt][qt] *= alpha;
  }
}

// O^T += V^T P^T : contraction over the block's 16 KT keys in steps of 32 (ksd outer, dt inner).  The V image's rows are 128 B with
// the transposed-read swizzle (chunk ^= ((row >> 1) & 3) << 1); hardware-transposed read: 16-lane group g, lane 4q+p supplies
// &V[key][16dt + 4p] of keys 32 ksd + 4 g + q and that + 16
template <int KT, class KeyRow>
__device__ __forceinline__ void attn_pv(const char* vimg, KeyRow key_row, const bf16x8 (&pf)[KT / 2][2], f32x4 (&o)[4][2], int fr, int g) {
#pragma unroll
  for (int ksd = 0; ksd < KT / 2; ++ksd) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const int qq = fr >> 2, pp = fr & 3;
      const int k0 = 32 * ksd + 4 * g + qq;
      const int key0 = key_row(k0), key1 = key_row(k0 + 16);
      const int ch = 2 * dt + (pp >> 1);
      const int off0 = key0 * 128 + ((ch ^ (((key0 >> 1) & 3) << 1)) << 4) + 8 * (pp & 1);
      const int off1 = key1 * 128 + ((ch ^ (((key1 >> 1) & 3) << 1)) << 4) + 8 * (pp & 1);
      const s16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(vimg + off0));
      const s16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(vimg + off1));
      union { s16x4 s2[2]; bf16x8 v; } u;
      u.s2[0] = t0;
      u.s2[1] = t1;
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) o[dt][qt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(u.v, pf[ksd][qt], o[dt][qt], 0, 0, 0);
    }
  }
}

// The row sum l of the lane's query (its probabilities live in the lanes fr, fr + 16, fr + 32, fr + 48); returns 1 / l
__device__ __forceinline__ float attn_finish(const float l_run, float& l) {
  l = l_run;
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  return 1.0f / l;
}
__device__ __forceinline__ float attn_finish(const float l_run) {
  float l;
  return attn_finish(l_run, l);
}

// Normalise and store: the lane holds O^T[d = 16dt + 4g + r][its query]; dst = the query's ctx row at column 64 head + 4 g
__device__ __forceinline__ void attn_store_ctx(__bf16* dst, const f32x4 (&o)[4][2], const int qt, const float inv) {
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    bf16x4 ov = {(__bf16)(o[dt][qt][0] * inv), (__bf16)(o[dt][qt][1] * inv), (__bf16)(o[dt][qt][2] * inv), (__bf16)(o[dt][qt][3] * inv)};
    *reinterpret_cast<bf16x4*>(dst + dt * 16) = ov;
  }
}

// One unit of the fused projection + attention kernels: a wave's 32 queries of one head against the NKB 64-key blocks of their sample,
// all three operands in LDS images.  q_row maps a query of the unit (0..31), key_row a key of the sample (0 .. 64 NKB - 1) to its image
// row; kbias holds the sample's 64 NKB key-bias words (16-B aligned); SKIP: the masked-block skip of attention.hip runs.  The first nq
// queries are live: query q's normalised output goes to ctx + q * ldc (ctx = the unit's first query at its head's first column).
template <int NKB, bool SKIP, class QRow, class KeyRow>
__device__ __forceinline__ void attn_unit(const char* qimg, const char* kimg, const char* vimg, QRow q_row, KeyRow key_row, const float* kbias,
                                          const float scale_log2e, const int lane, __bf16* ctx, const int ldc, const int nq) {
  constexpr int KB = 64, KT = KB / 16;
  const int g = lane >> 4, fr = lane & 15;
  bf16x8 qf[2][2];
  attn_q_frags(qimg, q_row, fr, g, qf);
  f32x4 o[4][2];
  float m_run[2], l_run[2];
  attn_init(o, m_run, l_run);
#pragma unroll
  for (int kb0 = 0; kb0 < NKB * KB; kb0 += KB) {
    if constexpr (SKIP) {
      if (masked_block_is_noop(kbias + kb0, lane, m_run)) continue;      // (as attention.hip: bit-identical, see above)
    }
    const auto blk_row = [&](int k) { return key_row(kb0 + k); };
    f32x4 sc[KT][2];
    attn_scores<KT>(kimg, blk_row, qf, fr, g, sc);
    const bool any_masked = __any(kbias[kb0 + lane] != 0.0f);      // (64 bias words of this key block: one per lane; wave-uniform)
    bf16x8 pf[KT / 2][2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) attn_softmax_rescale<KT>(sc, qt, kbias + kb0, any_masked, g, scale_log2e, m_run, l_run, pf, o);
    attn_pv<KT>(vimg, blk_row, pf, o, fr, g);
  }
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const float inv = attn_finish(l_run[qt]);
    const int q = qt * 16 + fr;
    if (q < nq) attn_store_ctx(ctx + (size_t)q * ldc + 4 * g, o, qt, inv);
  }
}
