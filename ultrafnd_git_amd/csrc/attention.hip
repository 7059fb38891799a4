// Multi-head self-attention, forward only: ctx = softmax(Q K^T / sqrt(64) + mask) V.
// (BertSelfAttention eager path / CLIPAttention; head_dim 64, 12 heads in both encoders.)
//
// One workgroup = one (batch, head, 128-query block); wave w owns 32 queries.  Keys/values are
// walked in blocks of 64 with an online softmax, so L = 50 (ViT), 128 and 512 (BERT) share
// the code and nothing of size L x L ever exists.
//
// MFMA orientation (v_mfma_f32_16x16x32_bf16; C/D: column = lane & 15, row = 4*(lane>>4)+r):
//   S^T[key][query] = K Q^T      A = K rows from LDS (ds_read_b128, swizzled), B = Q from registers
//     -> a lane holds ONE query (its column) and 4 keys per tile: the softmax statistics of a
//        query live in the 4 lanes {q, q+16, q+32, q+48}: two __shfl_xor, no LDS.
//   O^T[d][query] = V^T P^T      B = P^T: the S^T accumulators, converted to bf16 IN PLACE --
//        the accumulator layout of step 1 is exactly the B-operand layout of step 2 once the
//        contraction index is ordered as (keys 4g..4g+3 of tile 2s, keys 4g..4g+3 of tile 2s+1)
//        A = V^T fragments in that same key order, produced from the row-major V tile in LDS
//        by ds_read_b64_tr_b16 (hardware transpose): 4 keys x 16 d per 16-lane group.
// Masking follows HF: masked keys get the constant finfo.min-like score (a fully masked row
// degenerates to a uniform average, not NaN); keys beyond L contribute exactly zero.
// Training dropout (DROP, ufnd_attention_bf16_lse_dropout): P^T is multiplied by the mask in fp32 just before its in-place bf16
// conversion; l and lse stay those of the undropped probabilities.  The mask is drawn, never stored: element (q, k) of (b, h) is
// ((b heads + h) L + q) Lp + k with Lp = L rounded up to 4, so the 4 keys a lane holds per tile (4g..4g+3: aligned) are one
// Philox evaluation.  DESIGN.md section 4.
#include "attn_softmax.hpp"

// No implicit contraction: the block body (scores, softmax, rescale, P V, normalise and store) is attn_softmax.hpp's, the very
// code the fused projection + attention kernel (gemm_bf16_kernel.hpp, ATT) runs, so the two produce the same bits by construction;
// fused multiply-adds are spelled out.
#pragma clang fp contract(off)

namespace {

// Experiment switches of tools/clip_text_throughput.py (python -m ultrafnd_git_amd.build --defs=...): the causal entries without the
// key-block and wave skipping (UFND_CAUSAL_SKIP=0), and in the 4-wave, 128-query form (UFND_CAUSAL_WAVES=4)
#ifndef UFND_CAUSAL_SKIP
#define UFND_CAUSAL_SKIP 1
#endif
#ifndef UFND_CAUSAL_WAVES
#define UFND_CAUSAL_WAVES 2
#endif
constexpr int QB = 128;          // queries per workgroup (4 waves x 32; the short-sequence form: 2 waves, 64 queries)
constexpr float NEG_MASK = -3.0e38f;

// KB = keys per block (64: 162 registers, three workgroups per CU; 128: 240 registers, two -- measured at L = 512, B = 128 in round 3:
// 218 against 211 us per launch, not selected)
// NW = waves per workgroup (32 queries each).  Sequences of <= 64 tokens (ViT-B/32: 50) run with NW = 2: the 4-wave form spends
// half its waves on clamped duplicate queries there, and its 216 registers allow 8 waves per CU either way -- twice the
// samples in flight with 2-wave workgroups (a block is one dependent chain: loads -> S -> softmax -> O -> store).
// DROP: the Philox draws need ~170 registers in the 2-wave form; at three waves per SIMD it spilled, so it runs at two.
// CAUSAL (the CLIP text tower, ufnd_attention_bf16_causal[_varlen]): key k is visible to query q iff k <= q and the key mask keeps it.
// A workgroup walks the key blocks up to the one that holds its last query; a wave skips the blocks past its own last query (every
// probability there is +0 once the wave has seen key 0, which the entries' precondition makes visible) and, when all its queries are
// clamped duplicates (nothing of it is stored), every block; the per-element test runs
// in the blocks that cross a wave's diagonal only, on the 4 keys a lane holds per tile (attn_softmax.hpp).
template <int KB, int NW = 4, bool DROP = false, bool CAUSAL = false>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(NW == 2 && !DROP ? 3 : 2))) void attention_kernel(const __bf16* qkv, const int32_t* mask, __bf16* ctx, int L,
                                                        int heads, float scale_log2e, const int32_t* cu, float* lse, int nqb,
                                                        ufnd_dropout dr) {
  __shared__ __attribute__((aligned(16))) char ks[KB * 128];
  __shared__ __attribute__((aligned(16))) char vs[KB * 128];
  __shared__ __attribute__((aligned(16))) float kbias[KB];

  // 1-D grid of (query block, head, sample), query block fastest, in XCD-contiguous order: at L = 512 the four query blocks of a
  // (sample, head) each walk the same 128 KB of K / V -- dealt round-robin over the XCDs they fetched it four times over the
  // fabric (1.07 GB per launch at B = 128: the launch ran at the fabric's rate, not the matrix pipes')
  const int lid = xcd_contiguous_id((int)blockIdx.x, (int)gridDim.x);
  const int qb = lid % nqb, h = (lid / nqb) % heads, b = lid / (nqb * heads);
  const int H = heads * 64, ld = 3 * H;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, fr = lane & 15, g = lane >> 4;
  size_t tok0 = (size_t)b * L, mtok0 = tok0;      // (the key mask keeps the padded (B, L) layout)
  if (cu) {              // packed (un-padded) sequences: rows cu[b] .. cu[b+1], keys masked by mask[b L + key] if a mask is given
    tok0 = (size_t)cu[b];
    L = cu[b + 1] - cu[b];
    if (qb * (NW * 32) >= L) return;      // (block-uniform, before any barrier)
  }
  int kend = L;      // keys the workgroup walks
  if constexpr (CAUSAL && UFND_CAUSAL_SKIP) kend = (qb + 1) * (NW * 32) < L ? (qb + 1) * (NW * 32) : L;      // (block-uniform, before any barrier): 1 + its last query

  // Q fragments (B operand): lane (query fr, g) holds Q[query][8g + 32kk .. +7]
  bf16x8 qf[2][2];
  int qrow[2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int q = qb * (NW * 32) + wave * 32 + qt * 16 + fr;
    qrow[qt] = q;
    const int qc = q < L ? q : L - 1;
    const __bf16* src = qkv + (tok0 + qc) * ld + h * 64 + 8 * g;
    qf[qt][0] = *reinterpret_cast<const bf16x8*>(src);
    qf[qt][1] = *reinterpret_cast<const bf16x8*>(src + 32);
  }

  uint64_t dseed = 0, dstep = 0;
  uint32_t drow[2] = {0u, 0u};      // DROP: the Philox counter of (query, key group 0) per query tile
  if constexpr (DROP) {
    dseed = dr.state->seed;
    dstep = dropout_step_key(dr.state);
    const uint32_t lp4 = (uint32_t)(L + 3) >> 2;
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) drow[qt] = ((uint32_t)(b * heads + h) * (uint32_t)L + (uint32_t)qrow[qt]) * lp4 + (uint32_t)g;
  }

  f32x4 o[4][2];
  float m_run[2], l_run[2];
  attn_init(o, m_run, l_run);

  // K / V blocks travel HBM -> registers -> LDS.  With several blocks to walk (the 4-wave form: L > 64) the loads of block k+1
  // are issued right after block k has been written to LDS and stay in flight under block k's S^T / softmax / PV work (the
  // issue-early / write-late split: their latency was exposed in front of every block before); one register set, +16 VGPRs.
  constexpr int NPC = KB * 8 / (NW * 64);       // 16-B pieces per thread per matrix
  constexpr bool PREFETCH = NW == 4;
  bf16x8 kreg[NPC], vreg[NPC];
  float breg = -INFINITY;
  auto load_block = [&](int kb0) {
#pragma unroll
    for (int it = 0; it < NPC; ++it) {
      const int idx = tid + NW * 64 * it, key = idx >> 3, c = idx & 7;
      const int kr = (kb0 + key) < L ? (kb0 + key) : L - 1;
      const __bf16* src = qkv + (tok0 + kr) * ld + H + h * 64 + c * 8;
      kreg[it] = *reinterpret_cast<const bf16x8*>(src);
      vreg[it] = *reinterpret_cast<const bf16x8*>(src + H);
    }
    if (tid < KB) {
      const int key = kb0 + tid;
      breg = -INFINITY;
      if (key < L) breg = (!mask || mask[mtok0 + key] != 0) ? 0.0f : NEG_MASK;
    }
  };
  if constexpr (PREFETCH) load_block(0);
  for (int kb0 = 0; kb0 < kend; kb0 += KB) {
    __syncthreads();  // previous block's LDS reads are done
    // ---- stage K and V tiles (row-major 128-B rows, swizzled 16-B chunks) and the key bias
    if constexpr (!PREFETCH) load_block(kb0);
#pragma unroll
    for (int it = 0; it < NPC; ++it) {
      const int idx = tid + NW * 64 * it, key = idx >> 3, c = idx & 7;
      *reinterpret_cast<bf16x8*>(ks + key * 128 + ((c ^ ((key >> 1) & 7)) << 4)) = kreg[it];
      *reinterpret_cast<bf16x8*>(vs + key * 128 + ((c ^ (((key >> 1) & 3) << 1)) << 4)) = vreg[it];
    }
    if (tid < KB) kbias[tid] = breg;
    __syncthreads();
    if constexpr (PREFETCH) {
      if (kb0 + KB < kend) load_block(kb0 + KB);
    }

    const int wq0 = qb * (NW * 32) + wave * 32;      // the wave's first query
    if constexpr (CAUSAL && UFND_CAUSAL_SKIP) {
      if (kb0 > wq0 + 31 || wq0 >= L) continue;      // (wave-uniform; both barriers of the iteration are behind us / at the loop top)
    }
    if constexpr (KB == 64) {
      if (masked_block_is_noop(kbias, lane, m_run)) continue;      // (attn_softmax.hpp; both barriers of the iteration are behind us / at the loop top)
    }
    // ---- S^T = K Q^T on the staged block (key k of the block is LDS row k)
    constexpr int KT = KB / 16;
    const auto key_row = [](int k) { return k; };
    f32x4 s[KT][2];
    attn_scores<KT>(ks, key_row, qf, fr, g, s);

    // ---- online softmax
    bool any_masked = __any(kbias[lane] != 0.0f);            // (the block's key-bias words, 64 per pass; wave-uniform)
    if constexpr (KB == 128) any_masked = any_masked || __any(kbias[64 + lane] != 0.0f);
    if constexpr (CAUSAL) any_masked = any_masked || kb0 + KB - 1 > wq0;      // the block crosses the wave's diagonal
    bf16x8 pf[KT / 2][2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      f32x4 dm[KT];
      if constexpr (DROP) {
        // keys kb0 + 16 kt + 4 g .. +3 of this lane's query: counter (q Lp + kb0 + 16 kt + 4 g) / 4.  Queries or keys beyond L draw
        // multipliers nobody uses (their P is 0)
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
          float m4[4];
          dropout_mul4_ctr(dseed, dstep, dr.p, dr.tag, drow[qt] + (uint32_t)(kb0 >> 2) + 4u * kt, m4);
          dm[kt] = f32x4{m4[0], m4[1], m4[2], m4[3]};
        }
      }
      attn_softmax_rescale<KT, DROP, CAUSAL>(s, qt, kbias, any_masked, g, scale_log2e, m_run, l_run, pf, o, dm, qrow[qt] - kb0 - 4 * g, NEG_MASK);
    }

    // ---- O^T += V^T P^T
    attn_pv<KT>(vs, key_row, pf, o, fr, g);
  }

  // ---- normalise and store: lane holds O^T[d = 16dt + 4g + r][query fr]
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    float l;
    const float inv = attn_finish(l_run[qt], l);
    // training forwards keep the query's log-sum-exp (log2 domain, as the scores above): the backward recomputes P from it
    if (lse && g == 0 && qrow[qt] < L) lse[(tok0 + qrow[qt]) * heads + h] = m_run[qt] + log2f(l);
    if (qrow[qt] < L) attn_store_ctx(ctx + (tok0 + qrow[qt]) * H + h * 64 + 4 * g, o, qt, inv);
  }
}

// One launch of attention_kernel as an entry describes it.  The checks, the form and the grid are decided here, once.
constexpr int CQ = 32 * UFND_CAUSAL_WAVES;      // queries per workgroup of the causal forms
struct AttnLaunch {
  const char* name;                  // the entry's name in its messages
  const void* qkv;
  const int32_t* key_mask;
  void* ctx;
  int B, L, heads;                   // (varlen: L is max_len)
  bool varlen = false;               // packed rows: sample b's are cu[b] .. cu[b+1].  A flag of its own, because a varlen entry
  const int32_t* cu = nullptr;       // refuses a NULL cu: cu == nullptr alone would silently select the padded form
  float* lse = nullptr;
  bool dropout = false;              // train-mode dropout on the probabilities: needs lse and drop
  const ufnd_dropout* drop = nullptr;
  bool causal = false;
};

template <int NW, bool DROP, bool CAUSAL>
void launch_form(const AttnLaunch& a, int nqb, hipStream_t stream) {
  const float scale_log2e = 0.125f * 1.44269504088896340736f;  // 1/sqrt(64) * log2(e)
  hipLaunchKernelGGL((attention_kernel<64, NW, DROP, CAUSAL>), dim3(nqb * a.heads * a.B), dim3(NW * 64), 0, stream, (const __bf16*)a.qkv, a.key_mask,
                     (__bf16*)a.ctx, a.L, a.heads, scale_log2e, a.cu, a.lse, nqb, DROP ? *a.drop : ufnd_dropout{});
}

// Forms.  Causal (the CLIP text tower; built for its L <= 77): workgroups of UFND_CAUSAL_WAVES = 2 waves and 64 queries, so that at
// L = 77 query block 0 never touches key block 1 and only one wave of four runs on clamped duplicate queries.  Otherwise
// 4 waves and 128 queries, except for padded samples of L <= 64 (the ViT's 50), which take the 2-wave form (attention_kernel).
int attention_launch(const AttnLaunch& a, void* stream_) {
  UFND_REQUIRE(a.qkv && a.ctx && (!a.varlen || a.cu) && (!a.dropout || (a.lse && a.drop && a.drop->state)), "%s: null operand", a.name);
  if (a.dropout) UFND_REQUIRE(a.drop->p > 0.0f && a.drop->p < 1.0f, "%s: p=%g (0 < p < 1; p = 0 is ufnd_attention_bf16_lse)", a.name, (double)a.drop->p);
  UFND_REQUIRE(a.B >= 1 && (!a.varlen || a.B <= 65535) && a.L >= 1 && a.L <= 4096 && a.heads >= 1 && a.heads <= 64, "%s: B=%d %s=%d heads=%d", a.name,
               a.B, a.varlen ? "max_len" : "L", a.L, a.heads);
  UFND_REQUIRE(ufnd_aligned(a.qkv, 16) && ufnd_aligned(a.ctx, 16), "%s: 16-B alignment required", a.name);
  const bool two_waves = !a.causal && !a.varlen && a.L <= 64;
  const int nqb = ufnd_cdiv(a.L, a.causal ? CQ : (two_waves ? 64 : QB));
  // (vacuous for ufnd_attention_bf16_varlen_masked, which never had this check: B <= 65535, heads <= 64 and nqb <= 32 stay below 2^31)
  UFND_REQUIRE((long long)a.B * a.heads * nqb < (1ll << 31), "%s: grid too large", a.name);
  if (a.dropout) UFND_REQUIRE(ufnd_attn_dropout_fits(a.B, a.L, a.heads), "%s: B=%d L=%d heads=%d overflows the 32-bit dropout counter", a.name, a.B, a.L, a.heads);
  hipStream_t stream = (hipStream_t)stream_;
  if (a.causal) launch_form<UFND_CAUSAL_WAVES, false, true>(a, nqb, stream);
  else if (a.dropout && two_waves) launch_form<2, true, false>(a, nqb, stream);
  else if (a.dropout) launch_form<4, true, false>(a, nqb, stream);
  else if (two_waves) launch_form<2, false, false>(a, nqb, stream);
  else launch_form<4, false, false>(a, nqb, stream);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

}  // namespace

extern "C" int ufnd_attention_bf16(const void* qkv, const int32_t* key_mask, void* ctx, int B, int L, int heads, void* stream_) {
  return attention_launch({"attention", qkv, key_mask, ctx, B, L, heads}, stream_);
}

extern "C" int ufnd_attention_bf16_lse(const void* qkv, const int32_t* key_mask, void* ctx, float* lse, int B, int L, int heads,
                                       void* stream_) {
  AttnLaunch a{"attention", qkv, key_mask, ctx, B, L, heads};
  a.lse = lse;
  return attention_launch(a, stream_);
}

extern "C" int ufnd_attention_bf16_varlen_masked(const void* qkv, const int32_t* cu_seqlens, const int32_t* key_mask, void* ctx, int B,
                                                 int max_len, int heads, void* stream_) {
  AttnLaunch a{"attention_varlen", qkv, key_mask, ctx, B, max_len, heads};
  a.varlen = true, a.cu = cu_seqlens;
  return attention_launch(a, stream_);
}

extern "C" int ufnd_attention_bf16_lse_dropout(const void* qkv, const int32_t* key_mask, void* ctx, float* lse, int B, int L, int heads,
                                               const ufnd_dropout* drop, void* stream_) {
  AttnLaunch a{"attention_dropout", qkv, key_mask, ctx, B, L, heads};
  a.lse = lse, a.dropout = true, a.drop = drop;
  return attention_launch(a, stream_);
}

// Precondition of the causal entries: key 0 of every sample is visible (key_mask[b][0] != 0); rows whose every visible key is masked
// are unspecified.
extern "C" int ufnd_attention_bf16_causal(const void* qkv, const int32_t* key_mask, void* ctx, int B, int L, int heads, void* stream_) {
  AttnLaunch a{"attention_causal", qkv, key_mask, ctx, B, L, heads};
  a.causal = true;
  return attention_launch(a, stream_);
}

extern "C" int ufnd_attention_bf16_causal_varlen(const void* qkv, const int32_t* cu_seqlens, const int32_t* key_mask, void* ctx, int B, int max_len,
                                                 int heads, void* stream_) {
  AttnLaunch a{"attention_causal_varlen", qkv, key_mask, ctx, B, max_len, heads};
  a.varlen = a.causal = true, a.cu = cu_seqlens;
  return attention_launch(a, stream_);
}
