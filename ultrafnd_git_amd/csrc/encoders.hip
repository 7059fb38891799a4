// Row-wise pieces of the two encoders: LayerNorm, BERT embeddings, masked mean-pool + L2,
// ViT patchify / token assembly, frame pooling.  All HBM-bound: one wave per row, 16-B loads,
// wave-shuffle reductions, fp32 statistics; outputs feed the bf16 GEMMs directly.
#include "rowwise.hpp"

namespace {

template <int NI>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* x, int ldx, const float* gamma, const float* beta,
                                                        __bf16* ob, float* of, int M, int H, float eps, const int* m_live) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M || (m_live && row >= *m_live)) return;      // (m_live: M is the capacity, the first *m_live rows are live)
  f32x4 v[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) v[i] = ld4(x + (size_t)row * ldx + 4 * lane + 256 * i);
  ln_row<NI>(v, H, eps, gamma, beta, lane);
  store_row<NI>(v, ob, of, row, H, lane);
}

// Training dropout at a LayerNorm (the trainable text encoder, HF BertModel.train()); element (row, col) of the (M, H) site is
// row H + col: a lane's 4 columns are one Philox evaluation.
//   RESID (BertSelfOutput / BertOutput):  y = x + m o d  (d = the dense output with its bias; y stored: the backward's LayerNorm input),
//                                         out = LayerNorm(y)
//   !RESID (BertEmbeddings):              out = m o LayerNorm(x)
// Same launch count as the GEMM-with-residual + ufnd_layernorm pair it replaces.
template <int NI, bool RESID>
__global__ __launch_bounds__(256) void dropout_layernorm_kernel(const float* x, int ldx, const float* d, int ldd, const float* gamma,
                                                                const float* beta, float* y, __bf16* ob, float* of, int M, int H, float eps,
                                                                ufnd_dropout dr) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const uint64_t seed = dr.state->seed, step = dropout_step_key(dr.state);
  f32x4 v[NI], m[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int col = 4 * lane + 256 * i;
    float m4[4];
    dropout_mul4_ctr(seed, step, dr.p, dr.tag, (uint32_t)(((size_t)row * H + col) >> 2), m4);
    m[i] = f32x4{m4[0], m4[1], m4[2], m4[3]};
    v[i] = ld4(x + (size_t)row * ldx + col);
    if constexpr (RESID) {
      v[i] += m[i] * ld4(d + (size_t)row * ldd + col);
      *reinterpret_cast<f32x4*>(y + (size_t)row * H + col) = v[i];
    }
  }
  ln_row<NI>(v, H, eps, gamma, beta, lane);
  if constexpr (!RESID) {
#pragma unroll
    for (int i = 0; i < NI; ++i) v[i] *= m[i];
  }
  store_row<NI>(v, ob, of, row, H, lane);
}

template <int NI>
__global__ __launch_bounds__(256) void bert_embed_kernel(const int64_t* ids, const float* word, const float* pos,
                                                         const float* type0, const float* gamma, const float* beta,
                                                         __bf16* ob, float* of, int M, int L, int H, int vocab,
                                                         float eps, const int32_t* row_src, const int* m_live) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M || (m_live && row >= *m_live)) return;
  const int src = row_src ? row_src[row] : row;     // packed rows of ufnd_text_pack: the (B, L) index of the token
  long long id = ids[src];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);  // never read outside the table
  int l = src % L;
  l = l < 0 ? 0 : (l >= L ? L - 1 : l);
  f32x4 v[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int col = 4 * lane + 256 * i;
    v[i] = ld4(word + (size_t)id * H + col) + ld4(pos + (size_t)l * H + col) + ld4(type0 + col);
  }
  if (gamma) ln_row<NI>(v, H, eps, gamma, beta, lane);      // (gamma == NULL: the raw sums, for training forwards that keep them)
  store_row<NI>(v, ob, of, row, H, lane);
}

// masked mean over tokens (phase 1: grid (H/256, B), 256 threads = 4 token-groups x 64 lanes x 4 columns,
// LDS-reduced), then L2 normalise (phase 2, one block per sample).  text_blocks.py:82-86,100.
// PACKED (cu != NULL): sample b's positions 0 .. n_b - 1 are rows cu[b] .. cu[b+1] (ufnd_text_pack); the same groups, the same order.
template <bool PACKED>
__global__ __launch_bounds__(256) void meanpool_kernel(const float* hidden, const int32_t* mask, float* out, int L, int H, const int32_t* cu) {
  __shared__ f32x4 part[4][64];
  __shared__ float cnts[4];
  const int b = blockIdx.y, col = blockIdx.x * 256 + 4 * (threadIdx.x & 63), grp = threadIdx.x >> 6, lane = threadIdx.x & 63;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float cnt = 0.0f;
  const size_t r0 = PACKED ? (size_t)cu[b] : (size_t)b * L;
  const int n = PACKED ? cu[b + 1] - cu[b] : L;      // rows of the sample (positions past them are masked)
  // eight tokens of the group per pass: their mask words and rows are requested together (a mask load -> branch -> row
  // load chain per token made this kernel 27 us for 12.6 MB); rows are added in token order, only where the mask keeps them
  for (int l0 = grp; l0 < n; l0 += 32) {
    int mk[8];
    f32x4 x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int l = l0 + 4 * u;
      mk[u] = l < n ? mask[(size_t)b * L + l] : 0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int l = l0 + 4 * u < n ? l0 + 4 * u : n - 1;
      x[u] = ld4(hidden + (r0 + l) * H + col);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (mk[u] != 0) {
        acc += x[u];
        cnt += 1.0f;
      }
    }
  }
  part[grp][lane] = acc;
  if (lane == 0) cnts[grp] = cnt;
  __syncthreads();
  if (grp == 0) {
    const f32x4 s = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
    const float denom = fmaxf((cnts[0] + cnts[1]) + (cnts[2] + cnts[3]), 1e-6f);
    *reinterpret_cast<f32x4*>(out + (size_t)b * H + col) = s / denom;
  }
}
// LayerNorm + the masked mean of the packed pass in one kernel: layernorm_kernel's rows never reach memory.  One workgroup per
// sample; wave g normalises the sample's tokens g, g + 4, ... (a whole row per wave, ln_row: layernorm_kernel's arithmetic) and
// adds them in that order where the mask keeps them -- meanpool_kernel<true>'s groups, order and (p0 + p1) + (p2 + p3)
// combination, so the mean is bit-identical to the two launches'.  Eight rows of a wave are requested and normalised together.
template <int NI>
__global__ __launch_bounds__(256) void ln_meanpool_kernel(const float* y, const float* gamma, const float* beta, float eps, const int32_t* mask,
                                                          const int32_t* cu, float* out, int L, int H) {
  __shared__ f32x4 part[4][NI][64];
  __shared__ float cnts[4];
  const int b = blockIdx.x, grp = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const size_t r0 = (size_t)cu[b];
  const int n = cu[b + 1] - cu[b];      // rows of the sample (positions past them are masked)
  f32x4 acc[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float cnt = 0.0f;
  for (int l0 = grp; l0 < n; l0 += 32) {
    int mk[8];
    f32x4 v[8][NI];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int l = l0 + 4 * u;
      mk[u] = l < n ? mask[(size_t)b * L + l] : 0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int l = l0 + 4 * u < n ? l0 + 4 * u : n - 1;
#pragma unroll
      for (int i = 0; i < NI; ++i) v[u][i] = ld4(y + (r0 + l) * H + 4 * lane + 256 * i);
    }
    // every requested row is normalised, kept or not (a row past the sample is its last row again): eight independent reduction
    // chains the scheduler may interleave, where a branch per row would run them one after the other
#pragma unroll
    for (int u = 0; u < 8; ++u) ln_row<NI>(v[u], H, eps, gamma, beta, lane);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (mk[u] != 0) {      // (wave-uniform: one mask word per row)
#pragma unroll
        for (int i = 0; i < NI; ++i) acc[i] += v[u][i];
        cnt += 1.0f;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) part[grp][i][lane] = acc[i];
  if (lane == 0) cnts[grp] = cnt;
  __syncthreads();
  if (grp == 0) {
    const float denom = fmaxf((cnts[0] + cnts[1]) + (cnts[2] + cnts[3]), 1e-6f);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const f32x4 s = (part[0][i][lane] + part[1][i][lane]) + (part[2][i][lane] + part[3][i][lane]);
      *reinterpret_cast<f32x4*>(out + (size_t)b * H + 4 * lane + 256 * i) = s / denom;
    }
  }
}

// ufnd_text_pack: one workgroup.  n_b = 1 + the last kept position of sample b (0 for an all-masked sample); cu = exclusive prefix sum
// of n_b (cu[B] = the live row count); row_src[cu[b] + l] = b L + l for l < n_b.
// Slot bins (bins != NULL, L <= 128): sample b takes c_b = ceil(n_b / 32) contiguous 32-row slots of one 4-slot bin
// (ufnd_qkv_attention_bf16_bins: a bin is one workgroup's 128 tile rows).  Bins, in this order:
//   full:    [4-slot sample], [3-slot + 1-slot] (pairs by rank), [2 + 2], [the odd 2-slot + two 1-slot] (if full), [1 x 4];
//   partial: [3-slot alone] (3-slot samples beyond the 1-slot count), [the odd 2-slot (+ one 1-slot)], [the last 1-3 1-slot];
// every bin fills its slots from slot 0 on, samples in ascending order within a class.  This is an optimal packing (no bin
// count is lower) and a function of the n_b alone.  Bin i is 8 ints: slot j's {cu[b] + 32 s, (b << 10) | (s << 8) | n_b} for
// slot s of sample b, {0, -1} if empty; *nbins = the bin count (0 when every sample is all-masked).
// (the slot bins, by every thread of the pack workgroup after pack_scan_rows: lens[b] = cu[b], total = cu[B])
__device__ __forceinline__ void pack_slot_bins(const int* lens, int total, int B, int32_t* bins, int32_t* nbins) {
  __shared__ long long csum[PACK_THREADS / 64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int per = (B + PACK_THREADS - 1) / PACK_THREADS, b0 = tid * per, b1 = min(b0 + per, B);      // the scan's samples of this thread
  // ranks within the slot classes: four 16-bit counters in one 64-bit scan (counts <= PACK_MAX_B < 2^16)
  auto nrows = [&](int b) { return (b + 1 < B ? lens[b + 1] : total) - lens[b]; };
  long long cown = 0;
  for (int b = b0; b < b1; ++b) {
    const int c = (nrows(b) + 31) >> 5;
    if (c > 0) cown += 1ll << (16 * (c - 1));
  }
  long long cinc = cown;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long y = __shfl_up(cinc, o, 64);
    if (lane >= o) cinc += y;
  }
  if (lane == 63) csum[wave] = cinc;
  __syncthreads();
  long long cbase = 0, call = 0;
  for (int w = 0; w < PACK_THREADS / 64; ++w) {
    if (w < wave) cbase += csum[w];
    call += csum[w];
  }
  auto field = [](long long v, int c) { return (int)((v >> (16 * (c - 1))) & 0xffff); };
  const int n1 = field(call, 1), n2 = field(call, 2), n3 = field(call, 3), n4 = field(call, 4);
  const int p = min(n1, n3), r1 = n1 - p, h = n2 >> 1, t = n2 & 1, u = t ? min(2, r1) : 0;
  const bool odd_full = t && u == 2;
  const int f1 = (r1 - u) >> 2, rem1 = (r1 - u) & 3;
  const int b31 = n4, b22 = b31 + p, b211 = b22 + h, b1111 = b211 + (odd_full ? 1 : 0);
  const int bp3 = b1111 + f1, bp2 = bp3 + (n3 - p), bp1 = bp2 + ((t && !odd_full) ? 1 : 0), nb = bp1 + (rem1 ? 1 : 0);
  const int bodd = odd_full ? b211 : bp2;
  long long rank = cbase + cinc - cown;      // ranks of my first sample in each class
  for (int b = b0; b < b1; ++b) {
    const int n = nrows(b), c = (n + 31) >> 5;
    if (c == 0) continue;
    const int k = field(rank, c);
    rank += 1ll << (16 * (c - 1));
    int bin, s0;
    if (c == 4) {
      bin = k, s0 = 0;
    } else if (c == 3) {
      bin = k < p ? b31 + k : bp3 + (k - p), s0 = 0;
    } else if (c == 2) {
      bin = k < 2 * h ? b22 + (k >> 1) : bodd, s0 = k < 2 * h ? 2 * (k & 1) : 0;
    } else if (k < p) {
      bin = b31 + k, s0 = 3;
    } else if (k - p < u) {
      bin = bodd, s0 = 2 + (k - p);
    } else {
      const int k1 = k - p - u;
      bin = (k1 >> 2) < f1 ? b1111 + (k1 >> 2) : bp1, s0 = k1 & 3;
    }
    for (int s = 0; s < c; ++s) {
      bins[(size_t)bin * 8 + 2 * (s0 + s)] = lens[b] + 32 * s;
      bins[(size_t)bin * 8 + 2 * (s0 + s) + 1] = (b << 10) | (s << 8) | n;
    }
  }
  // the empty slots of the partial bins (no sample writes them)
  for (int i = bp3 + tid; i < nb; i += PACK_THREADS) {
    const int used = i < bp2 ? 3 : (i < bp1 ? 2 + u : rem1);
    for (int j = used; j < 4; ++j) {
      bins[(size_t)i * 8 + 2 * j] = 0;
      bins[(size_t)i * 8 + 2 * j + 1] = -1;
    }
  }
  if (tid == 0) *nbins = nb;
}

__global__ __launch_bounds__(PACK_THREADS) void text_pack_kernel(const int32_t* mask, int B, int L, int32_t* cu, int32_t* row_src,
                                                                 int32_t* bins, int32_t* nbins) {
  __shared__ int lens[PACK_MAX_B];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int b = wave; b < B; b += PACK_THREADS / 64) {      // a wave per sample: the largest kept position + 1
    int last = 0;
    for (int l = lane; l < L; l += 64) last = mask[(size_t)b * L + l] != 0 ? l + 1 : last;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) last = max(last, __shfl_xor(last, o, 64));
    if (lane == 0) lens[b] = last;
  }
  const int total = pack_scan_rows(lens, B, L, cu, row_src);      // (rowwise.hpp: cu, row_src; lens[b] = cu[b])
  if (bins) pack_slot_bins(lens, total, B, bins, nbins);
}

// ufnd_text_pack_tiles: ufnd_text_pack + the sample tiles of ufnd_qkv_attention_bf16_tiles (the table's layout: ultrafnd_hip.h).  Whole
// samples, back to back, in 256-row tiles by first-fit-decreasing: samples in descending n_b (ties: ascending b) each go to the first
// tile with n_b free rows and fewer than TILE_CAP samples.  Any two samples fit one tile, so first fit leaves at most one tile with a
// single sample: (B + 1) / 2 tiles always suffice.  The rank of a sample is counted (B <= 512: B comparisons per thread); wave 0 then
// places the samples in rank order with the tiles' free rows and sample counts in registers -- tile 64 c + lane in element c of its
// lanes -- one ballot per sample; the other threads then write the descriptors, the row map and the key biases, a thread per tile its
// unit list.  bins != NULL: the slot bins as well.
constexpr int TILE_MAX_B = UFND_TEXT_TILE_MAX_B, TILE_CAP = UFND_TEXT_TILE_SAMPLES, TILE_INTS = UFND_TEXT_TILE_INTS, TILE_MAX = TILE_MAX_B / 2;
__global__ __launch_bounds__(PACK_THREADS) void text_pack_tiles_kernel(const int32_t* mask, int B, int L, int32_t* cu, int32_t* row_src,
                                                                       int32_t* tiles, int32_t* ntiles, int32_t* bins, int32_t* nbins) {
  __shared__ int lens[TILE_MAX_B], order[TILE_MAX_B], place[TILE_MAX_B];
  __shared__ __attribute__((aligned(16))) int nb[TILE_MAX_B];      // n_b (0 past B: the rank loop reads whole groups of four)
  __shared__ int t_rows[TILE_MAX], t_cnt[TILE_MAX], t_cu0[TILE_MAX];
  __shared__ unsigned char t_n[TILE_MAX * TILE_CAP];
  __shared__ unsigned long long kept[TILE_MAX_B][2];      // the mask row of sample b as bits (positions 0-63, 64-127)
  __shared__ int nlive_s, nt_s;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (tid == 0) nlive_s = 0;
  if (tid >= B && tid < TILE_MAX_B) nb[tid] = 0;
  // a wave per sample, four samples' loads in flight: the mask row as two ballots, n_b = the largest kept position + 1
  constexpr int NWV = PACK_THREADS / 64;
  for (int b0 = wave; b0 < B; b0 += 4 * NWV) {
    int v[4][2];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int b = b0 + NWV * j, l = lane + 64 * h;
        v[j][h] = (b < B && l < L) ? mask[(size_t)b * L + l] : 0;
      }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int b = b0 + NWV * j;
      if (b >= B) break;
      const unsigned long long m0 = __ballot(v[j][0] != 0), m1 = __ballot(v[j][1] != 0);
      const int last = m1 ? 128 - __clzll((long long)m1) : (m0 ? 64 - __clzll((long long)m0) : 0);
      if (lane == 0) {
        lens[b] = last;
        nb[b] = last;
        kept[b][0] = m0;
        kept[b][1] = m1;
      }
    }
  }
  const int total = pack_scan_rows(lens, B, L, cu, row_src);      // (rowwise.hpp: cu, row_src; lens[b] = cu[b]; barriers inside)
  if (bins) pack_slot_bins(lens, total, B, bins, nbins);          // (ufnd_text_pack_bins' table too, where the caller keeps both current)
  if (tid < B && nb[tid] > 0) {                 // rank in descending n_b, ties in ascending b
    const int n = nb[tid];
    int rank = 0;
#pragma unroll 4
    for (int b = 0; b < B; b += 4) {
      const int4 v = *reinterpret_cast<const int4*>(nb + b);
      rank += (v.x > n || (v.x == n && b < tid)) + (v.y > n || (v.y == n && b + 1 < tid)) + (v.z > n || (v.z == n && b + 2 < tid)) +
              (v.w > n || (v.w == n && b + 3 < tid));
    }
    order[rank] = tid;
    atomicAdd(&nlive_s, 1);
  }
  __syncthreads();
  const int nl = nlive_s;
  if (wave == 0) {
    // st[c] of a lane: tile 64 c + lane's (samples << 16) | rows used; key[c]: its free rows, -1 once it holds TILE_CAP samples
    int st[TILE_MAX / 64], key[TILE_MAX / 64];
#pragma unroll
    for (int c = 0; c < TILE_MAX / 64; ++c) { st[c] = 0; key[c] = 256; }
    // up to 128 samples need at most 64 tiles, so every sample finds its tile in chunk 0: one short dependent chain per sample (ballot,
    // first set bit, the chosen lane's update), which is what this kernel's duration is made of (about 0.1 us a sample)
    for (int i0 = 0; nl <= 128 && i0 < nl; i0 += 64) {
      const int vn = i0 + lane < nl ? nb[order[i0 + lane]] : 0;
      const int cnt = min(64, nl - i0);
      int s0 = st[0], k0 = key[0];
      for (int j = 0; j < cnt; ++j) {
        const int n = __builtin_amdgcn_readlane(vn, j);
        const bool mine = lane == __ffsll((long long)__ballot(k0 >= n)) - 1;
        if (mine) place[i0 + j] = (lane << 12) | ((s0 >> 16) << 8) | (s0 & 0xffff);
        s0 += mine ? (1 << 16) + n : 0;
        k0 = s0 < (TILE_CAP << 16) ? 256 - (s0 & 0xffff) : -1;
      }
      st[0] = s0;
      key[0] = k0;
    }
    for (int i0 = 0; nl > 128 && i0 < nl; i0 += 64) {
      const int vn = i0 + lane < nl ? nb[order[i0 + lane]] : 0;
      const int cnt = min(64, nl - i0);
      int pv = 0;      // lane j: where sample i0 + j went, (tile << 12) | (slot << 8) | its first tile row
      // (no LDS traffic inside: the loop is one dependent chain per sample -- ballot, first set bit, the chosen lane's update -- and the
      //  placements collect in pv, lane j's for sample i0 + j)
      for (int j = 0; j < cnt; ++j) {
        const int n = __builtin_amdgcn_readlane(vn, j);
        bool placed = false;
#pragma unroll
        for (int c = 0; c < TILE_MAX / 64; ++c) {      // (the first 64 tiles take 128 samples or more: the later chunks are rarely reached)
          const unsigned long long m = placed ? 0ull : __ballot(key[c] >= n);
          if (m == 0) continue;
          const int l = __ffsll((long long)m) - 1;
          const int was = __builtin_amdgcn_readlane(st[c], l);
          pv = lane == j ? ((64 * c + l) << 12) | ((was >> 16) << 8) | (was & 0xffff) : pv;
          st[c] += lane == l ? (1 << 16) + n : 0;
          key[c] = st[c] < (TILE_CAP << 16) ? 256 - (st[c] & 0xffff) : -1;
          placed = true;
        }
      }
      if (i0 + lane < nl) place[i0 + lane] = pv;
    }
    int nt = 0;
#pragma unroll
    for (int c = 0; c < TILE_MAX / 64; ++c) {
      nt += __popcll(__ballot(st[c] != 0));
      t_rows[64 * c + lane] = st[c] & 0xffff;
      t_cnt[64 * c + lane] = st[c] >> 16;
    }
    if (lane == 0) {
      nt_s = nt;
      *ntiles = nt;
    }
  }
  __syncthreads();
  const int nt = nt_s;
  if (tid < nl) {      // the descriptor of the sample of rank tid
    const int b = order[tid], p = place[tid], t = p >> 12, slot = (p >> 8) & 15, r0 = p & 255;
    tiles[(size_t)t * TILE_INTS + 4 + 2 * slot] = lens[b];
    tiles[(size_t)t * TILE_INTS + 5 + 2 * slot] = (b << 16) | (r0 << 8) | nb[b];
    t_n[t * TILE_CAP + slot] = (unsigned char)nb[b];
    if (slot == 0) t_cu0[t] = lens[b];
  }
  for (int i = wave; i < nl; i += NWV) {      // a wave per sample: row map and key biases of its rows
    const int b = order[i], n = nb[b], p = place[i], r0 = p & 255, row0 = lens[b];
    int32_t* td = tiles + (size_t)(p >> 12) * TILE_INTS;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = lane + 64 * h;
      if (k >= n) continue;
      td[UFND_TEXT_TILE_ROWMAP + r0 + k] = row0 + k;
      td[UFND_TEXT_TILE_KBIAS + r0 + k] = __float_as_int(((kept[b][h] >> lane) & 1) ? 0.0f : -3.0e38f);
    }
  }
  __syncthreads();      // (t_n, t_cu0: written by the samples' threads, read by the tiles')
  if (tid < nt) {      // header and unit list of tile tid
    int32_t* td = tiles + (size_t)tid * TILE_INTS;
    const int cnt = t_cnt[tid];
    int u = 0;
    for (int j = 0; j < cnt; ++j)
      for (int q = 0; q < (t_n[tid * TILE_CAP + j] + 31) >> 5; ++q) td[UFND_TEXT_TILE_UNIT0 + u++] = j | (q << 8);
    td[0] = cnt;
    td[1] = t_rows[tid];
    td[2] = u;
    td[3] = 0;
  }
  for (int idx = tid; idx < nt * 256; idx += PACK_THREADS) {      // rows past a tile's live ones: its first row, masked
    const int t = idx >> 8, r = idx & 255;
    if (r < t_rows[t]) continue;
    tiles[(size_t)t * TILE_INTS + UFND_TEXT_TILE_ROWMAP + r] = t_cu0[t];
    tiles[(size_t)t * TILE_INTS + UFND_TEXT_TILE_KBIAS + r] = __float_as_int(-3.0e38f);
  }
}

__global__ __launch_bounds__(256) void l2norm_rows_kernel(float* x, int H) {
  __shared__ float sh[4];
  float* row = x + (size_t)blockIdx.x * H;
  float sq = 0.0f;
  for (int c = threadIdx.x; c < H; c += 256) sq += row[c] * row[c];
  sq = wave_sum(sq);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = sq;
  __syncthreads();
  const float nrm = sqrtf((sh[0] + sh[1]) + (sh[2] + sh[3])) + 1e-9f;
  for (int c = threadIdx.x; c < H; c += 256) row[c] = row[c] / nrm;
}

// frames (N,3,S,S) fp32 -> patches (N*G*G, 3*P*P) bf16, element order (c, ky, kx).
// One workgroup per (frame, patch row py): its threads walk the 3 x P image rows of that band in order, 8 pixels (32 B in, 16 B
// out) per thread and step, so the reads are whole contiguous image rows and the index arithmetic is 32-bit with compile-time
// divisors (PT = patch size, GT = patches per row; 0 = run-time values).  The first version spent its time in 64-bit div / mod
// per four pixels: 45 us for 115 MB (2.6 TB/s).
template <int PT, int GT>
__global__ __launch_bounds__(256) void patchify_kernel(const float* frames, __bf16* patches, int S_, int P_) {
  const int P = PT ? PT : P_, G = GT ? GT : S_ / P_, S = P * G;
  const int n = blockIdx.x / G, py = blockIdx.x - n * G;
  const int K = 3 * P * P, CPR = P / 8;              // 8-pixel chunks per patch row
  const int chunks = 3 * P * G * CPR;                // of this band
  const float* src = frames + ((size_t)n * 3 * S + (size_t)py * P) * S;       // + (c * S + ky) * S + px * P + kx
  __bf16* dst = patches + ((size_t)n * G * G + (size_t)py * G) * K;           // + px * K + c * P * P + ky * P + kx
  for (int q = threadIdx.x; q < chunks; q += 256) {
    const int x8 = q % (G * CPR), r = q / (G * CPR);      // chunk inside the image row; image row of the band (c, ky)
    const int ky = r % P, c = r / P;
    const int px = x8 / CPR, kx = (x8 - px * CPR) * 8;
    const float* sp = src + ((size_t)c * S + ky) * S + x8 * 8;
    const f32x4 v0 = ld4(sp), v1 = ld4(sp + 4);
    bf16x8 o = {(__bf16)v0[0], (__bf16)v0[1], (__bf16)v0[2], (__bf16)v0[3], (__bf16)v1[0], (__bf16)v1[1], (__bf16)v1[2], (__bf16)v1[3]};
    *reinterpret_cast<bf16x8*>(dst + (size_t)px * K + c * P * P + ky * P + kx) = o;
  }
}

// x[n][0] = cls + pos[0]; x[n][1+p] = patch_emb[n*P+p] + pos[1+p]; then pre-LayerNorm
template <int NI>
__global__ __launch_bounds__(256) void vit_assemble_kernel(const float* pe, const float* cls, const float* pos,
                                                           const float* gamma, const float* beta, float* of, __bf16* ob,
                                                           float* stats, int M, int P, int H, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int n = row / (P + 1), t = row % (P + 1);
  f32x4 v[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int col = 4 * lane + 256 * i;
    const f32x4 base = (t == 0) ? ld4(cls + col) : ld4(pe + ((size_t)n * P + (t - 1)) * H + col);
    v[i] = base + ld4(pos + (size_t)t * H + col);
  }
  if (gamma) ln_row<NI>(v, H, eps, gamma, beta, lane);      // (gamma == NULL: the raw sums)
  store_row<NI>(v, ob, of, row, H, lane);
  if (stats) row_stats<NI>(v, stats, row, lane);
}

// per-frame L2 normalise, mean over frames, L2 normalise again (F > 1); one block per sample
__global__ __launch_bounds__(256) void l2norm_frames_kernel(const float* e, float* out, int F, int D) {
  __shared__ float sh[4];
  const int b = blockIdx.x;
  float acc[4] = {0, 0, 0, 0};
  for (int f = 0; f < F; ++f) {
    const float* row = e + ((size_t)b * F + f) * D;
    float sq = 0.0f;
    for (int c = threadIdx.x; c < D; c += 256) sq += row[c] * row[c];
    const float nrm = sqrtf(block_sum4(sq, sh)) + 1e-9f;
    int n = 0;
    for (int c = threadIdx.x; c < D; c += 256, ++n) acc[n] += row[c] / nrm;
  }
  if (F == 1) {
    int n = 0;
    for (int c = threadIdx.x; c < D; c += 256, ++n) out[(size_t)b * D + c] = acc[n];
    return;
  }
  float sq = 0.0f;
  int n = 0;
  for (int c = threadIdx.x; c < D; c += 256, ++n) {
    acc[n] /= (float)F;
    sq += acc[n] * acc[n];
  }
  const float nrm = sqrtf(block_sum4(sq, sh)) + 1e-9f;
  n = 0;
  for (int c = threadIdx.x; c < D; c += 256, ++n) out[(size_t)b * D + c] = acc[n] / nrm;
}

// encode_fields (text_blocks.py:108-128): mean of the VALID part vectors of a record, then
// v / (||v|| + 1e-9); a record without parts yields the zero vector.  One block per record.
__global__ __launch_bounds__(256) void field_mean_l2_kernel(const float* parts, const int32_t* valid, float* out, int Mx,
                                                            int D) {
  __shared__ float sh[4];
  const int n = blockIdx.x;
  float acc[4] = {0, 0, 0, 0};
  int cnt = 0;
  for (int m = 0; m < Mx; ++m) {
    if (valid[(size_t)n * Mx + m] == 0) continue;
    ++cnt;
    const float* row = parts + ((size_t)n * Mx + m) * D;
    int k = 0;
    for (int c = threadIdx.x; c < D; c += 256, ++k) acc[k] += row[c];
  }
  float sq = 0.0f;
  int k = 0;
  for (int c = threadIdx.x; c < D; c += 256, ++k) {
    acc[k] = cnt ? acc[k] / (float)cnt : 0.0f;
    sq += acc[k] * acc[k];
  }
  sq = wave_sum(sq);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = sq;
  __syncthreads();
  const float nrm = sqrtf((sh[0] + sh[1]) + (sh[2] + sh[3])) + 1e-9f;
  k = 0;
  for (int c = threadIdx.x; c < D; c += 256, ++k) out[(size_t)n * D + c] = cnt ? acc[k] / nrm : 0.0f;
}

}  // namespace

extern "C" int ufnd_layernorm(const float* x, int ldx, const float* gamma, const float* beta, void* out_bf16,
                              float* out_f32, int M, int H, float eps, void* stream_) {
  UFND_REQUIRE(x && gamma && beta && (out_bf16 || out_f32) && M >= 1, "layernorm: null argument");
  UFND_REQUIRE(h_ok(H), "layernorm: H=%d (supported 256/512/768/1024)", H);
  UFND_REQUIRE(ldx % 4 == 0 && ldx >= H && ufnd_aligned(x, 16) && ufnd_aligned(gamma, 16) && ufnd_aligned(beta, 16) &&
                   (!out_f32 || ufnd_aligned(out_f32, 16)) && (!out_bf16 || ufnd_aligned(out_bf16, 8)), "layernorm: alignment");
  NI_LAUNCH(H, layernorm_kernel, dim3(ufnd_cdiv(M, 4)), (hipStream_t)stream_, x, ldx, gamma, beta, (__bf16*)out_bf16,
            out_f32, M, H, eps, (const int*)nullptr);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_dropout_residual_layernorm(const float* x, int ldx, const float* d, int ldd, const float* gamma, const float* beta, float* y,
                                               void* out_bf16, float* out_f32, int M, int H, float eps, const ufnd_dropout* drop, void* stream_) {
  UFND_REQUIRE(x && d && gamma && beta && y && (out_bf16 || out_f32) && M >= 1 && drop && drop->state, "dropout_residual_layernorm: null argument");
  UFND_REQUIRE(drop->p > 0.0f && drop->p < 1.0f, "dropout_residual_layernorm: p=%g (0 < p < 1)", (double)drop->p);
  UFND_REQUIRE(h_ok(H), "dropout_residual_layernorm: H=%d (supported 256/512/768/1024)", H);
  UFND_REQUIRE(ldx % 4 == 0 && ldx >= H && ldd % 4 == 0 && ldd >= H && ufnd_aligned(x, 16) && ufnd_aligned(d, 16) && ufnd_aligned(y, 16) &&
                   ufnd_aligned(gamma, 16) && ufnd_aligned(beta, 16) && (!out_f32 || ufnd_aligned(out_f32, 16)) && (!out_bf16 || ufnd_aligned(out_bf16, 8)),
               "dropout_residual_layernorm: alignment");
  UFND_REQUIRE((long long)M * H / 4 <= (1ll << 32), "dropout_residual_layernorm: M=%d H=%d overflows the 32-bit dropout counter", M, H);
  NI_LAUNCH_T(H, dropout_layernorm_kernel, true, dim3(ufnd_cdiv(M, 4)), (hipStream_t)stream_, x, ldx, d, ldd, gamma, beta, y, (__bf16*)out_bf16,
            out_f32, M, H, eps, *drop);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_layernorm_dropout(const float* x, int ldx, const float* gamma, const float* beta, void* out_bf16, float* out_f32, int M, int H,
                                      float eps, const ufnd_dropout* drop, void* stream_) {
  UFND_REQUIRE(x && gamma && beta && (out_bf16 || out_f32) && M >= 1 && drop && drop->state, "layernorm_dropout: null argument");
  UFND_REQUIRE(drop->p > 0.0f && drop->p < 1.0f, "layernorm_dropout: p=%g (0 < p < 1)", (double)drop->p);
  UFND_REQUIRE(h_ok(H), "layernorm_dropout: H=%d (supported 256/512/768/1024)", H);
  UFND_REQUIRE(ldx % 4 == 0 && ldx >= H && ufnd_aligned(x, 16) && ufnd_aligned(gamma, 16) && ufnd_aligned(beta, 16) &&
                   (!out_f32 || ufnd_aligned(out_f32, 16)) && (!out_bf16 || ufnd_aligned(out_bf16, 8)), "layernorm_dropout: alignment");
  UFND_REQUIRE((long long)M * H / 4 <= (1ll << 32), "layernorm_dropout: M=%d H=%d overflows the 32-bit dropout counter", M, H);
  NI_LAUNCH_T(H, dropout_layernorm_kernel, false, dim3(ufnd_cdiv(M, 4)), (hipStream_t)stream_, x, ldx, (const float*)nullptr, 0, gamma, beta,
            (float*)nullptr, (__bf16*)out_bf16, out_f32, M, H, eps, *drop);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_bert_embed(const int64_t* ids, const float* word, const float* pos, const float* type0,
                               const float* gamma, const float* beta, void* x_bf16, float* x_f32, int B, int L, int H,
                               int vocab, float eps, void* stream_) {
  UFND_REQUIRE(ids && word && pos && type0 && ((gamma && beta) || (!gamma && !beta)) && (x_bf16 || x_f32), "bert_embed: null argument");
  UFND_REQUIRE(h_ok(H) && B >= 1 && L >= 1 && vocab >= 1, "bert_embed: B=%d L=%d H=%d vocab=%d", B, L, H, vocab);
  UFND_REQUIRE(ufnd_aligned(word, 16) && ufnd_aligned(pos, 16) && ufnd_aligned(type0, 16) &&
                   (!x_f32 || ufnd_aligned(x_f32, 16)) && (!x_bf16 || ufnd_aligned(x_bf16, 8)), "bert_embed: alignment");
  const int M = B * L;
  NI_LAUNCH(H, bert_embed_kernel, dim3(ufnd_cdiv(M, 4)), (hipStream_t)stream_, ids, word, pos, type0, gamma, beta,
            (__bf16*)x_bf16, x_f32, M, L, H, vocab, eps, (const int32_t*)nullptr, (const int*)nullptr);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

// the first phase alone: the masked mean, no L2 (the audio encoder's out.mean(dim=1) over a clip's valid frames)
extern "C" int ufnd_masked_meanpool(const float* hidden, const int32_t* mask, float* out, int B, int L, int H, void* stream_) {
  UFND_REQUIRE(hidden && mask && out, "meanpool: null argument");
  UFND_REQUIRE(B >= 1 && B <= 65535 && L >= 1, "meanpool: B=%d L=%d (1 <= B <= 65535 clips, L >= 1 rows)", B, L);
  UFND_REQUIRE(H >= 256 && H % 256 == 0 && ufnd_aligned(hidden, 16) && ufnd_aligned(out, 16), "meanpool: H=%d (multiple of 256)", H);
  hipLaunchKernelGGL(meanpool_kernel<false>, dim3(H / 256, B), dim3(256), 0, (hipStream_t)stream_, hidden, mask, out, L, H,
                     (const int32_t*)nullptr);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_masked_meanpool_l2(const float* hidden, const int32_t* mask, float* out, int B, int L, int H,
                                       void* stream_) {
  UFND_REQUIRE(hidden && mask && out && B >= 1 && L >= 1, "meanpool: null argument");
  UFND_REQUIRE(H >= 256 && H % 256 == 0 && ufnd_aligned(hidden, 16) && ufnd_aligned(out, 16), "meanpool: H=%d (multiple of 256)", H);
  hipLaunchKernelGGL(meanpool_kernel<false>, dim3(H / 256, B), dim3(256), 0, (hipStream_t)stream_, hidden, mask, out, L, H,
                     (const int32_t*)nullptr);
  UFND_CHECK_LAUNCH();
  hipLaunchKernelGGL(l2norm_rows_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream_, out, H);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_text_pack(const int32_t* mask, int B, int L, int32_t* cu_seqlens, int32_t* row_src, void* stream_) {
  UFND_REQUIRE(mask && cu_seqlens && row_src, "text_pack: null argument");
  UFND_REQUIRE(B >= 1 && B <= PACK_MAX_B && L >= 1 && (long long)B * L < (1ll << 31), "text_pack: B=%d L=%d (B <= %d)", B, L, PACK_MAX_B);
  hipLaunchKernelGGL(text_pack_kernel, dim3(1), dim3(PACK_THREADS), 0, (hipStream_t)stream_, mask, B, L, cu_seqlens, row_src,
                     (int32_t*)nullptr, (int32_t*)nullptr);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_text_pack_bins(const int32_t* mask, int B, int L, int32_t* cu_seqlens, int32_t* row_src, int32_t* bins,
                                   int32_t* nbins, void* stream_) {
  UFND_REQUIRE(mask && cu_seqlens && row_src && bins && nbins, "text_pack_bins: null argument");
  UFND_REQUIRE(B >= 1 && B <= PACK_MAX_B && L >= 1 && L <= 128, "text_pack_bins: B=%d L=%d (B <= %d, L <= 128)", B, L, PACK_MAX_B);
  hipLaunchKernelGGL(text_pack_kernel, dim3(1), dim3(PACK_THREADS), 0, (hipStream_t)stream_, mask, B, L, cu_seqlens, row_src, bins, nbins);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_text_pack_tiles(const int32_t* mask, int B, int L, int32_t* cu_seqlens, int32_t* row_src, int32_t* tiles,
                                    int32_t* ntiles, int32_t* bins, int32_t* nbins, void* stream_) {
  UFND_REQUIRE(mask && cu_seqlens && row_src && tiles && ntiles && !bins == !nbins, "text_pack_tiles: null argument");
  UFND_REQUIRE(B >= 1 && B <= TILE_MAX_B && L >= 1 && L <= 128, "text_pack_tiles: B=%d L=%d (B <= %d, L <= 128)", B, L, TILE_MAX_B);
  hipLaunchKernelGGL(text_pack_tiles_kernel, dim3(1), dim3(PACK_THREADS), 0, (hipStream_t)stream_, mask, B, L, cu_seqlens, row_src, tiles, ntiles,
                     bins, nbins);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_bert_embed_live(const int64_t* ids, const int32_t* row_src, const int* m_live, const float* word, const float* pos,
                                    const float* type0, const float* gamma, const float* beta, void* x_bf16, float* x_f32, int capacity,
                                    int L, int H, int vocab, float eps, void* stream_) {
  UFND_REQUIRE(ids && row_src && m_live && word && pos && type0 && gamma && beta && (x_bf16 || x_f32), "bert_embed_live: null argument");
  UFND_REQUIRE(h_ok(H) && capacity >= 1 && L >= 1 && vocab >= 1, "bert_embed_live: capacity=%d L=%d H=%d vocab=%d", capacity, L, H, vocab);
  UFND_REQUIRE(ufnd_aligned(word, 16) && ufnd_aligned(pos, 16) && ufnd_aligned(type0, 16) &&
                   (!x_f32 || ufnd_aligned(x_f32, 16)) && (!x_bf16 || ufnd_aligned(x_bf16, 8)), "bert_embed_live: alignment");
  NI_LAUNCH(H, bert_embed_kernel, dim3(ufnd_cdiv(capacity, 4)), (hipStream_t)stream_, ids, word, pos, type0, gamma, beta,
            (__bf16*)x_bf16, x_f32, capacity, L, H, vocab, eps, row_src, m_live);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_layernorm_live(const float* x, int ldx, const float* gamma, const float* beta, void* out_bf16, float* out_f32,
                                   int capacity, int H, float eps, const int* m_live, void* stream_) {
  UFND_REQUIRE(x && gamma && beta && (out_bf16 || out_f32) && m_live && capacity >= 1, "layernorm_live: null argument");
  UFND_REQUIRE(h_ok(H), "layernorm_live: H=%d (supported 256/512/768/1024)", H);
  UFND_REQUIRE(ldx % 4 == 0 && ldx >= H && ufnd_aligned(x, 16) && ufnd_aligned(gamma, 16) && ufnd_aligned(beta, 16) &&
                   (!out_f32 || ufnd_aligned(out_f32, 16)) && (!out_bf16 || ufnd_aligned(out_bf16, 8)), "layernorm_live: alignment");
  NI_LAUNCH(H, layernorm_kernel, dim3(ufnd_cdiv(capacity, 4)), (hipStream_t)stream_, x, ldx, gamma, beta, (__bf16*)out_bf16,
            out_f32, capacity, H, eps, m_live);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_masked_meanpool_l2_live(const float* hidden, const int32_t* mask, const int32_t* cu_seqlens, float* out, int B, int L,
                                            int H, void* stream_) {
  UFND_REQUIRE(hidden && mask && cu_seqlens && out && B >= 1 && L >= 1, "meanpool_live: null argument");
  UFND_REQUIRE(H >= 256 && H % 256 == 0 && ufnd_aligned(hidden, 16) && ufnd_aligned(out, 16), "meanpool_live: H=%d (multiple of 256)", H);
  hipLaunchKernelGGL(meanpool_kernel<true>, dim3(H / 256, B), dim3(256), 0, (hipStream_t)stream_, hidden, mask, out, L, H, cu_seqlens);
  UFND_CHECK_LAUNCH();
  hipLaunchKernelGGL(l2norm_rows_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream_, out, H);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

// ufnd_layernorm_live (fp32 output) + ufnd_masked_meanpool_l2_live in two launches instead of three, without the (capacity, H)
// buffer between them: bit-identical features (ln_meanpool_kernel)
extern "C" int ufnd_ln_masked_meanpool_l2_live(const float* y, const float* gamma, const float* beta, float eps, const int32_t* mask,
                                               const int32_t* cu_seqlens, float* out, int B, int L, int H, void* stream_) {
  UFND_REQUIRE(y && gamma && beta && mask && cu_seqlens && out && B >= 1 && L >= 1, "ln_meanpool_live: null argument");
  UFND_REQUIRE(h_ok(H), "ln_meanpool_live: H=%d (supported 256/512/768/1024)", H);
  UFND_REQUIRE(ufnd_aligned(y, 16) && ufnd_aligned(gamma, 16) && ufnd_aligned(beta, 16) && ufnd_aligned(out, 16), "ln_meanpool_live: alignment");
  NI_LAUNCH(H, ln_meanpool_kernel, dim3(B), (hipStream_t)stream_, y, gamma, beta, eps, mask, cu_seqlens, out, L, H);
  UFND_CHECK_LAUNCH();
  hipLaunchKernelGGL(l2norm_rows_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream_, out, H);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_vit_patchify(const float* frames, void* patches, int N, int image, int patch, void* stream_) {
  UFND_REQUIRE(frames && patches && N >= 1, "patchify: null argument");
  UFND_REQUIRE(patch % 8 == 0 && image % patch == 0 && ufnd_aligned(frames, 16) && ufnd_aligned(patches, 16),
               "patchify: image=%d patch=%d (patch a multiple of 8, 16-B aligned buffers)", image, patch);
  const int G = image / patch;
  if (patch == 32 && G == 7) hipLaunchKernelGGL((patchify_kernel<32, 7>), dim3(N * G), dim3(256), 0, (hipStream_t)stream_, frames, (__bf16*)patches, image, patch);
  else hipLaunchKernelGGL((patchify_kernel<0, 0>), dim3(N * G), dim3(256), 0, (hipStream_t)stream_, frames, (__bf16*)patches, image, patch);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_vit_assemble(const float* patch_emb, const float* cls, const float* pos, const float* gamma,
                                 const float* beta, float* x_f32, void* x_bf16, float* stats, int N, int P, int H, float eps,
                                 void* stream_) {
  UFND_REQUIRE(patch_emb && cls && pos && ((gamma && beta) || (!gamma && !beta)) && (x_f32 || x_bf16) && N >= 1 && P >= 1, "vit_assemble: null argument");
  UFND_REQUIRE(h_ok(H), "vit_assemble: H=%d", H);
  const int M = N * (P + 1);
  UFND_REQUIRE(!stats || ufnd_aligned(stats, 16), "vit_assemble: stats alignment");
  UFND_REQUIRE((!x_f32 || ufnd_aligned(x_f32, 16)) && (!x_bf16 || ufnd_aligned(x_bf16, 8)), "vit_assemble: alignment");
  NI_LAUNCH(H, vit_assemble_kernel, dim3(ufnd_cdiv(M, 4)), (hipStream_t)stream_, patch_emb, cls, pos, gamma, beta, x_f32,
            (__bf16*)x_bf16, stats, M, P, H, eps);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_l2norm_frames(const float* e, float* out, int B, int F, int D, void* stream_) {
  UFND_REQUIRE(e && out && B >= 1 && F >= 1 && D >= 1 && D <= 1024, "l2norm_frames: B=%d F=%d D=%d", B, F, D);
  hipLaunchKernelGGL(l2norm_frames_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream_, e, out, F, D);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_field_mean_l2(const float* parts, const int32_t* valid, float* out, int N, int Mx, int D, void* stream_) {
  UFND_REQUIRE(parts && valid && out && N >= 1 && Mx >= 1 && D >= 1 && D <= 1024, "field_mean_l2: N=%d M=%d D=%d", N, Mx, D);
  hipLaunchKernelGGL(field_mean_l2_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream_, parts, valid, out, Mx, D);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

// ------------------------------------------------------------------------------------------------
// Fold guard: the largest |mean| / std among the rows of a LayerNorm-statistics buffer (see ufnd_gemm_bf16_ln).
// ------------------------------------------------------------------------------------------------
namespace {
// Four lanes per row: lane j of a quad adds 16-B chunks j, j + 4, ... of the row's `parts` {sum, sumsq} pairs (parts is even),
// the quad combines by DPP.
__global__ __launch_bounds__(256) void ln_fold_guard_kernel(const float* stats, int M, int parts, float inv_h, float eps, float* guard) {
  __shared__ float sh[4];
  float worst = 0.0f;
  const int nq = parts >> 1, sub = threadIdx.x & 3;
  const long long total = M;
  // two rows per quad and pass, their (at most 3 + 3: parts <= 24) chunk loads issued together (clamped, masked at use): the
  // kernel is a stream of 192-B rows and was latency-bound with one load in flight per lane (36 us for 55 MB)
  const long long step = (long long)gridDim.x * 64;
  for (long long r = (long long)blockIdx.x * 64 + (threadIdx.x >> 2); r < total; r += 2 * step) {
    f32x4 v[2][3];
    bool live[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const long long rk = r + k * step;
      live[k] = rk < total;
      const long long rc = live[k] ? rk : r;
      const f32x4* p = reinterpret_cast<const f32x4*>(stats + (size_t)rc * parts * 2);
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        const int c = sub + 4 * u;
        v[k][u] = p[c < nq ? c : sub];
      }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      float sm = 0.0f, sq = 0.0f;
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        if (sub + 4 * u < nq) {
          sm += v[k][u][0] + v[k][u][2];
          sq += v[k][u][1] + v[k][u][3];
        }
      }
      sm += quad_xor1(sm); sq += quad_xor1(sq);
      sm += quad_xor2(sm); sq += quad_xor2(sq);
      const float mean = sm * inv_h;
      const float var = fmaxf(sq * inv_h - mean * mean, 0.0f);
      if (live[k]) {
        float ratio = fabsf(mean) * rsqrtf(var + eps);
        ratio = ratio == ratio ? ratio : INFINITY;      // (a NaN statistic must trip the guard: fmaxf would drop it)
        worst = fmaxf(worst, ratio);
      }
    }
  }
  worst = wave_max(worst);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = worst;
  __syncthreads();
  if (threadIdx.x == 0)
    atomicMax(reinterpret_cast<int*>(guard), __float_as_int(fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]))));   // non-negative floats order like ints
}
}  // namespace

extern "C" int ufnd_ln_fold_guard(const float* stats, int M, int parts, int width, float eps, float* guard, void* stream_) {
  UFND_REQUIRE(stats && guard && M >= 1 && parts >= 2 && parts <= 24 && parts % 2 == 0 && width >= 1 && ufnd_aligned(stats, 16),
               "ln_fold_guard: M=%d parts=%d (even)", M, parts);
  const int want = (int)((M + 63ll) / 64);
  hipLaunchKernelGGL(ln_fold_guard_kernel, dim3(want < 2048 ? want : 2048), dim3(256), 0, (hipStream_t)stream_, stats, M, parts,
                     1.0f / (float)width, eps, guard);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}
