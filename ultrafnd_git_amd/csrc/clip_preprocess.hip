// CLIP image preprocessing on decoded uint8 frames, batched and ragged on the device: what the checkpoint's CLIPImageProcessor does on
// its Pillow backend (the processor the reference instantiates, src/models/semantic_forgery.py:54-61; the reference's loader resizes
// on the host, src/training/run_train_eval.py:304-313), equal to Pillow and the processor in every byte and every fp32 bit.
//
//   size       the short edge becomes S, the long edge int(S * long / short); W <= H makes the width the short edge
//   one pass   in -> out samples: scale = in / out, fs = max(scale, 1), support = 2 fs; output xx: c = (xx + 0.5) scale,
//              xmin = max(int(c - support + 0.5), 0), xmax = min(int(c + support + 0.5), in);
//              w[x] = bicubic((x + xmin - c + 0.5) (1 / fs)), a = -0.5, normalised by their double sum in index order;
//              k = (int)(w 2^22 +- 0.5), the sign of w;  pixel = clip((2^21 + sum k[x] p[xmin + x]) >> 22, 0, 255) in int32
//   order      horizontal, then vertical, a uint8 image between them; a pass with in == out is the identity table (one tap of 2^22)
//   crop       S x S at top = (h' - S) / 2, left = (w' - S) / 2 of the resized image
//   value map  r = fl32(double(v) 0.00392156862745098);  (r - fl32(mean[c])) / fl32(std[c]) in fp32: 768 values built on the host
//
// The tables (first, count, k[] of the S crop columns and the S crop rows) are built on the host in double (video.clip_resize_tables):
// the kernel sees tables, not scales.  ONE launch, a workgroup of 256 threads per (frame, tile of tile_rows output rows):
//   1. the intermediate rows r0 .. r1 - 1 the tile's vertical taps reach are resampled horizontally, RB rows at a time: the rows'
//      source bytes [x_lo, x_lo + x_span) are staged in LDS -- a wave per contiguous segment (the whole row of dense HWC pixels, one
//      row of each plane of CHW frames) in 16-byte reads, the LDS image shifted by the address's low 4 bits so that both sides are
//      aligned; any other view is gathered byte by byte -- then thread x runs column x of all staged rows: one coefficient load per
//      tap serves RB rows x 3 channels.  The rounded, clipped uint8 result goes to the intermediate image in LDS.
//   2. the vertical pass reads the intermediate as dwords (4 consecutive bytes of a row per LDS read), writes rgb and / or the value map's
//      floats.  The uint8 intermediate never travels through memory.
// Frame t >= len_b is computed from frame len_b - 1 (the same bits, the reference's padding rule); a clip of length 0 from an all-zero
// intermediate (the reference's dummy frame), nothing of it is read.  Every table entry is clamped into the source span and the tile
// before it addresses anything.  Integer sums are exact: the result does not depend on the tile, the staging mode or the batch.
// No atomics, no scratch, no workspace, no host synchronisation; hipGraph-capturable.
#include "frames.hpp"

namespace {

constexpr int NT = 256;      // threads of a workgroup
constexpr int RB = 8;        // source rows staged at a time (at most)
constexpr int BITS = 22;
constexpr int LUT_BYTES = 3 * 256 * 4, SOFF_BYTES = 128, HEAD_BYTES = LUT_BYTES + SOFF_BYTES;
constexpr int STAGE_BYTES = UFND_CLIP_PRE_STAGE_BYTES;
static_assert(RB * 3 * 4 <= SOFF_BYTES && HEAD_BYTES % 16 == 0 && UFND_CLIP_PRE_INTER_BYTES % 16 == 0 && UFND_CLIP_PRE_INTER_BYTES_LARGE % 16 == 0, "LDS layout");
static_assert(HEAD_BYTES + UFND_CLIP_PRE_INTER_BYTES + STAGE_BYTES <= 65536 && HEAD_BYTES + UFND_CLIP_PRE_INTER_BYTES_LARGE + STAGE_BYTES <= 160000, "LDS size");
static_assert(3 * ((UFND_CLIP_PRE_MAX_SPAN + 15) / 16 * 16 + 16) <= STAGE_BYTES && (3 * UFND_CLIP_PRE_MAX_SPAN + 15) / 16 * 16 + 16 <= STAGE_BYTES,
              "one source row of the widest span fits the stage in every mode");

enum { MODE_GATHER = 0, MODE_PIXELS = 1, MODE_PLANES = 2 };      // any view; stride_c = 1 and stride_w = 3; stride_w = 1

struct Args {
  const uint8_t* src;
  long long sb, st, sc, sh, sw;
  const int32_t* lengths;
  const int32_t* tab;
  const float* vmap;
  float* pv;
  uint8_t* rgb;
  int T, H, S, KH, KV, x_lo, x_span, TR, lds_rows, tiles, mode, rb, ipitch, segpitch, rgb_words;
};

__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// len bytes from g to s, one wave; s = (16-byte aligned) + (g & 15): the 16-byte body is aligned on both sides
__device__ __forceinline__ void copy_segment(const uint8_t* __restrict__ g, uint8_t* __restrict__ s, int len, int lane) {
  int head = (16 - (int)(reinterpret_cast<uintptr_t>(g) & 15)) & 15;
  head = head < len ? head : len;
  const int nvec = (len - head) >> 4, tail0 = head + (nvec << 4);
  for (int i = lane; i < nvec; i += 64) *reinterpret_cast<uint4*>(s + head + 16 * i) = *reinterpret_cast<const uint4*>(g + head + 16 * i);
  if (lane < head) s[lane] = g[lane];
  if (lane < len - tail0) s[tail0 + lane] = g[tail0 + lane];
}

// The horizontal pass over the nb <= RB staged rows: thread x runs crop column x of every row.  One coefficient load per tap (the next
// tap's is in flight) serves RB rows x 3 channels; |k| < 2^23 and a byte, so the products are 24-bit multiplies (v_mad_i32_i24, full
// rate; a 32-bit multiply-add is a quarter-rate v_mad_u64_u32).  Rows nb .. RB - 1 of a short batch read the stage's first bytes
// (offset 0, inside the first staged row) and are not written.  Every (row, channel) has its own byte offset soff[row][c], also where
// the three channels are neighbours: the compiler then issues 24 independent byte reads per tap and cannot merge neighbours into
// 16-bit reads at odd addresses (measured: the merged form took 1.75 times as long).
__device__ __forceinline__ void horizontal_columns(const Args& a, const uint8_t* __restrict__ stage, const int* __restrict__ soff, uint8_t* __restrict__ rows_out,
                                                   int nb, int tid) {
  const int PS = a.mode == MODE_PLANES ? 1 : 3;      // bytes between source columns
  const int S = a.S, x_hi = a.x_lo + a.x_span;
  const int32_t *hfirst = a.tab, *hcount = a.tab + S, *hk = a.tab + 4 * S;
  for (int x = tid; x < S; x += NT) {
    int first = hfirst[x];
    first = first < a.x_lo ? a.x_lo : (first > x_hi - 1 ? x_hi - 1 : first);
    int cnt = hcount[x];
    cnt = cnt > a.KH ? a.KH : cnt;
    cnt = cnt > x_hi - first ? x_hi - first : cnt;
    const int32_t* kx = hk + (size_t)x * a.KH;
    int acc[RB][3], so[RB][3];
#pragma unroll
    for (int rr = 0; rr < RB; ++rr) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        acc[rr][c] = 1 << (BITS - 1);
        so[rr][c] = rr < nb ? soff[rr * 3 + c] + (first - a.x_lo) * PS : 0;
      }
    }
    int k = cnt > 0 ? kx[0] : 0;
    for (int j = 0; j < cnt; ++j) {
      const int kn = j + 1 < cnt ? kx[j + 1] : 0;
      const uint8_t* s = stage + j * PS;
#pragma unroll
      for (int rr = 0; rr < RB; ++rr) {
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[rr][c] += __mul24(k, (int)s[so[rr][c]]);
      }
      k = kn;
    }
#pragma unroll
    for (int rr = 0; rr < RB; ++rr) {
      if (rr < nb) {      // (uniform)
        uint8_t* o = rows_out + rr * a.ipitch + 3 * x;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = (uint8_t)clip8(acc[rr][c]);
      }
    }
  }
}

template <int INTER_BYTES>
__global__ __launch_bounds__(NT) void clip_preprocess_kernel(const Args a) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[HEAD_BYTES + INTER_BYTES + STAGE_BYTES];
  float* lut = reinterpret_cast<float*>(lds);
  int* soff = reinterpret_cast<int*>(lds + LUT_BYTES);      // [row of the batch][channel]: where the channel's bytes of source column x_lo start in `stage`
  uint8_t* inter = lds + HEAD_BYTES;                        // lds_rows x ipitch: the horizontally resampled rows r0 .. of this tile
  uint8_t* stage = inter + INTER_BYTES;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = (int)(blockIdx.x % (unsigned)a.tiles);
  const int f = (int)(blockIdx.x / (unsigned)a.tiles);      // the output frame, b T + t
  const int b = f / a.T, t = f - b * a.T;
  const int n = clip_len(a.lengths, b, a.T);
  const int ts = n == 0 ? -1 : (t < n ? t : n - 1);         // the source frame; none for an empty clip
  const int S = a.S;
  const int32_t *vfirst = a.tab + 2 * S, *vcount = a.tab + 3 * S, *vk = a.tab + 4 * S + (size_t)S * a.KH;

  const int y0 = tile * a.TR, y1 = y0 + a.TR < S ? y0 + a.TR : S;
  int r0 = vfirst[y0];
  r0 = r0 < 0 ? 0 : (r0 > a.H - 1 ? a.H - 1 : r0);
  int r1 = vfirst[y1 - 1] + vcount[y1 - 1];
  r1 = r1 > a.H ? a.H : r1;
  int rows = r1 - r0;
  rows = rows < 0 ? 0 : (rows > a.lds_rows ? a.lds_rows : rows);      // (lds_rows ipitch <= INTER_BYTES: checked by the entry)

  for (int i = tid; i < 768; i += NT) lut[i] = a.vmap[i];

  if (ts < 0) {      // (uniform) the all-zero frame
    uint32_t* w = reinterpret_cast<uint32_t*>(inter);
    for (int i = tid; i < rows * (a.ipitch >> 2); i += NT) w[i] = 0u;
  } else {
    const uint8_t* fr = a.src + b * a.sb + ts * a.st;
    for (int rb0 = 0; rb0 < rows; rb0 += a.rb) {
      const int nb = rows - rb0 < a.rb ? rows - rb0 : a.rb;
      __syncthreads();      // the previous batch's stage has been read
      if (a.mode == MODE_GATHER) {
        const int nbytes = 3 * a.x_span;
        for (int rr = 0; rr < nb; ++rr) {
          const uint8_t* g = fr + (long long)(r0 + rb0 + rr) * a.sh + a.x_lo * a.sw;
          uint8_t* s = stage + rr * a.segpitch;
          for (int e = tid; e < nbytes; e += NT) {
            const int x = e / 3, c = e - 3 * x;
            s[e] = g[x * a.sw + c * a.sc];
          }
        }
        if (tid < nb * 3) soff[tid] = (tid / 3) * a.segpitch + tid % 3;
      } else {
        const int nseg = a.mode == MODE_PLANES ? 3 : 1;
        const int len = a.mode == MODE_PLANES ? a.x_span : 3 * a.x_span;
        for (int q = wave; q < nb * nseg; q += NT / 64) {      // (wave-uniform)
          const int rr = q / nseg, sg = q - rr * nseg;
          const uint8_t* g = fr + (long long)(r0 + rb0 + rr) * a.sh + a.x_lo * a.sw + sg * a.sc;
          const int at = q * a.segpitch + (int)(reinterpret_cast<uintptr_t>(g) & 15);
          copy_segment(g, stage + at, len, lane);
          if (nseg == 3) {
            if (lane == 0) soff[q] = at;
          } else if (lane < 3) {
            soff[rr * 3 + lane] = at + lane;
          }
        }
      }
      __syncthreads();
      horizontal_columns(a, stage, soff, inter + rb0 * a.ipitch, nb, tid);
    }
  }
  __syncthreads();

  const int nd = a.ipitch >> 2;      // dwords of an intermediate row
  const size_t frame = (size_t)f;
  for (int it = tid; it < (y1 - y0) * nd; it += NT) {
    const int yy = it / nd, d = it - yy * nd, y = y0 + yy;
    int first = vfirst[y] - r0;
    first = first < 0 ? 0 : first;
    int cnt = vcount[y];
    cnt = cnt > a.KV ? a.KV : cnt;
    cnt = cnt > rows - first ? rows - first : cnt;
    const int32_t* ky = vk + (size_t)y * a.KV;
    const uint8_t* col = inter + first * a.ipitch + 4 * d;
    int acc[4] = {1 << (BITS - 1), 1 << (BITS - 1), 1 << (BITS - 1), 1 << (BITS - 1)};
    int k = cnt > 0 ? ky[0] : 0;
    for (int j = 0; j < cnt; ++j) {
      const int kn = j + 1 < cnt ? ky[j + 1] : 0;
      const uint32_t w = *reinterpret_cast<const uint32_t*>(col + j * a.ipitch);
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] += __mul24(k, (int)((w >> (8 * q)) & 255u));
      k = kn;
    }
    int v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = clip8(acc[q]);
    const int e0 = 4 * d;      // byte e of the row is channel e % 3 of column e / 3
    if (a.rgb) {
      uint8_t* o = a.rgb + (frame * S + y) * (size_t)(3 * S) + e0;
      if (a.rgb_words) {      // (uniform) 3 S is a multiple of 4 and rgb is 4-byte aligned
        *reinterpret_cast<uint32_t*>(o) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (e0 + q < 3 * S) o[q] = (uint8_t)v[q];
      }
    }
    if (a.pv) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int e = e0 + q, x = e / 3, c = e - 3 * x;
        if (e < 3 * S) a.pv[((frame * 3 + c) * S + y) * (size_t)S + x] = lut[c * 256 + v[q]];
      }
    }
  }
}

}  // namespace

extern "C" int ufnd_clip_preprocess(const void* frames, long long stride_b, long long stride_t, long long stride_c, long long stride_h, long long stride_w,
                                    const int32_t* lengths, const int32_t* tables, const float* value_map, float* pixel_values, void* rgb, int B, int T,
                                    int H, int W, int S, int taps_h, int taps_v, int x_lo, int x_span, int tile_rows, int lds_rows, void* stream_) {
  UFND_REQUIRE(frames && tables && value_map, "clip_preprocess: null argument (frames, tables, value_map)");
  UFND_REQUIRE(pixel_values || rgb, "clip_preprocess: no output asked for (pixel_values, rgb)");
  UFND_REQUIRE(B >= 1 && T >= 1 && (long long)B * T <= UFND_CLIP_PRE_MAX_FRAMES, "clip_preprocess: B=%d T=%d (B, T >= 1, B T <= 2^24 frames)", B, T);
  UFND_REQUIRE(H >= 1 && W >= 1 && H <= UFND_CLIP_PRE_MAX_EDGE && W <= UFND_CLIP_PRE_MAX_EDGE, "clip_preprocess: H=%d W=%d (1 .. %d each)", H, W,
               UFND_CLIP_PRE_MAX_EDGE);
  UFND_REQUIRE(S >= UFND_CLIP_PRE_MIN_SIZE && S <= UFND_CLIP_PRE_MAX_SIZE, "clip_preprocess: image_size=%d (%d .. %d)", S, UFND_CLIP_PRE_MIN_SIZE,
               UFND_CLIP_PRE_MAX_SIZE);
  UFND_REQUIRE(taps_h >= 1 && taps_h <= UFND_CLIP_PRE_MAX_TAPS && taps_v >= 1 && taps_v <= UFND_CLIP_PRE_MAX_TAPS,
               "clip_preprocess: taps_h=%d taps_v=%d (1 .. %d taps per pass)", taps_h, taps_v, UFND_CLIP_PRE_MAX_TAPS);
  UFND_REQUIRE(x_lo >= 0 && x_span >= 1 && x_span <= UFND_CLIP_PRE_MAX_SPAN && (long long)x_lo + x_span <= W,
               "clip_preprocess: x_lo=%d x_span=%d (a span of 1 .. %d source columns inside the row of %d)", x_lo, x_span, UFND_CLIP_PRE_MAX_SPAN, W);
  UFND_REQUIRE(tile_rows >= 1 && tile_rows <= UFND_CLIP_PRE_MAX_TILE_ROWS, "clip_preprocess: tile_rows=%d (1 .. %d)", tile_rows, UFND_CLIP_PRE_MAX_TILE_ROWS);
  const int ipitch = (3 * S + 3) / 4 * 4;
  UFND_REQUIRE(lds_rows >= 1 && lds_rows <= H && (long long)lds_rows * ipitch <= UFND_CLIP_PRE_INTER_BYTES_LARGE,
               "clip_preprocess: lds_rows=%d (1 .. H rows of %d bytes, at most %d bytes of intermediate)", lds_rows, ipitch, UFND_CLIP_PRE_INTER_BYTES_LARGE);
  const int tiles = ufnd_cdiv(S, tile_rows);
  UFND_REQUIRE((long long)B * T * tiles <= 2147483647ll, "clip_preprocess: workgroups=%lld (B T ceil(image_size / tile_rows) <= 2^31 - 1)",
               (long long)B * T * tiles);
  UFND_REQUIRE(stride_b >= 0 && stride_t >= 0 && stride_c >= 0 && stride_h >= 0 && stride_w >= 0, "clip_preprocess: negative stride");
  UFND_REQUIRE(ufnd_aligned(tables, 4) && ufnd_aligned(value_map, 4) && ufnd_aligned(pixel_values, 4) && ufnd_aligned(lengths, 4),
               "clip_preprocess: alignment (tables, value_map, pixel_values, lengths: 4 bytes)");
  Args a;
  a.src = (const uint8_t*)frames;
  a.sb = stride_b, a.st = stride_t, a.sc = stride_c, a.sh = stride_h, a.sw = stride_w;
  a.lengths = lengths, a.tab = tables, a.vmap = value_map, a.pv = pixel_values, a.rgb = (uint8_t*)rgb;
  a.T = T, a.H = H, a.S = S, a.KH = taps_h, a.KV = taps_v, a.x_lo = x_lo, a.x_span = x_span, a.TR = tile_rows, a.lds_rows = lds_rows, a.tiles = tiles;
  a.mode = (stride_c == 1 && stride_w == 3) ? MODE_PIXELS : (stride_w == 1 ? MODE_PLANES : MODE_GATHER);
  const int len = a.mode == MODE_PLANES ? x_span : 3 * x_span, nseg = a.mode == MODE_PLANES ? 3 : 1;
  a.segpitch = (len + 15) / 16 * 16 + 16;
  a.rb = STAGE_BYTES / (nseg * a.segpitch);      // >= 1: x_span <= the span limit (static_assert above)
  a.rb = a.rb > RB ? RB : a.rb;
  a.ipitch = ipitch;
  a.rgb_words = (3 * S) % 4 == 0 && ufnd_aligned(rgb, 4);
  const dim3 grid((unsigned)((long long)B * T * tiles));
  if ((long long)lds_rows * ipitch <= UFND_CLIP_PRE_INTER_BYTES)
    hipLaunchKernelGGL(clip_preprocess_kernel<UFND_CLIP_PRE_INTER_BYTES>, grid, dim3(NT), 0, (hipStream_t)stream_, a);
  else
    hipLaunchKernelGGL(clip_preprocess_kernel<UFND_CLIP_PRE_INTER_BYTES_LARGE>, grid, dim3(NT), 0, (hipStream_t)stream_, a);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}
