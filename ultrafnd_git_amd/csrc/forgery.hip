// Image-forgery evidence: DeepForgeryDetector.ela_lbp and FaceWarpAnalyzer.score (src/core_blocks/visual_blocks.py:265-406), batched.  The
// reference resizes one frame per clip to 256 x 256 (nearest neighbour), re-encodes it as JPEG through OpenCV, and reads the error level
// (ELA) map |rgb - decoded| : its mean / std / max / min, a 3 x 3 "how many neighbours are greater" histogram of its luma, and, for the
// score, the gradient magnitude of the source's luma.  A JPEG round trip is deterministic integer arithmetic -- entropy coding is
// lossless -- so no bitstream is built: colour conversion, 2 x 2 chroma downsampling, libjpeg's jfdctint, quantisation, dequantisation,
// jidctint, fancy h2v2 upsampling, colour conversion back.  Every value equals what baseline 4:2:0 libjpeg decodes, in every byte.
//   resize     per clip the frame len / 2, source pixel ((y H) >> 8, (x W) >> 8) -> rgb (B, 256, 256, 3) in the workspace
//   roundtrip  dct: a workgroup owns 16 x 128 pixels = 8 MCUs = 32 Y + 8 Cb + 8 Cr blocks in LDS, one thread per block row, then per block
//              column (forward columns, quantise, dequantise, inverse columns without leaving the registers), then per block row again
//              -> decoded Y (256^2), Cb, Cr (128^2) planes;  upsample: the planes -> rec (B, 256, 256, 3).  Two launches: the upsampler reads
//              decoded chroma across block and workgroup boundaries.  jpeg_mode 0 (the reference without OpenCV): rec = rgb, one copy kernel.
//   maps       per 16-row slab: the ELA map and its luma (optionally stored), integer partials sum, sum of squares, max, min, the nine LBP
//              counts; the source luma's sum of sqrt(gx^2 + gy^2) in double and of gx^2 + gy^2 as an integer
//   finish     one wave per clip, the 16 slabs in order: stats, the histogram, the tiled and normalised vector, the gradient mean / std, the score
// No global atomics, fixed reduction orders: a clip's results are the same bits alone, in any batch and from run to run.
#include "common.hpp"
#include "frames.hpp"

namespace {

constexpr int SIDE = 256, PLANE = SIDE * SIDE, RGB = PLANE * 3;      // the reference's working size
constexpr int CSIDE = 128, CPLANE = CSIDE * CSIDE;                   // 4:2:0 chroma
constexpr int SLABS = 16, SLAB_ROWS = SIDE / SLABS;                  // resize, upsample, maps: workgroups per image
constexpr int DCT_GROUPS = 32;                                       // dct: workgroups per image, 16 rows x 128 columns each
constexpr int PART = 16;                                             // int32 partials per slab: sum, sum of squares, max, min, 9 counts, sum n
constexpr int CENTRES = 127 * 127;

struct QTables {      // natural order, luma then chroma
  uint8_t q[128];
};

// the workspace: [rgb B 196608 u8][rec 2 B 196608 u8][gsum B 16 f64][Y B 65536][Cb B 16384][Cr B 16384][part 2 B 16 16 i32]
struct Workspace {
  uint8_t* rgb;
  uint8_t* rec[2];
  uint8_t *y, *cb, *cr;
  int32_t* part[2];
  double* gsum;
  size_t bytes;
};
inline Workspace carve(void* base, long long B) {
  Workspace w;
  size_t off = 0;
  auto take = [&](size_t n) { const size_t at = off; off += (n + 255) / 256 * 256; return (char*)base + at; };
  w.rgb = (uint8_t*)take((size_t)B * RGB);
  w.rec[0] = (uint8_t*)take((size_t)B * RGB);
  w.rec[1] = (uint8_t*)take((size_t)B * RGB);
  w.gsum = (double*)take((size_t)B * SLABS * sizeof(double));
  w.y = (uint8_t*)take((size_t)B * PLANE);
  w.cb = (uint8_t*)take((size_t)B * CPLANE);
  w.cr = (uint8_t*)take((size_t)B * CPLANE);
  w.part[0] = (int32_t*)take((size_t)B * SLABS * PART * sizeof(int32_t));
  w.part[1] = (int32_t*)take((size_t)B * SLABS * PART * sizeof(int32_t));
  w.bytes = off;
  return w;
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
// byte k of 12 bytes held in three dwords (k is a compile-time constant wherever this is called)
__device__ __forceinline__ int byte_of(const uint32_t (&w)[3], int k) { return (int)((w[k >> 2] >> (8 * (k & 3))) & 255u); }
__device__ __forceinline__ void put_byte(uint32_t (&w)[3], int k, int v) { w[k >> 2] |= (uint32_t)v << (8 * (k & 3)); }
__device__ __forceinline__ void load3(const uint8_t* p, uint32_t (&w)[3]) {
  const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
  w[0] = q[0]; w[1] = q[1]; w[2] = q[2];
}
__device__ __forceinline__ void store3(uint8_t* p, const uint32_t (&w)[3]) {
  uint32_t* q = reinterpret_cast<uint32_t*>(p);
  q[0] = w[0]; q[1] = w[1]; q[2] = w[2];
}

// ---- resize: grid B 16, 256 threads; a thread gathers 4 neighbouring output pixels and stores their 12 bytes as three dwords, 4 times
__global__ __launch_bounds__(256) void forgery_resize_kernel(const uint8_t* src, long long sb, long long st, long long sc, long long sh, long long sw,
                                                             const int32_t* lengths, uint8_t* rgb, int T, int H, int W) {
  const int b = blockIdx.x / SLABS, slab = blockIdx.x % SLABS;
  const int n = clip_len(lengths, b, T);
  if (n == 0) return;      // (uniform) an empty clip has no frame: nothing of it is read, its plane is not written
  const uint8_t* fr = src + b * sb + (long long)(n / 2) * st;      // frames[len(frames) // 2]
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int q = i * 256 + threadIdx.x;
    const int y = slab * SLAB_ROWS + (q >> 6), x0 = (q & 63) * 4;
    const uint8_t* row = fr + (((long long)y * H) >> 8) * sh;
    uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint8_t* px = row + (((long long)(x0 + j) * W) >> 8) * sw;
      put_byte(w, 3 * j + 0, px[0]);
      put_byte(w, 3 * j + 1, px[sc]);
      put_byte(w, 3 * j + 2, px[2 * sc]);
    }
    store3(rgb + (size_t)b * RGB + ((size_t)y * SIDE + x0) * 3, w);
  }
}

// ---- copy (jpeg_mode 0): grid B 48, 256 threads, 16 bytes each: rec = rgb for the clips that have a frame
constexpr int COPY_GROUPS = RGB / (256 * 16);
__global__ __launch_bounds__(256) void forgery_copy_kernel(const uint8_t* rgb, const int32_t* lengths, uint8_t* rec, int T) {
  const int b = blockIdx.x / COPY_GROUPS;
  if (clip_len(lengths, b, T) == 0) return;      // (uniform)
  const size_t at = ((size_t)blockIdx.x * 256 + threadIdx.x) * 16;
  *reinterpret_cast<uint4*>(rec + at) = *reinterpret_cast<const uint4*>(rgb + at);
}

// ---- the two LL&M passes of libjpeg's "islow" DCTs (jfdctint.c, jidctint.c): CONST_BITS 13, PASS1_BITS 2, constants FIX(x) = round(x 2^13)
constexpr int C_0_298 = 2446, C_0_390 = 3196, C_0_541 = 4433, C_0_765 = 6270, C_0_899 = 7373, C_1_175 = 9633;
constexpr int C_1_501 = 12299, C_1_847 = 15137, C_1_961 = 16069, C_2_053 = 16819, C_2_562 = 20995, C_3_072 = 25172;
template <typename I>
__device__ __forceinline__ I descale(I x, int n) { return (x + ((I)1 << (n - 1))) >> n; }

// forward, in place.  FIRST (rows): outputs 0 and 4 are << 2, the others DESCALE(., 11); second (columns): DESCALE(., 2) and DESCALE(., 15)
template <bool FIRST>
__device__ __forceinline__ void fdct8(int (&d)[8]) {
  const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  constexpr int N = FIRST ? 11 : 15;
  d[0] = FIRST ? (t10 + t11) * 4 : descale(t10 + t11, 2);
  d[4] = FIRST ? (t10 - t11) * 4 : descale(t10 - t11, 2);
  const int e = (t12 + t13) * C_0_541;
  d[2] = descale(e + t13 * C_0_765, N);
  d[6] = descale(e - t12 * C_1_847, N);
  const int z5 = ((t4 + t6) + (t5 + t7)) * C_1_175;
  const int z1 = -(t4 + t7) * C_0_899, z2 = -(t5 + t6) * C_2_562;
  const int z3 = -(t4 + t6) * C_1_961 + z5, z4 = -(t5 + t7) * C_0_390 + z5;
  d[7] = descale(t4 * C_0_298 + z1 + z3, N);
  d[5] = descale(t5 * C_2_053 + z2 + z4, N);
  d[3] = descale(t6 * C_3_072 + z2 + z3, N);
  d[1] = descale(t7 * C_1_501 + z1 + z4, N);
}
// inverse, every output DESCALE(., N): 11 for the columns, 18 for the rows.  The rows run in 64 bits: a workspace value can reach 2^15
// after a coarse quantiser, times a 15-bit constant, summed four times.
template <typename I, int N>
__device__ __forceinline__ void idct8(const int (&c)[8], int (&o)[8]) {
  const I e = ((I)c[2] + c[6]) * C_0_541;
  const I a2 = e - (I)c[6] * C_1_847, a3 = e + (I)c[2] * C_0_765;
  const I a0 = ((I)c[0] + c[4]) * 8192, a1 = ((I)c[0] - c[4]) * 8192;
  const I t10 = a0 + a3, t13 = a0 - a3, t11 = a1 + a2, t12 = a1 - a2;
  const I b0 = c[7], b1 = c[5], b2 = c[3], b3 = c[1];
  const I z5 = ((b0 + b2) + (b1 + b3)) * C_1_175;
  const I z1 = -(b0 + b3) * C_0_899, z2 = -(b1 + b2) * C_2_562;
  const I z3 = -(b0 + b2) * C_1_961 + z5, z4 = -(b1 + b3) * C_0_390 + z5;
  const I t0 = b0 * C_0_298 + z1 + z3, t1 = b1 * C_2_053 + z2 + z4, t2 = b2 * C_3_072 + z2 + z3, t3 = b3 * C_1_501 + z1 + z4;
  o[0] = (int)descale(t10 + t3, N); o[7] = (int)descale(t10 - t3, N);
  o[1] = (int)descale(t11 + t2, N); o[6] = (int)descale(t11 - t2, N);
  o[2] = (int)descale(t12 + t1, N); o[5] = (int)descale(t12 - t1, N);
  o[3] = (int)descale(t13 + t0, N); o[4] = (int)descale(t13 - t0, N);
}

// ---- dct: grid B 32, 256 threads.  Block b < 32 is the Y block (b / 16, b % 16) of the 16 x 128 region, 32 + 8 comp + k chroma block k.
// A block's row r starts at LDS word 72 b + 9 r: the odd row stride keeps the column pass off a single bank.
constexpr int BLOCKS = 48, BLOCK_WORDS = 72, ROW_WORDS = 9, TASKS = BLOCKS * 8;
__global__ __launch_bounds__(256) void forgery_dct_kernel(const uint8_t* rgb, const int32_t* lengths, QTables qt, uint8_t* yp, uint8_t* cbp, uint8_t* crp, int T) {
  __shared__ int blk[BLOCKS * BLOCK_WORDS];
  __shared__ uint8_t chroma[2][16][128];
  __shared__ int quant[128];
  const int b = blockIdx.x / DCT_GROUPS, g = blockIdx.x % DCT_GROUPS;
  if (clip_len(lengths, b, T) == 0) return;      // (uniform)
  const int y0 = (g >> 1) * 16, x0 = (g & 1) * 128, tid = threadIdx.x;
  if (tid < 128) quant[tid] = qt.q[tid];
  const uint8_t* img = rgb + (size_t)b * RGB;
  // colour conversion: a thread converts 4 neighbouring pixels, twice
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int q = i * 256 + tid, row = q >> 5, x = (q & 31) * 4;
    uint32_t w[3];
    load3(img + ((size_t)(y0 + row) * SIDE + x0 + x) * 3, w);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = byte_of(w, 3 * j), gg = byte_of(w, 3 * j + 1), bb = byte_of(w, 3 * j + 2), col = x + j;
      const int yy = (19595 * r + 38470 * gg + 7471 * bb + 32768) >> 16;
      blk[((row >> 3) * 16 + (col >> 3)) * BLOCK_WORDS + (row & 7) * ROW_WORDS + (col & 7)] = yy - 128;
      chroma[0][row][col] = (uint8_t)((-11059 * r - 21709 * gg + 32768 * bb + (128 << 16) + 32767) >> 16);
      chroma[1][row][col] = (uint8_t)((32768 * r - 27439 * gg - 5329 * bb + (128 << 16) + 32767) >> 16);
    }
  }
  __syncthreads();
  // 2 x 2 chroma downsample, bias 1 on even output columns and 2 on odd ones (x0 / 2 is even: the local parity is the image's)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int o = i * 256 + tid, comp = o >> 9, r = (o >> 6) & 7, c = o & 63;
    const int s = (chroma[comp][2 * r][2 * c] + chroma[comp][2 * r][2 * c + 1]) + (chroma[comp][2 * r + 1][2 * c] + chroma[comp][2 * r + 1][2 * c + 1]);
    blk[(32 + comp * 8 + (c >> 3)) * BLOCK_WORDS + r * ROW_WORDS + (c & 7)] = ((s + 1 + (c & 1)) >> 2) - 128;
  }
  __syncthreads();
  for (int task = tid; task < TASKS; task += 256) {      // forward rows
    int* p = blk + (task >> 3) * BLOCK_WORDS + (task & 7) * ROW_WORDS;
    int d[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = p[k];
    fdct8<true>(d);
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k] = d[k];
  }
  __syncthreads();
  for (int task = tid; task < TASKS; task += 256) {      // forward columns, quantise, dequantise, inverse columns
    const int blockno = task >> 3, c = task & 7;
    int* p = blk + blockno * BLOCK_WORDS + c;
    const int* q = quant + (blockno >= 32 ? 64 : 0) + c;
    int d[8], o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = p[k * ROW_WORDS];
    fdct8<false>(d);
#pragma unroll
    for (int k = 0; k < 8; ++k) {      // the coefficient is scaled by 8: divide |c| by 8 q with rounding, restore the sign, multiply by q
      const int qk = q[k * 8], qv = 8 * qk;
      const int mag = ((d[k] < 0 ? -d[k] : d[k]) + (qv >> 1)) / qv;
      d[k] = (d[k] < 0 ? -mag : mag) * qk;
    }
    idct8<int, 11>(d, o);
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k * ROW_WORDS] = o[k];
  }
  __syncthreads();
  for (int task = tid; task < TASKS; task += 256) {      // inverse rows, + 128, clamp: 8 bytes of a decoded plane
    const int blockno = task >> 3, r = task & 7;
    const int* p = blk + blockno * BLOCK_WORDS + r * ROW_WORDS;
    int d[8], o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = p[k];
    idct8<long long, 18>(d, o);
    uint32_t lo = 0u, hi = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      lo |= (uint32_t)clamp255(o[k] + 128) << (8 * k);
      hi |= (uint32_t)clamp255(o[k + 4] + 128) << (8 * k);
    }
    uint8_t* dst;
    if (blockno < 32) {
      dst = yp + (size_t)b * PLANE + (size_t)(y0 + (blockno >> 4) * 8 + r) * SIDE + x0 + (blockno & 15) * 8;
    } else {
      uint8_t* plane = (blockno < 40 ? cbp : crp) + (size_t)b * CPLANE;
      dst = plane + (size_t)(y0 / 2 + r) * CSIDE + x0 / 2 + (blockno & 7) * 8;
    }
    *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
  }
}

// ---- upsample: grid B 16, 256 threads; a thread makes 4 neighbouring pixels (two chroma columns), 4 times.  s = 3 near + far over the two
// chroma rows (far: the row above for even y, below for odd y, replicated at the edges); even x: (3 s_i + s_{i-1} + 8) >> 4, odd x:
// (3 s_i + s_{i+1} + 7) >> 4, the neighbour column replicated at the edges (which is libjpeg's (4 s + 8) >> 4 and (4 s + 7) >> 4 there).
__global__ __launch_bounds__(256) void forgery_upsample_kernel(const uint8_t* yp, const uint8_t* cbp, const uint8_t* crp, const int32_t* lengths, uint8_t* rec,
                                                               int T) {
  const int b = blockIdx.x / SLABS, slab = blockIdx.x % SLABS;
  if (clip_len(lengths, b, T) == 0) return;      // (uniform)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int q = i * 256 + threadIdx.x;
    const int y = slab * SLAB_ROWS + (q >> 6), x0 = (q & 63) * 4;
    const int near = y >> 1, far = (y & 1) ? min(near + 1, CSIDE - 1) : max(near - 1, 0);
    const int i0 = x0 >> 1;
    const int col[4] = {max(i0 - 1, 0), i0, i0 + 1, min(i0 + 2, CSIDE - 1)};
    int up[2][4];      // the four upsampled values of Cb, Cr, minus 128
#pragma unroll
    for (int comp = 0; comp < 2; ++comp) {
      const uint8_t* plane = (comp ? crp : cbp) + (size_t)b * CPLANE;
      int s[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) s[k] = 3 * (int)plane[near * CSIDE + col[k]] + (int)plane[far * CSIDE + col[k]];
      up[comp][0] = ((3 * s[1] + s[0] + 8) >> 4) - 128;
      up[comp][1] = ((3 * s[1] + s[2] + 7) >> 4) - 128;
      up[comp][2] = ((3 * s[2] + s[1] + 8) >> 4) - 128;
      up[comp][3] = ((3 * s[2] + s[3] + 7) >> 4) - 128;
    }
    const uint32_t y4 = *reinterpret_cast<const uint32_t*>(yp + (size_t)b * PLANE + y * SIDE + x0);
    uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int yy = (int)((y4 >> (8 * j)) & 255u), cb = up[0][j], cr = up[1][j];
      put_byte(w, 3 * j + 0, clamp255(yy + ((91881 * cr + 32768) >> 16)));
      put_byte(w, 3 * j + 1, clamp255(yy + ((-22554 * cb + 32768 - 46802 * cr) >> 16)));
      put_byte(w, 3 * j + 2, clamp255(yy + ((116130 * cb + 32768) >> 16)));
    }
    store3(rec + (size_t)b * RGB + ((size_t)y * SIDE + x0) * 3, w);
  }
}

__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// ---- maps: grid B 16, 256 threads.  A wave takes a row at a time, a lane 4 neighbouring pixels of it (12 bytes of rgb, 12 of rec); the
// slab's 16 rows plus the row below (the LBP centres of the last row look down) and, of the source luma, the row above (gy).
__global__ __launch_bounds__(256) void forgery_maps_kernel(const uint8_t* rgb, const uint8_t* rec, const int32_t* lengths, float scale, uint8_t* ela_out,
                                                           uint8_t* gray_out, int32_t* part, double* gsum, int T, int want_lbp, int want_grad) {
  __shared__ alignas(16) uint8_t egray[SLAB_ROWS + 1][SIDE];      // luma of the ELA map, rows y0 .. y0 + 16
  __shared__ alignas(16) uint8_t sgray[SLAB_ROWS + 1][SIDE];      // luma of the source, rows y0 - 1 .. y0 + 15
  __shared__ int bins[9];
  __shared__ int redi[4][5];
  __shared__ double redd[4];
  const int b = blockIdx.x / SLABS, slab = blockIdx.x % SLABS;
  if (clip_len(lengths, b, T) == 0) return;      // (uniform)
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, y0 = slab * SLAB_ROWS;
  if (tid < 9) bins[tid] = 0;
  const uint8_t* img = rgb + (size_t)b * RGB;
  const uint8_t* dec = rec + (size_t)b * RGB;
  int sum = 0, sq = 0, top = 0, low = 255;
  for (int rr = wave - 1; rr <= SLAB_ROWS; rr += 4) {      // (uniform per wave)
    const int y = y0 + rr, x0 = lane * 4;
    if (y < 0 || y >= SIDE) continue;
    const bool own = rr >= 0 && rr < SLAB_ROWS;
    const size_t at = ((size_t)y * SIDE + x0) * 3;
    uint32_t a[3], d[3] = {0u, 0u, 0u}, e[3] = {0u, 0u, 0u};
    load3(img + at, a);
    if (rr >= 0) load3(dec + at, d);
    uint32_t g4 = 0u, s4 = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int v[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int diff = byte_of(a, 3 * j + c) - byte_of(d, 3 * j + c);
        const float amp = (float)(diff < 0 ? -diff : diff) * scale;      // float32, as the reference; clip, then truncate
        v[c] = (int)fminf(fmaxf(amp, 0.0f), 255.0f);
        put_byte(e, 3 * j + c, v[c]);
        if (own) {
          sum += v[c];
          sq += v[c] * v[c];
          top = max(top, v[c]);
          low = min(low, v[c]);
        }
      }
      g4 |= luma_u8((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2]) << (8 * j);
      s4 |= luma_u8((uint32_t)byte_of(a, 3 * j), (uint32_t)byte_of(a, 3 * j + 1), (uint32_t)byte_of(a, 3 * j + 2)) << (8 * j);
    }
    if (rr >= 0) *reinterpret_cast<uint32_t*>(&egray[rr][x0]) = g4;
    if (rr < SLAB_ROWS) *reinterpret_cast<uint32_t*>(&sgray[rr + 1][x0]) = s4;
    if (own && ela_out) store3(ela_out + (size_t)b * RGB + at, e);
    if (own && gray_out) *reinterpret_cast<uint32_t*>(gray_out + (size_t)b * PLANE + (size_t)y * SIDE + x0) = g4;
  }
  __syncthreads();
  double gs = 0.0;
  int ns = 0;
  if (want_grad) {      // thread = column: forward differences against the left and the upper neighbour, zero in column 0 and row 0
    const int x = tid;
    for (int r = 0; r < SLAB_ROWS; ++r) {
      const int g = sgray[r + 1][x];
      const int gx = x > 0 ? g - (int)sgray[r + 1][x - 1] : 0;
      const int gy = y0 + r > 0 ? g - (int)sgray[r][x] : 0;
      const int n = gx * gx + gy * gy;
      gs += sqrt((double)n);
      ns += n;
    }
  }
  if (want_lbp) {      // centres at odd (y, x) up to 253: thread -> centre column 2 (tid % 128) + 1, rows 1 + 2 (tid / 128) + 4 i
    const int x = 2 * (tid & 127) + 1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 1 + 2 * (tid >> 7) + 4 * i;
      if (x <= 253 && y0 + r <= 253) {
        const int c = egray[r][x];
        int code = 0;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx)
            if (dy || dx) code += (int)egray[r + dy][x + dx] > c;
        atomicAdd(&bins[code], 1);      // (LDS, integer: order-free)
      }
    }
  }
  sum = wave_sum_i(sum);
  sq = wave_sum_i(sq);
  ns = wave_sum_i(ns);
  top = wave_max_i(top);
  low = -wave_max_i(-low);
  gs = wave_sum_d(gs);
  if (lane == 0) {
    redi[wave][0] = sum; redi[wave][1] = sq; redi[wave][2] = top; redi[wave][3] = low; redi[wave][4] = ns;
    redd[wave] = gs;
  }
  __syncthreads();
  int32_t* out = part + ((size_t)b * SLABS + slab) * PART;
  if (tid == 0) {
    out[0] = (redi[0][0] + redi[1][0]) + (redi[2][0] + redi[3][0]);
    out[1] = (redi[0][1] + redi[1][1]) + (redi[2][1] + redi[3][1]);
    out[2] = max(max(redi[0][2], redi[1][2]), max(redi[2][2], redi[3][2]));
    out[3] = min(min(redi[0][3], redi[1][3]), min(redi[2][3], redi[3][3]));
    out[13] = (redi[0][4] + redi[1][4]) + (redi[2][4] + redi[3][4]);
    if (want_grad) gsum[(size_t)b * SLABS + slab] = (redd[0] + redd[1]) + (redd[2] + redd[3]);
  }
  if (tid < 9) out[4 + tid] = bins[tid];
}

// ---- finish: grid B, 64 threads.  Lane 0 walks the 16 slabs in order; the vector is tiled and normalised by the whole wave.
__global__ __launch_bounds__(64) void forgery_finish_kernel(const int32_t* part0, const int32_t* part_score, const double* gsum, const int32_t* lengths,
                                                            float* stats, float* lbp, float* features, float* grad, float* score, int T, int dim) {
  __shared__ float v[14];
  __shared__ float nrm;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (clip_len(lengths, b, T) == 0) {      // (uniform) no frame: the reference's zero vector and score 0.0
    if (stats && tid < 4) stats[(size_t)b * 4 + tid] = 0.0f;
    if (lbp && tid < 10) lbp[(size_t)b * 10 + tid] = 0.0f;
    if (grad && tid < 2) grad[(size_t)b * 2 + tid] = 0.0f;
    if (score && tid == 0) score[b] = 0.0f;
    if (features)
      for (int j = tid; j < dim; j += blockDim.x) features[(size_t)b * dim + j] = 0.0f;
    return;
  }
  const bool vector = stats || lbp || features;
  if (tid == 0) {
    constexpr long long N = 3ll * PLANE;
    if (vector) {
      const int32_t* p = part0 + (size_t)b * SLABS * PART;
      long long s = 0, q = 0, cnt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      int top = 0, low = 255;
      for (int i = 0; i < SLABS; ++i) {
        s += p[i * PART];
        q += p[i * PART + 1];
        top = max(top, p[i * PART + 2]);
        low = min(low, p[i * PART + 3]);
#pragma unroll
        for (int k = 0; k < 9; ++k) cnt[k] += p[i * PART + 4 + k];
      }
      // mean = S / N; variance = (N Q - S^2) / N^2, the numerator an exact integer below 2^53
      v[0] = (float)((double)s / (double)N);
      v[1] = (float)sqrt((double)(N * q - s * s) / ((double)N * (double)N));
      v[2] = (float)top;
      v[3] = (float)low;
#pragma unroll
      for (int k = 0; k < 9; ++k) v[4 + k] = (float)((double)cnt[k] / 1.0 / (double)CENTRES);      // density: count / bin width / total
      v[13] = 0.0f;                                                                                 // no code reaches [9, 10]
    }
    if (grad || score) {
      double g = 0.0;
      for (int i = 0; i < SLABS; ++i) g += gsum[(size_t)b * SLABS + i];
      const double mean = g / (double)PLANE;
      long long n2 = 0;
      for (int i = 0; i < SLABS; ++i) n2 += part0[((size_t)b * SLABS + i) * PART + 13];
      const double m2 = (double)n2 / (double)PLANE;      // the mean of sqrt(n)^2, exact
      const double g_mean = mean, g_std = sqrt(fmax(m2 - mean * mean, 0.0));
      if (grad) {
        grad[(size_t)b * 2] = (float)g_mean;
        grad[(size_t)b * 2 + 1] = (float)g_std;
      }
      if (score) {
        long long s = 0;
        for (int i = 0; i < SLABS; ++i) s += part_score[((size_t)b * SLABS + i) * PART];
        const double ela_mean = (double)s / (double)N / 255.0;
        const double raw = 0.5 * tanh(g_std / (g_mean + 1e-6)) + 0.5 * ela_mean;      // all in double, rounded once below
        score[b] = (float)fmin(1.0, fmax(0.0, raw));
      }
    }
  }
  __syncthreads();
  if (stats && tid < 4) stats[(size_t)b * 4 + tid] = v[tid];
  if (lbp && tid < 10) lbp[(size_t)b * 10 + tid] = v[4 + tid];
  if (features) tile_normalise(v, 14, features + (size_t)b * dim, dim, &nrm);
}

int shape_checks(const char* what, int B, int T) {
  UFND_REQUIRE(B >= 1 && B <= (1 << 16) && T >= 1, "%s: B=%d T=%d (1 <= B <= 65536 clips of T >= 1 frames)", what, B, T);
  return UFND_OK;
}

}  // namespace

extern "C" size_t ufnd_forgery_workspace_bytes(int B) {
  if (B < 1 || B > (1 << 16)) return 0;
  return carve(nullptr, B).bytes;
}

extern "C" int ufnd_forgery_resize(const void* frames, long long stride_b, long long stride_t, long long stride_c, long long stride_h, long long stride_w,
                                   const int32_t* lengths, void* workspace, int B, int T, int H, int W, void* stream_) {
  UFND_REQUIRE(frames && workspace, "forgery_resize: null argument");
  const int rc = shape_checks("forgery_resize", B, T);
  if (rc != UFND_OK) return rc;
  UFND_REQUIRE(H >= 1 && W >= 1 && H <= (1 << 20) && W <= (1 << 20), "forgery_resize: H=%d W=%d (1 .. 2^20 each)", H, W);
  UFND_REQUIRE(stride_b >= 0 && stride_t >= 0 && stride_c >= 0 && stride_h >= 0 && stride_w >= 0, "forgery_resize: negative stride");
  UFND_REQUIRE(ufnd_aligned(workspace, 256), "forgery_resize: workspace alignment (256 bytes)");
  const Workspace w = carve(workspace, B);
  hipLaunchKernelGGL(forgery_resize_kernel, dim3((unsigned)(B * SLABS)), dim3(256), 0, (hipStream_t)stream_, (const uint8_t*)frames, stride_b, stride_t, stride_c,
                     stride_h, stride_w, lengths, w.rgb, T, H, W);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_forgery_roundtrip(const int32_t* lengths, void* workspace, const unsigned char* qtables, int B, int T, int jpeg_mode, int slot, void* stream_) {
  UFND_REQUIRE(workspace, "forgery_roundtrip: null argument");
  const int rc = shape_checks("forgery_roundtrip", B, T);
  if (rc != UFND_OK) return rc;
  UFND_REQUIRE(jpeg_mode == 0 || jpeg_mode == 1, "forgery_roundtrip: jpeg_mode=%d (1: the libjpeg round trip, 0: none)", jpeg_mode);
  UFND_REQUIRE(slot == 0 || slot == 1, "forgery_roundtrip: slot=%d (0 or 1)", slot);
  UFND_REQUIRE(ufnd_aligned(workspace, 256), "forgery_roundtrip: workspace alignment (256 bytes)");
  const Workspace w = carve(workspace, B);
  hipStream_t stream = (hipStream_t)stream_;
  if (jpeg_mode == 0) {
    hipLaunchKernelGGL(forgery_copy_kernel, dim3((unsigned)(B * COPY_GROUPS)), dim3(256), 0, stream, (const uint8_t*)w.rgb, lengths, w.rec[slot], T);
    UFND_CHECK_LAUNCH();
    return UFND_OK;
  }
  UFND_REQUIRE(qtables, "forgery_roundtrip: null quantisation tables");
  QTables qt;
  for (int k = 0; k < 128; ++k) {
    UFND_REQUIRE(qtables[k] >= 1, "forgery_roundtrip: quantiser %d is 0 (1 .. 255)", k);
    qt.q[k] = qtables[k];
  }
  hipLaunchKernelGGL(forgery_dct_kernel, dim3((unsigned)(B * DCT_GROUPS)), dim3(256), 0, stream, (const uint8_t*)w.rgb, lengths, qt, w.y, w.cb, w.cr, T);
  UFND_CHECK_LAUNCH();
  hipLaunchKernelGGL(forgery_upsample_kernel, dim3((unsigned)(B * SLABS)), dim3(256), 0, stream, (const uint8_t*)w.y, (const uint8_t*)w.cb, (const uint8_t*)w.cr,
                     lengths, w.rec[slot], T);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_forgery_maps(const int32_t* lengths, void* workspace, float ela_scale, void* ela_map, void* ela_gray, int B, int T, int slot, int want_lbp,
                                 int want_grad, void* stream_) {
  UFND_REQUIRE(workspace, "forgery_maps: null argument");
  const int rc = shape_checks("forgery_maps", B, T);
  if (rc != UFND_OK) return rc;
  UFND_REQUIRE(slot == 0 || slot == 1, "forgery_maps: slot=%d (0 or 1)", slot);
  UFND_REQUIRE(ela_scale == ela_scale && ela_scale - ela_scale == 0.0f, "forgery_maps: ela_scale is not finite");
  UFND_REQUIRE(!want_grad || slot == 0, "forgery_maps: want_grad with slot=%d (the gradient partials belong to slot 0)", slot);
  UFND_REQUIRE(ufnd_aligned(workspace, 256) && ufnd_aligned(ela_map, 4) && ufnd_aligned(ela_gray, 4), "forgery_maps: alignment (workspace 256 bytes, maps 4)");
  const Workspace w = carve(workspace, B);
  hipLaunchKernelGGL(forgery_maps_kernel, dim3((unsigned)(B * SLABS)), dim3(256), 0, (hipStream_t)stream_, (const uint8_t*)w.rgb, (const uint8_t*)w.rec[slot], lengths,
                     ela_scale, (uint8_t*)ela_map, (uint8_t*)ela_gray, w.part[slot], w.gsum, T, want_lbp, want_grad);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_forgery_finish(const int32_t* lengths, const void* workspace, float* stats, float* lbp, float* features, float* grad, float* score, int B, int T,
                                   int dim, int score_slot, void* stream_) {
  UFND_REQUIRE(workspace && (stats || lbp || features || grad || score), "forgery_finish: null argument");
  const int rc = shape_checks("forgery_finish", B, T);
  if (rc != UFND_OK) return rc;
  UFND_REQUIRE(!features || dim >= 1, "forgery_finish: dim=%d (>= 1)", dim);
  UFND_REQUIRE(score_slot == 0 || score_slot == 1, "forgery_finish: score_slot=%d (0 or 1)", score_slot);
  const Workspace w = carve(const_cast<void*>(workspace), B);
  hipLaunchKernelGGL(forgery_finish_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream_, (const int32_t*)w.part[0], (const int32_t*)w.part[score_slot],
                     (const double*)w.gsum, lengths, stats, lbp, features, grad, score, T, dim);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}
