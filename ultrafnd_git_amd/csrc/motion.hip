// Video motion forensics: OpticalFlow3DCNN.extract (src/core_blocks/visual_blocks.py) and ChronosGuard (src/models/chronos_guard.py) on the
// branches the reference itself takes without OpenCV: nearest-neighbour resize to 256 x 256, a float64 luma truncated to uint8, 32-bin
// frame histograms, |frame difference| as the flow, a 1-2-4 temporal pyramid of per-pixel means with an 8-bin orientation histogram.
//   gray     per frame: gather source pixel ((y H) >> 8, (x W) >> 8), luma in double with individually rounded operations in the
//            reference's order, the uint8 plane, the frame's 32-bin counts per 16-row slab (LDS integer adds)
//   pairs    per clip and 1024-pixel tile, a thread owns 4 pixels and walks time once: per-pair integer sums of |d| (a partial per
//            wave), and per pixel and pyramid chunk integer sums of |d| and sign(d) -> m, a, the 8-bin index; per-tile partials
//            per chunk: sum and centred second moment of m in double, max m, the 8 counts
//   finish   one workgroup per clip: fixed-order reduction of the partials -> cut scores, flow magnitudes, the seven ChronosGuard
//            statistics, the 77 pooled values, both tiled and L2-normalised vectors, the tamper score
// Everything up to the per-pixel m and a is integer arithmetic and two correctly rounded fp32 divisions, so it reproduces the
// reference bit for bit; the statistics above it are evaluated in double.  No global atomics, fixed reduction orders: a clip's results
// are the same bits alone, in any batch and from run to run.  Degenerate clips give what the reference gives, NaN included: an empty
// pyramid chunk (fewer than 4 pairs) is a NaN mean, a zero-variance series is a NaN correlation.
#include "common.hpp"
#include "frames.hpp"

namespace {

constexpr int SIDE = 256, PLANE = SIDE * SIDE;      // the reference's working size
constexpr int SLABS = 16;                           // gray: workgroups per frame, 16 rows each
constexpr int TILES = PLANE / 1024;                 // pairs: workgroups per clip, 256 threads x 4 pixels
constexpr int PAIR_PARTS = TILES * 4;               // per-pair partials of a clip: one per wave
constexpr int CHUNKS = 7, CHUNK_FEATS = 11, POOLED = CHUNKS * CHUNK_FEATS;

// the workspace: [gray B T 65536 u8][hist B T 16 32 i32][pair B max(T-1,1) 256 i32][moments B 7 64 2 f64][max B 7 64 f32][bins B 7 64 8 i32]
struct Workspace {
  uint8_t* gray;
  int32_t* hist;
  int32_t* pair;
  double* mom;
  float* mx;
  int32_t* bins;
  size_t bytes;
};
inline Workspace carve(void* base, long long B, long long T) {
  Workspace w;
  size_t off = 0;
  auto take = [&](size_t n) { const size_t at = off; off += (n + 255) / 256 * 256; return (char*)base + at; };
  w.gray = (uint8_t*)take((size_t)B * T * PLANE);
  w.mom = (double*)take((size_t)B * CHUNKS * TILES * 2 * sizeof(double));
  w.hist = (int32_t*)take((size_t)B * T * SLABS * 32 * sizeof(int32_t));
  w.pair = (int32_t*)take((size_t)B * (T > 1 ? T - 1 : 1) * PAIR_PARTS * sizeof(int32_t));
  w.mx = (float*)take((size_t)B * CHUNKS * TILES * sizeof(float));
  w.bins = (int32_t*)take((size_t)B * CHUNKS * TILES * 8 * sizeof(int32_t));
  w.bytes = off;
  return w;
}

// ---- gray: grid B T 16, 256 threads; a thread packs 4 neighbouring outputs into one 32-bit store, 4 times
__global__ __launch_bounds__(256) void motion_gray_kernel(const uint8_t* src, long long sb, long long st, long long sc, long long sh, long long sw,
                                                          const int32_t* lengths, uint8_t* gray, int32_t* hist, int T, int H, int W) {
  __shared__ int bins[32];
  const int slab = blockIdx.x % SLABS;
  const long long frame = blockIdx.x / SLABS;
  const int b = (int)(frame / T), t = (int)(frame % T);
  if (t >= clip_len(lengths, b, T)) return;      // (uniform: frames past a clip's end are neither read nor written)
  const int tid = threadIdx.x;
  if (tid < 32) bins[tid] = 0;
  __syncthreads();
  const uint8_t* fr = src + b * sb + t * st;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int q = i * 256 + tid;
    const int y = slab * (SIDE / SLABS) + (q >> 6), x0 = (q & 63) * 4;
    const uint8_t* row = fr + (((long long)y * H) >> 8) * sh;
    uint32_t packed = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint8_t* px = row + (((long long)(x0 + j) * W) >> 8) * sw;
      const uint32_t v = luma_u8(px[0], px[sc], px[2 * sc]);
      packed |= v << (8 * j);
      atomicAdd(&bins[min(31, (int)(32u * v) / 255)], 1);      // np.histogram(bins=32, range=(0, 255)) for every uint8 value
    }
    *reinterpret_cast<uint32_t*>(gray + (size_t)frame * PLANE + y * SIDE + x0) = packed;
  }
  __syncthreads();
  if (tid < 32) hist[((size_t)frame * SLABS + slab) * 32 + tid] = bins[tid];
}

// ---- pairs and pyramid: grid B 64, 256 threads
struct ChunkAcc {      // a pixel quad's sums over one pyramid chunk
  int a[4], s[4];
};
template <bool PYRAMID>
__global__ __launch_bounds__(256) void motion_pairs_kernel(const uint8_t* gray, const int32_t* lengths, int32_t* pair, double* mom, float* mx, int32_t* binsg,
                                                           int T) {
  __shared__ double redd[4][CHUNKS];
  __shared__ float redm[4][CHUNKS];
  __shared__ int bins[CHUNKS][8];
  const int b = blockIdx.x / TILES, tile = blockIdx.x % TILES;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n = clip_len(lengths, b, T);
  const int Tp = n > 1 ? n - 1 : 0, Tm = T > 1 ? T - 1 : 1;
  // the chunks of np.array slicing: levels of 1, 2, 4 parts of max(1, Tp // parts) pairs, the last part of a level runs to Tp
  const int s1 = max(1, Tp / 2), s2 = max(1, Tp / 4);
  const int c1 = min(s1, Tp), q1 = min(s2, Tp), q2 = min(2 * s2, Tp), q3 = min(3 * s2, Tp);
  const int lo0 = 0, hi0 = Tp, lo1 = 0, hi1 = c1, lo2 = c1, hi2 = Tp, lo3 = 0, hi3 = q1, lo4 = q1, hi4 = q2, lo5 = q2, hi5 = q3, lo6 = q3, hi6 = Tp;
  ChunkAcc k0 = {}, k1 = {}, k2 = {}, k3 = {}, k4 = {}, k5 = {}, k6 = {}, seg = {};
  const uint8_t* px = gray + (size_t)b * T * PLANE + tile * 1024 + tid * 4;
  uint32_t prev = Tp > 0 ? *reinterpret_cast<const uint32_t*>(px) : 0u;
  int seg_lo = 0;
  for (int t = 0; t < Tp; ++t) {
    const uint32_t cur = *reinterpret_cast<const uint32_t*>(px + (size_t)(t + 1) * PLANE);
    if (pair) {
      const int tot = wave_sum_i((int)__builtin_amdgcn_sad_u8(cur, prev, 0u));
      if (lane == 0) pair[((size_t)b * Tm + t) * PAIR_PARTS + tile * 4 + wave] = tot;
    }
    if (PYRAMID) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int d = (int)((cur >> (8 * j)) & 255u) - (int)((prev >> (8 * j)) & 255u);
        seg.a[j] += d < 0 ? -d : d;
        seg.s[j] += (d > 0) - (d < 0);
      }
      const int hi = t + 1;      // a run of pairs between two chunk boundaries ends here: add it to every chunk that holds it (uniform)
      if (hi == q1 || hi == q2 || hi == q3 || hi == c1 || hi == Tp) {
#define MOTION_FLUSH(K, LO, HI)                   \
  if (LO <= seg_lo && hi <= HI) {                 \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) { \
      K.a[j] += seg.a[j];                         \
      K.s[j] += seg.s[j];                         \
    }                                             \
  }
        MOTION_FLUSH(k0, lo0, hi0) MOTION_FLUSH(k1, lo1, hi1) MOTION_FLUSH(k2, lo2, hi2) MOTION_FLUSH(k3, lo3, hi3)
        MOTION_FLUSH(k4, lo4, hi4) MOTION_FLUSH(k5, lo5, hi5) MOTION_FLUSH(k6, lo6, hi6)
#undef MOTION_FLUSH
        seg = ChunkAcc{};
        seg_lo = hi;
      }
    }
    prev = cur;
  }
  if (!PYRAMID) return;
  if (tid < CHUNKS * 8) (&bins[0][0])[tid] = 0;
  __syncthreads();
  // per pixel and chunk: m = fl(sum|d| / n), a = fl(0.25 (2n + sum sign) / n) (the angle of a pair is exactly 0.75, 0.25 or 0.5), both
  // divisions correctly rounded -- mean angles sit on bin edges very often
  float m[CHUNKS][4];
  double sum[CHUNKS];
  float top[CHUNKS];
#define MOTION_PIXELS(C, K, LO, HI)                                           \
  {                                                                           \
    const int cn = HI > LO ? HI - LO : 0;                                     \
    sum[C] = 0.0;                                                             \
    top[C] = 0.0f;                                                            \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                           \
      m[C][j] = 0.0f;                                                         \
      if (cn > 0) {                                                           \
        m[C][j] = __fdiv_rn((float)K.a[j], (float)cn);                        \
        const float ang = __fdiv_rn(0.25f * (float)(2 * cn + K.s[j]), (float)cn); \
        atomicAdd(&bins[C][min(7, (int)floorf(8.0f * ang))], 1);              \
        sum[C] += (double)m[C][j];                                            \
        top[C] = fmaxf(top[C], m[C][j]);                                      \
      }                                                                       \
    }                                                                         \
  }
  MOTION_PIXELS(0, k0, lo0, hi0) MOTION_PIXELS(1, k1, lo1, hi1) MOTION_PIXELS(2, k2, lo2, hi2) MOTION_PIXELS(3, k3, lo3, hi3)
  MOTION_PIXELS(4, k4, lo4, hi4) MOTION_PIXELS(5, k5, lo5, hi5) MOTION_PIXELS(6, k6, lo6, hi6)
#undef MOTION_PIXELS
  // the tile's sum of m, then its second moment about the tile's own mean (finish combines the tiles by Chan's rule)
#pragma unroll
  for (int c = 0; c < CHUNKS; ++c) {
    const double ws = wave_sum_d(sum[c]);
    const float wm = wave_max(top[c]);
    if (lane == 0) {
      redd[wave][c] = ws;
      redm[wave][c] = wm;
    }
  }
  __syncthreads();
  double tsum[CHUNKS], dev2[CHUNKS];
#pragma unroll
  for (int c = 0; c < CHUNKS; ++c) {
    tsum[c] = (redd[0][c] + redd[1][c]) + (redd[2][c] + redd[3][c]);
    const double mean = tsum[c] * (1.0 / 1024.0);
    dev2[c] = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double d = (double)m[c][j] - mean;
      dev2[c] += d * d;
    }
  }
  float tmax[CHUNKS];
#pragma unroll
  for (int c = 0; c < CHUNKS; ++c) tmax[c] = fmaxf(fmaxf(redm[0][c], redm[1][c]), fmaxf(redm[2][c], redm[3][c]));
  __syncthreads();
#pragma unroll
  for (int c = 0; c < CHUNKS; ++c) {
    const double ws = wave_sum_d(dev2[c]);
    if (lane == 0) redd[wave][c] = ws;
  }
  __syncthreads();
  const size_t part = ((size_t)b * CHUNKS) * TILES + tile;      // + c TILES
  if (tid == 0) {
#pragma unroll
    for (int c = 0; c < CHUNKS; ++c) {
      mom[(part + (size_t)c * TILES) * 2 + 0] = tsum[c];
      mom[(part + (size_t)c * TILES) * 2 + 1] = (redd[0][c] + redd[1][c]) + (redd[2][c] + redd[3][c]);
      mx[part + (size_t)c * TILES] = tmax[c];
    }
  }
  if (tid < CHUNKS * 8) binsg[(part + (size_t)(tid >> 3) * TILES) * 8 + (tid & 7)] = bins[tid >> 3][tid & 7];
}

// ---- ChronosGuard finish: grid B, 256 threads.  A wave per pair: lanes 0..31 hold the bins of frame t, lanes 32..63 those of t + 1.
__global__ __launch_bounds__(256) void motion_chronos_finish_kernel(const int32_t* hist, const int32_t* pair, const int32_t* lengths, float* cut, float* flow,
                                                                    float* stats, float* features, float* tamper, int T, int feat_dim) {
  __shared__ float v7[8];
  __shared__ float nrm;
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n = clip_len(lengths, b, T);
  const int Tp = n > 1 ? n - 1 : 0, Tm = T - 1;
  for (int t = wave; t < Tm; t += 4) {
    float c32 = 0.0f, f32 = 0.0f;
    if (t < Tp) {      // (uniform per wave)
      const int32_t* hp = hist + ((size_t)b * T + t + (lane >> 5)) * SLABS * 32 + (lane & 31);
      int cnt = 0;
#pragma unroll
      for (int w = 0; w < SLABS; ++w) cnt += hp[w * 32];
      // density=True: counts / bin width / total, in that order, in double; then sum_k |h0_k - h1_k| by a fixed tree over the 32 bins
      const double h = (double)cnt / 7.96875 / 65536.0;
      const double other = __shfl_xor(h, 32, 64);
      double term = lane < 32 ? fabs(h - other) : 0.0;
#pragma unroll
      for (int o = 16; o >= 1; o >>= 1) term += __shfl_xor(term, o, 64);
      c32 = (float)__shfl(term, 0, 64);
      const int32_t* pp = pair + ((size_t)b * Tm + t) * PAIR_PARTS + lane * 4;
      const int tot = wave_sum_i((pp[0] + pp[1]) + (pp[2] + pp[3]));
      f32 = (float)tot * (1.0f / 65536.0f);      // exact: tot <= 255 * 65536 < 2^24
    }
    if (lane == 0) {
      cut[(size_t)b * Tm + t] = c32;
      flow[(size_t)b * Tm + t] = f32;
    }
  }
  __syncthreads();
  if (wave == 0) {      // the seven statistics in double over the fp32 series: mean, std, max of both, their correlation
    const float* cs = cut + (size_t)b * Tm;
    const float* fs = flow + (size_t)b * Tm;
    double sc = 0.0, sf = 0.0;
    float mc = 0.0f, mf = 0.0f;
    for (int t = lane; t < Tp; t += 64) {
      sc += (double)cs[t];
      sf += (double)fs[t];
      mc = fmaxf(mc, cs[t]);
      mf = fmaxf(mf, fs[t]);
    }
    sc = wave_sum_d(sc);
    sf = wave_sum_d(sf);
    mc = wave_max(mc);
    mf = wave_max(mf);
    const double meanc = Tp > 0 ? sc / Tp : 0.0, meanf = Tp > 0 ? sf / Tp : 0.0;
    double qcc = 0.0, qff = 0.0, qcf = 0.0;
    for (int t = lane; t < Tp; t += 64) {
      const double dc = (double)cs[t] - meanc, df = (double)fs[t] - meanf;
      qcc += dc * dc;
      qff += df * df;
      qcf += dc * df;
    }
    qcc = wave_sum_d(qcc);
    qff = wave_sum_d(qff);
    qcf = wave_sum_d(qcf);
    if (lane == 0) {
      double corr = 0.0;
      if (Tp > 3) {      // np.corrcoef: cov / std / std, clipped to [-1, 1]; 0 / 0 = NaN for a series without variance, kept
        corr = qcf / sqrt(qcc) / sqrt(qff);
        if (corr > 1.0) corr = 1.0;
        if (corr < -1.0) corr = -1.0;
      }
      v7[0] = (float)meanc;
      v7[1] = Tp > 0 ? (float)sqrt(qcc / Tp) : 0.0f;
      v7[2] = mc;
      v7[3] = (float)meanf;
      v7[4] = Tp > 0 ? (float)sqrt(qff / Tp) : 0.0f;
      v7[5] = mf;
      v7[6] = (float)corr;
      for (int k = 0; k < 7; ++k) stats[(size_t)b * 7 + k] = v7[k];
      // 0.6 norm01(mean cut, 0.05, 0.5) + 0.4 norm01(|std flow - mean flow|, 0, 0.5), norm01(x, lo, hi) = clip((x - lo) / (hi - lo + 1e-9), 0, 1)
      const double a = fmin(1.0, fmax(0.0, ((double)v7[0] - 0.05) / (0.5 - 0.05 + 1e-9)));
      const double m = fmin(1.0, fmax(0.0, fabs((double)v7[4] - (double)v7[3]) / (0.5 - 0.0 + 1e-9)));
      tamper[b] = Tp > 0 ? (float)fmin(1.0, fmax(0.0, 0.6 * a + 0.4 * m)) : 0.0f;
    }
  }
  __syncthreads();
  tile_normalise(v7, 7, features + (size_t)b * feat_dim, feat_dim, &nrm);
}

// ---- OpticalFlow3DCNN finish: grid B, 128 threads.  Thread c < 7 combines chunk c's 64 tile partials in tile order.
__global__ __launch_bounds__(128) void motion_flow_finish_kernel(const double* mom, const float* mx, const int32_t* binsg, const int32_t* lengths, float* pooled,
                                                                 float* out, int T, int dim) {
  __shared__ float v[POOLED];
  __shared__ float nrm;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = clip_len(lengths, b, T);
  const int Tp = n > 1 ? n - 1 : 0;
  if (tid < CHUNKS) {
    const int c = tid;
    const int s1 = max(1, Tp / 2), s2 = max(1, Tp / 4);
    int lo, hi;
    if (c == 0) { lo = 0; hi = Tp; }
    else if (c == 1) { lo = 0; hi = min(s1, Tp); }
    else if (c == 2) { lo = min(s1, Tp); hi = Tp; }
    else { lo = min((c - 3) * s2, Tp); hi = c == 6 ? Tp : min((c - 2) * s2, Tp); }
    const size_t part = ((size_t)b * CHUNKS + c) * TILES;
    float* f = v + c * CHUNK_FEATS;
    if (Tp == 0) {      // fewer than two frames: the reference returns zeros
      for (int k = 0; k < CHUNK_FEATS; ++k) f[k] = 0.0f;
    } else if (hi <= lo) {      // an empty chunk: the mean of nothing is NaN, and no angle lands in a bin
      const float nan = __builtin_nanf("");
      f[0] = f[1] = f[2] = nan;
      for (int k = 3; k < CHUNK_FEATS; ++k) f[k] = 0.0f;
    } else {
      double tot = 0.0;
      for (int i = 0; i < TILES; ++i) tot += mom[(part + i) * 2];
      const double mean = tot / (double)PLANE;
      double m2 = 0.0, between = 0.0;
      float top = 0.0f;
      for (int i = 0; i < TILES; ++i) {
        const double d = mom[(part + i) * 2] * (1.0 / 1024.0) - mean;
        m2 += mom[(part + i) * 2 + 1];
        between += d * d;
        top = fmaxf(top, mx[part + i]);
      }
      f[0] = (float)mean;
      f[1] = (float)sqrt((m2 + 1024.0 * between) / (double)PLANE);
      f[2] = top;
      for (int k = 0; k < 8; ++k) {
        int cnt = 0;
        for (int i = 0; i < TILES; ++i) cnt += binsg[(part + i) * 8 + k];
        f[3 + k] = (float)cnt;
      }
    }
  }
  __syncthreads();
  if (pooled && tid < POOLED) pooled[(size_t)b * POOLED + tid] = v[tid];
  if (Tp == 0) {      // (uniform) zeros, not 0 / 1e-9
    for (int j = tid; j < dim; j += blockDim.x) out[(size_t)b * dim + j] = 0.0f;
    return;
  }
  tile_normalise(v, POOLED, out + (size_t)b * dim, dim, &nrm);
}

int shape_checks(const char* what, int B, int T) {
  UFND_REQUIRE(B >= 1 && T >= 1 && (long long)B * T <= (1ll << 24) && (long long)B * TILES < (1ll << 31), "%s: B=%d T=%d (B >= 1 clips of T >= 1 frames, B T <= 2^24)",
               what, B, T);
  return UFND_OK;
}

}  // namespace

extern "C" size_t ufnd_motion_workspace_bytes(int B, int T) {
  if (B < 1 || T < 1 || (long long)B * T > (1ll << 24)) return 0;
  return carve(nullptr, B, T).bytes;
}

extern "C" int ufnd_motion_gray(const void* frames, long long stride_b, long long stride_t, long long stride_c, long long stride_h, long long stride_w,
                                const int32_t* lengths, void* workspace, int B, int T, int H, int W, void* stream_) {
  UFND_REQUIRE(frames && workspace, "motion_gray: null argument");
  const int rc = shape_checks("motion_gray", B, T);
  if (rc != UFND_OK) return rc;
  UFND_REQUIRE(H >= 1 && W >= 1 && H <= (1 << 20) && W <= (1 << 20), "motion_gray: H=%d W=%d (1 .. 2^20 each)", H, W);
  UFND_REQUIRE(stride_b >= 0 && stride_t >= 0 && stride_c >= 0 && stride_h >= 0 && stride_w >= 0, "motion_gray: negative stride");
  UFND_REQUIRE(ufnd_aligned(workspace, 256), "motion_gray: workspace alignment (256 bytes)");
  const Workspace w = carve(workspace, B, T);
  hipLaunchKernelGGL(motion_gray_kernel, dim3((unsigned)((long long)B * T * SLABS)), dim3(256), 0, (hipStream_t)stream_, (const uint8_t*)frames, stride_b,
                     stride_t, stride_c, stride_h, stride_w, lengths, w.gray, w.hist, T, H, W);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_motion_pairs(const int32_t* lengths, void* workspace, int B, int T, int pair_sums, int levels, void* stream_) {
  UFND_REQUIRE(workspace, "motion_pairs: null argument");
  const int rc = shape_checks("motion_pairs", B, T);
  if (rc != UFND_OK) return rc;
  UFND_REQUIRE(levels == 0 || levels == 3, "motion_pairs: levels=%d (the 1-2-4 pyramid of 3 levels, or 0 for none)", levels);
  UFND_REQUIRE(pair_sums || levels, "motion_pairs: neither pair sums nor the pyramid asked for");
  UFND_REQUIRE(ufnd_aligned(workspace, 256), "motion_pairs: workspace alignment (256 bytes)");
  const Workspace w = carve(workspace, B, T);
  int32_t* pair = pair_sums ? w.pair : nullptr;
  if (levels)
    hipLaunchKernelGGL(motion_pairs_kernel<true>, dim3(B * TILES), dim3(256), 0, (hipStream_t)stream_, (const uint8_t*)w.gray, lengths, pair, w.mom, w.mx, w.bins, T);
  else
    hipLaunchKernelGGL(motion_pairs_kernel<false>, dim3(B * TILES), dim3(256), 0, (hipStream_t)stream_, (const uint8_t*)w.gray, lengths, pair, w.mom, w.mx, w.bins, T);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_motion_chronos_finish(const int32_t* lengths, const void* workspace, float* cut_scores, float* flow_mags, float* stats, float* features,
                                          float* tamper_score, int B, int T, int feat_dim, void* stream_) {
  UFND_REQUIRE(workspace && stats && features && tamper_score && (T == 1 || (cut_scores && flow_mags)), "motion_chronos_finish: null argument");
  const int rc = shape_checks("motion_chronos_finish", B, T);
  if (rc != UFND_OK) return rc;
  UFND_REQUIRE(feat_dim >= 1, "motion_chronos_finish: dim=%d (>= 1)", feat_dim);
  const Workspace w = carve(const_cast<void*>(workspace), B, T);
  hipLaunchKernelGGL(motion_chronos_finish_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream_, (const int32_t*)w.hist, (const int32_t*)w.pair, lengths, cut_scores,
                     flow_mags, stats, features, tamper_score, T, feat_dim);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}

extern "C" int ufnd_motion_flow_finish(const int32_t* lengths, const void* workspace, float* pooled, float* features, int B, int T, int dim, int levels,
                                       void* stream_) {
  UFND_REQUIRE(workspace && features, "motion_flow_finish: null argument");
  const int rc = shape_checks("motion_flow_finish", B, T);
  if (rc != UFND_OK) return rc;
  UFND_REQUIRE(dim >= 1, "motion_flow_finish: dim=%d (>= 1)", dim);
  UFND_REQUIRE(levels == 3, "motion_flow_finish: levels=%d (the 1-2-4 pyramid of 3 levels)", levels);
  const Workspace w = carve(const_cast<void*>(workspace), B, T);
  hipLaunchKernelGGL(motion_flow_finish_kernel, dim3(B), dim3(128), 0, (hipStream_t)stream_, (const double*)w.mom, (const float*)w.mx, (const int32_t*)w.bins,
                     lengths, pooled, features, T, dim);
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}
