// Sample-rate conversion, the stage between a decoded waveform and every 16 kHz audio entry: the reference's _ensure_mono_16k
// (src/core_blocks/audio_blocks.py:34-45) resamples one clip at a time on the host with librosa; this is the batched device stage.
// Band-limited windowed-sinc interpolation in polyphase form (include/ultrafnd_hip.h states the filter): with o / n the reduced
// rate ratio,  y[q n + p] = sum_k h[p][k] xz[q o + k - width],  xz the mixed, scaled clip, zero outside [0, len).
//
// Formulation: a VALU FIR through LDS with the taps in scalar registers.  The host folds G strides into one super-stride
// (o' = G o, n' = G n; phase g n + p of the super-stride is phase p shifted by g o taps), so that small n still gives a workgroup
// many phases.  A workgroup owns `qt` (<= 64) super-strides of ONE clip: it stages samples q0 o' - width .. once into LDS (channel
// mix and zero substitution by index while staging: nothing at or past x[len] is read).  A wave owns a GROUP of 4 neighbouring
// phases; lane l owns super-stride q0 + l.  Per tap k the wave fetches the 4 phases' taps with ONE scalar load (the address is
// wave-uniform), each lane reads ONE sample from LDS (lane stride o': conflict-free when o' is odd) and issues 4 fmaf.  The
// group's band is the union of its phases' bands, rounded out to multiples of 8 taps; the table holds zeros where a phase has no tap.
// A filter longer than LDS (huge o / n) is walked in chunks of `kc` taps, restaged per chunk.
//
// One value, one arithmetic.  Output (q, p) is ONE chain of fmaf from +0 over the taps of phase p in ASCENDING k:
//     acc = 0;  for k = first[p] .. first[p] + count[p] - 1:  acc = fmaf(h[p][k], xz[q o + k - width], acc)
// The zero taps the group table adds before and after the band contribute fmaf(0, x, acc) = acc exactly for finite x, so the
// value does not depend on the group, G, the tile, the chunking, the batch or the row.  (A non-finite sample inside the clip
// reaches, as NaN, every output whose group band covers it -- up to 7 + 4 o / n taps beyond the true support.)  No atomics, no
// scratch, no host synchronisation; hipGraph-capturable.
#include "common.hpp"

namespace {

constexpr int QT = UFND_RESAMPLE_OUT_TILE;      // super-strides of a workgroup: one per lane
constexpr int PG = 4;                           // phases of a group (one 16-byte scalar load per tap)
constexpr int TA = 8;                           // taps of a loop step: group bands and chunks are multiples of it
constexpr int THREADS = 1024, WAVES = THREADS / 64;
constexpr int LDS_FLOATS = UFND_RESAMPLE_LDS_FLOATS;
constexpr int TARGET_WORKGROUPS = 256;          // phase slices are added until the grid has this many (one per CU)

struct Geometry {
  const void* waves;
  long long sb, sc, ss;      // element strides of (clip, channel, sample)
  const int32_t* lengths;
  int32_t* out_lengths;
  int C, n_max, o, n, op, np, width, ngroups, gps, qt, kc, nchunks, tap_rows;
  long long m_max;
  float scale;
};

template <class T>
__global__ __launch_bounds__(THREADS) void resample_kernel(const Geometry a, const float* __restrict__ taps, const int32_t* __restrict__ groups,
                                                           float* __restrict__ out_all) {
  __shared__ __attribute__((aligned(16))) float xs[LDS_FLOATS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = blockIdx.x, b = blockIdx.y, slice = blockIdx.z;
  int len = a.lengths ? a.lengths[b] : a.n_max;
  len = len < 0 ? 0 : (len > a.n_max ? a.n_max : len);
  const long long mb = ((long long)a.n * len + a.o - 1) / a.o;
  if (tile == 0 && slice == 0 && tid == 0) a.out_lengths[b] = (int32_t)mb;
  const long long q0 = (long long)tile * a.qt;
  float* out = out_all + (size_t)b * (size_t)a.m_max;
  const int g0 = slice * a.gps, g1 = min(g0 + a.gps, a.ngroups);

  if (q0 * a.np >= mb) {      // (uniform) nothing of the clip here: the zero padding of this slice's phases
    const int p0 = PG * g0, pn = min(PG * g1, a.np) - p0;
    for (int idx = tid; idx < a.qt * pn; idx += THREADS) {
      const long long j = (q0 + idx / pn) * a.np + p0 + idx % pn;
      if (j < a.m_max) out[j] = 0.0f;
    }
    return;
  }

  const T* x = static_cast<const T*>(a.waves) + (long long)b * a.sb;
  const long long base = q0 * a.op - a.width;      // the sample LDS slot 0 holds in chunk 0
  const int span = (a.qt - 1) * a.op + a.kc;
  auto stage = [&](int c) {      // xs[i] = xz[base + c kc + i]: float(v) per channel, summed in index order, / C, * scale
    const long long s0 = base + (long long)c * a.kc;
    for (int i = tid; i < span; i += THREADS) {
      const long long s = s0 + i;
      float v = 0.0f;
      if (s >= 0 && s < len) {
        const T* p = x + s * a.ss;
        float sum = (float)p[0];
        for (int ch = 1; ch < a.C; ++ch) sum += (float)p[ch * a.sc];
        v = sum / (float)a.C;
        v = v * a.scale;
      }
      xs[i] = v;
    }
  };

  const int lq = min(lane, a.qt - 1);      // (lanes past qt repeat the last super-stride and write nothing)
  const int rounds = (g1 - g0 + WAVES - 1) / WAVES;
  for (int r = 0; r < rounds; ++r) {
    const int g = g0 + r * WAVES + wave;
    const bool live = g < g1;      // (wave-uniform)
    int gfirst = 0, gcount = 0, goff = 0;
    if (live) {
      gfirst = groups[3 * g], gcount = groups[3 * g + 1], goff = groups[3 * g + 2];
      if (gfirst < 0 || gcount < 0 || goff < 0 || (gfirst | gcount) % TA || goff + gcount > a.tap_rows) gcount = 0;      // a broken table reads nothing
    }
    float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f, acc3 = 0.0f;
    for (int c = 0; c < a.nchunks; ++c) {
      if (r == 0 || a.nchunks > 1) {      // the common filter fits one chunk: staged once, read by every round
        if (r || c) __syncthreads();
        stage(c);
        __syncthreads();
      }
      if (live) {
        const int k_lo = max(gfirst, c * a.kc), k_hi = min(gfirst + gcount, (c + 1) * a.kc);      // (multiples of TA)
        const float* xp = xs + lq * a.op - c * a.kc;                                         // indexed by k
        const f32x4* tp = reinterpret_cast<const f32x4*>(taps) + (goff - gfirst);            // indexed by k
        for (int k = k_lo; k < k_hi; k += TA) {
#pragma unroll
          for (int u = 0; u < TA; ++u) {
            const f32x4 h = tp[k + u];
            const float s = xp[k + u];
            acc0 = fmaf(h[0], s, acc0);
            acc1 = fmaf(h[1], s, acc1);
            acc2 = fmaf(h[2], s, acc2);
            acc3 = fmaf(h[3], s, acc3);
          }
        }
      }
    }
    if (live && lane < a.qt) {
      const float acc[PG] = {acc0, acc1, acc2, acc3};
      const long long j0 = (q0 + lane) * a.np + PG * g;
#pragma unroll
      for (int e = 0; e < PG; ++e) {
        const long long j = j0 + e;
        if (PG * g + e < a.np && j < a.m_max) out[j] = j < mb ? acc[e] : 0.0f;
      }
    }
  }
}

}  // namespace

extern "C" int ufnd_resample(const void* waves, int dtype, long long stride_b, long long stride_c, long long stride_s, const int32_t* lengths,
                             const float* taps, const int32_t* groups, float* out, int32_t* out_lengths, int B, int C, int n_max, int o, int n, int G,
                             int width, int ngroups, int tap_rows, int qt, int kc, int nchunks, float scale, void* stream_) {
  UFND_REQUIRE(waves && taps && groups && out && out_lengths, "resample: null argument (waves, taps, groups, out, out_lengths)");
  UFND_REQUIRE(dtype == UFND_RESAMPLE_F32 || dtype == UFND_RESAMPLE_I16, "resample: dtype=%d (0: fp32, 1: int16)", dtype);
  UFND_REQUIRE(B >= 1 && B <= 65535 && C >= 1 && C <= 64 && n_max >= 1 && n_max <= (1 << 30),
               "resample: B=%d C=%d n_max=%d (1 <= B <= 65535 clips of 1 <= C <= 64 channels and 1 <= n_max <= 2^30 samples)", B, C, n_max);
  UFND_REQUIRE(o >= 1 && o <= UFND_RESAMPLE_MAX_RATIO_TERM && n >= 1 && n <= UFND_RESAMPLE_MAX_RATIO_TERM,
               "resample: o=%d n=%d (the reduced rate ratio: 1 .. %d each)", o, n, UFND_RESAMPLE_MAX_RATIO_TERM);
  UFND_REQUIRE(stride_b >= 0 && stride_c >= 0 && stride_s >= 0, "resample: negative stride");
  UFND_REQUIRE(G >= 1 && (long long)G * n <= 65536 && (long long)G * o <= (1 << 20), "resample: G=%d (G n <= 65536, G o <= 2^20)", G);
  const int np = G * n, op = G * o;
  UFND_REQUIRE(width >= 0 && ngroups == ufnd_cdiv(np, PG) && tap_rows >= 0, "resample: width=%d ngroups=%d tap_rows=%d (ngroups = ceil(G n / 4))", width,
               ngroups, tap_rows);
  UFND_REQUIRE(qt >= 1 && qt <= QT && kc >= TA && kc % TA == 0 && nchunks >= 1 && (long long)(qt - 1) * op + kc <= LDS_FLOATS,
               "resample: qt=%d kc=%d nchunks=%d (1 <= qt <= %d, kc a multiple of 8, (qt - 1) G o + kc <= %d floats of LDS)", qt, kc, nchunks, QT,
               LDS_FLOATS);
  const long long m_max = ((long long)n * n_max + o - 1) / o;
  const long long tiles = (m_max + (long long)qt * np - 1) / ((long long)qt * np);
  UFND_REQUIRE(m_max <= 0x7fffffffll && tiles <= 0x7fffffffll, "resample: %lld output samples per clip (at most 2^31 - 1)", m_max);
  UFND_REQUIRE(ufnd_aligned(taps, 16) && ufnd_aligned(waves, dtype == UFND_RESAMPLE_F32 ? 4 : 2), "resample: alignment (taps 16 bytes, waves its element)");
  // phase slices: more workgroups for few short clips; a slice keeps at least one group per wave
  int slices = (int)((TARGET_WORKGROUPS + tiles * B - 1) / (tiles * B));
  slices = slices > ngroups / WAVES ? ngroups / WAVES : slices;
  slices = slices < 1 ? 1 : slices;
  const int gps = ufnd_cdiv(ngroups, slices);
  slices = ufnd_cdiv(ngroups, gps);
  Geometry a;
  a.waves = waves, a.sb = stride_b, a.sc = stride_c, a.ss = stride_s, a.lengths = lengths, a.out_lengths = out_lengths;
  a.C = C, a.n_max = n_max, a.o = o, a.n = n, a.op = op, a.np = np, a.width = width, a.ngroups = ngroups, a.gps = gps, a.qt = qt, a.kc = kc;
  a.nchunks = nchunks, a.tap_rows = tap_rows, a.m_max = m_max, a.scale = scale;
  const dim3 grid((unsigned)tiles, (unsigned)B, (unsigned)slices);
  if (dtype == UFND_RESAMPLE_F32) {
    hipLaunchKernelGGL(resample_kernel<float>, grid, dim3(THREADS), 0, (hipStream_t)stream_, a, taps, groups, out);
  } else {
    hipLaunchKernelGGL(resample_kernel<int16_t>, grid, dim3(THREADS), 0, (hipStream_t)stream_, a, taps, groups, out);
  }
  UFND_CHECK_LAUNCH();
  return UFND_OK;
}
