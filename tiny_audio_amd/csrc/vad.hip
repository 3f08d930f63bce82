// ta355 voice activity detection: per-frame speech decisions of whole recordings from band-wise likelihood ratios against a
// minimum-statistics noise floor (include/ta355.h, "voice activity detection"; contract tests/vad_ref.py; DESIGN.md section 3, "Voice
// activity detection").  R recordings lie in one flat f32 buffer, recording r at samples offsets[r] .. offsets[r + 1] (n of them), at any
// sample offset; samples outside [0, n) of a recording are 0, whatever lies beside it in the buffer.  Its grid is the diarizer's: frame i
// for every i >= 0 with 256 i < n - 256, F = (n - 1) / 256 of them (0 for n <= 256).  Two launches, no atomics, nobody waits for another
// workgroup; every order below depends on nothing but n and the options, so two runs give the same bits and a recording gives the same
// bits alone as inside a batch.
//
// ---- 1 vad_energy_kernel, one workgroup per VAD_EF = 32 frames of one recording: E [R, ldE, 16] f32, rows of 64 bytes.
//    The workgroup's samples [256 i0 - 72, 256 (i0 + 31) + 328) are read once into LDS, 4 bytes per lane (a recording starts at any
//    sample).  Frame i is the 400 samples from 256 i - 72 times the periodic Hann window (one rounding).  Frames 2 j and 2 j + 1 ride
//    as the real and the imaginary part of one 400-point complex transform (fft400.h: 16-point transforms on 25 lanes, twiddles,
//    25-point transforms on 16 lanes; a wave carries two such pairs at a time), and come apart as
//      A[f] = (Z[f] + conj Z[400 - f]) / 2,   B[f] = (Z[f] - conj Z[400 - f]) / 2 i.
//    One lane per (frame, band b):
//      p[f]  = re^2 + im^2                                   (the product and the addition may contract into one fma)
//      E[b]  = (((((p[2 + 6 b] + p[3 + 6 b]) + p[4 + 6 b]) + p[5 + 6 b]) + p[6 + 6 b]) + p[7 + 6 b]) * (1 / 160000)      6 bins ascending
//    A non-finite sample makes every bin of its frame NaN, and of the frame that shares its transform.
//
// ---- 2 vad_stat_kernel, one workgroup per tile of VAD_TILE = 256 frames of one recording, a lane per frame.  The tile plus a halo of
//    W + h frames per side of E is staged in LDS, G bands at a time (G = 16 where that fits 64 KB, which the defaults do; 8, 4, 2 or 1
//    for a wide noise window: the bands are independent, so G changes no bit), band-major so that a wave reads consecutive frames.
//      S[j][b] = (E[lo][b] + E[lo + 1][b] + ... + E[hi][b]) / (hi - lo + 1),  lo = max(0, j - h), hi = min(F - 1, j + h)     ascending
//      N[i][b] = min S[j][b] over max(0, i - W) <= j <= min(F - 1, i + W)
//      g = (S + e0) / (beta N + e0);   t = (g - 1) - ln g where g > 1, NaN where g is NaN, else 0
//      L[i] = (((t[0] + t[1]) + t[2]) + ... + t[15]) / 16,   flag[i] = L[i] > theta                                       16 bands ascending
//    S lives in LDS as its bit pattern, -1 for a NaN: S >= +0 otherwise, so the signed-integer minimum is the float minimum, and a NaN
//    wins it and comes back as a NaN (all ones) -- fminf would drop it.  All zeros give S = N = 0, g = 1, L = 0 exactly.  Every barrier
//    sits under conditions uniform over the workgroup (F, the tile, the options).
#include "common.h"
#include "fft400.h"
#include "vad_tables.h"
#include "../../include/ta355.h"

#define VAD_T 256                                        // threads of both kernels
#define VAD_EF TA_VAD_ENERGY_FRAMES                      // frames per workgroup of the energy kernel
#define VAD_NFFT 400
#define VAD_SPAN ((VAD_EF - 1) * TA_VAD_HOP + VAD_NFFT)  // 8336 samples staged per workgroup
#define VAD_G 2                                          // frame pairs per wave at once
#define VAD_TILE TA_VAD_TILE
#define VAD_LDS_MAX 65536                                // dynamic LDS of the statistic kernel: no opt-in beyond 64 KB

static_assert(VAD_T == 256 && VAD_EF % (4 * 2 * VAD_G) == 0, "four waves, each 2 VAD_G frames per iteration");
static_assert(TA_VAD_BANDS * 2 * VAD_G == 64, "a lane per (frame, band) of a wave's iteration");
static_assert(TA_VAD_FIRST_BIN + TA_VAD_BANDS * TA_VAD_BAND_BINS <= VAD_NFFT / 2, "the bands stay below the Nyquist bin");
static_assert(VAD_TILE == VAD_T, "a lane per frame of the tile");
static_assert(TA_VAD_LEAD + TA_VAD_HOP / 2 == VAD_NFFT / 2, "the window is centred on the frame");

__host__ __device__ __forceinline__ long vad_frames(long n) { return n <= TA_VAD_HOP ? 0 : (n - 1) / TA_VAD_HOP; }

__global__ __launch_bounds__(VAD_T) void vad_energy_kernel(const float* __restrict__ wav, const long* __restrict__ offsets, long max_n,
                                                           float* __restrict__ E, long ldE) {
  __shared__ float span[VAD_SPAN];
  __shared__ float win[VAD_NFFT], tw[2 * VAD_NFFT];
  __shared__ __attribute__((aligned(16))) float scr[VAD_T / 64][VAD_G * VAD_NFFT * 2];
  const int r = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long o = offsets[r], n = offsets[r + 1] - o;
  if (n <= TA_VAD_HOP || n > max_n) return;              // no frame, or refused: nothing is written (uniform, before any barrier)
  const int F = (int)vad_frames(n);                       // <= ldE: the host checked max_n
  const int i0 = blockIdx.x * VAD_EF;
  if (i0 >= F) return;
  const float* x = wav + o;
  const long s0 = (long)i0 * TA_VAD_HOP - TA_VAD_LEAD;
  for (int q = tid; q < VAD_SPAN; q += VAD_T) {
    const long i = s0 + q;
    span[q] = (i >= 0 && i < n) ? x[i] : 0.f;
  }
  for (int j = tid; j < VAD_NFFT; j += VAD_T) win[j] = VAD_HANN[j];
  for (int j = tid; j < 2 * VAD_NFFT; j += VAD_T) tw[j] = VAD_TW400[j];
  __syncthreads();                                        // the only workgroup barrier: the waves go their own way from here
  float* my = scr[wave];
  float* Eo = E + (long)r * ldE * TA_VAD_BANDS;
  for (int it = 0; it < VAD_EF / (8 * VAD_G); ++it) {
    const int l0 = (it * 4 + wave) * 2 * VAD_G;           // this wave's first frame of the iteration, counted from i0
    if (i0 + l0 >= F) break;                              // wave-uniform
    // ---- stage A: lane = (pair g, n2), the 16-point transforms over n1 (sample j = 25 n1 + n2)
    if (lane < VAD_G * 25) {
      const int g = lane / 25, n2 = lane - g * 25;
      const int la = l0 + 2 * g;
      const bool va = i0 + la < F, vb = i0 + la + 1 < F;
      const float* fa = span + la * TA_VAD_HOP;           // la + 1 <= VAD_EF - 1: both frames lie inside the span
      cpx a[16];
#pragma unroll
      for (int n1 = 0; n1 < 16; ++n1) {
        const int j = 25 * n1 + n2;
        const float wv = win[j];
        a[n1].re = va ? fa[j] * wv : 0.f;
        a[n1].im = vb ? fa[TA_VAD_HOP + j] * wv : 0.f;
      }
      fft16(a);
      float* dst = my + ((g * 16) * 25 + n2) * 2;
#pragma unroll
      for (int k1 = 0; k1 < 16; ++k1) {
        cpx v = a[k1];
        if (k1 > 0) {
          const int j = n2 * k1;                          // < 400
          v = cmul(v, tw[2 * j], tw[2 * j + 1]);
        }
        *(float2*)(dst + k1 * 50) = make_float2(v.re, v.im);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // ---- stage B: lane = (pair g, k1), the 25-point transforms over n2; bin k = k1 + 16 k2
    if (lane < VAD_G * 16) {
      const int g = lane >> 4, k1 = lane & 15;
      const float* src = my + ((g * 16 + k1) * 25) * 2;
      cpx y[25];
#pragma unroll
      for (int n2 = 0; n2 < 25; ++n2) { const float2 v = *(const float2*)(src + 2 * n2); y[n2] = {v.x, v.y}; }
      fft25(y);                                           // (every active lane holds its inputs: in-order LDS per wave)
      float* dst = my + (g * VAD_NFFT + k1) * 2;
#pragma unroll
      for (int k2 = 0; k2 < 25; ++k2) *(float2*)(dst + 32 * k2) = make_float2(y[k2].re, y[k2].im);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // ---- bands: lane = (frame f of the iteration, band b); frame f is the real (f even) or imaginary (f odd) part of pair f / 2
    {
      const int f = lane >> 4, b = lane & 15;
      const float* Z = my + (f >> 1) * VAD_NFFT * 2;
      const bool second = f & 1;
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < TA_VAD_BAND_BINS; ++j) {
        const int k = TA_VAD_FIRST_BIN + TA_VAD_BAND_BINS * b + j;
        const float2 z = *(const float2*)(Z + 2 * k), c = *(const float2*)(Z + 2 * (VAD_NFFT - k));
        const float re = second ? 0.5f * (z.y + c.y) : 0.5f * (z.x + c.x);
        const float im = second ? 0.5f * (c.x - z.x) : 0.5f * (z.y - c.y);
        const float p = re * re + im * im;
        s = j == 0 ? p : s + p;
      }
      const int i = i0 + l0 + f;
      if (i < F) Eo[(long)i * TA_VAD_BANDS + b] = s * (1.0f / ((float)VAD_NFFT * (float)VAD_NFFT));
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();                      // the next iteration overwrites the scratch
  }
}

__global__ __launch_bounds__(VAD_T) void vad_stat_kernel(const long* __restrict__ offsets, long max_n, const float* __restrict__ E, long ldE,
                                                         int h, int W, float beta, float theta, float e0, int lgG, int NFp, int NSp,
                                                         float* __restrict__ stat, unsigned char* __restrict__ flags, long ld,
                                                         int* __restrict__ n_frames) {
  extern __shared__ __attribute__((aligned(16))) float vad_lds[];
  const int r = blockIdx.y, tid = threadIdx.x, G = 1 << lgG;
  const long n = offsets[r + 1] - offsets[r];
  if (n < 0 || n > max_n) {                               // refused (uniform): no row
    if (blockIdx.x == 0 && tid == 0) n_frames[r] = -1;
    return;
  }
  const int F = (int)vad_frames(n);
  if (blockIdx.x == 0 && tid == 0) n_frames[r] = F;
  const int i0 = blockIdx.x * VAD_TILE;
  if (i0 >= F) return;
  float* El = vad_lds;                                    // [G][NFp]: E of frames e_lo .. e_lo + NF - 1
  int* Sk = (int*)(vad_lds + G * NFp);                    // [G][NSp]: S of frames s_lo .. s_lo + NS - 1, as bits (-1: NaN)
  const int NF = VAD_TILE + 2 * (W + h), NS = VAD_TILE + 2 * W;
  const int e_lo = i0 - W - h, s_lo = i0 - W;
  const float* Er = E + (long)r * ldE * TA_VAD_BANDS;
  const int i = i0 + tid;
  const bool live = i < F;
  const int m_lo = (i - W > 0 ? i - W : 0) - s_lo, m_hi = (i + W < F - 1 ? i + W : F - 1) - s_lo;
  float acc = 0.f;
  for (int g0 = 0; g0 < TA_VAD_BANDS; g0 += G) {
    for (int idx = tid; idx < NF * G; idx += VAD_T) {
      const int e = idx >> lgG, b = idx & (G - 1), j = e_lo + e;
      El[b * NFp + e] = (j >= 0 && j < F) ? Er[(long)j * TA_VAD_BANDS + g0 + b] : 0.f;
    }
    __syncthreads();
    for (int b = 0; b < G; ++b)
      for (int jj = tid; jj < NS; jj += VAD_T) {
        const int j = s_lo + jj;
        if (j < 0 || j >= F) continue;
        const int lo = j - h > 0 ? j - h : 0, hi = j + h < F - 1 ? j + h : F - 1;
        const float* p = El + b * NFp + (lo - e_lo);
        float s = p[0];
        for (int q = 1; q <= hi - lo; ++q) s += p[q];
        s = s / (float)(hi - lo + 1);
        Sk[b * NSp + jj] = s != s ? -1 : __float_as_int(s);
      }
    __syncthreads();
    if (live)
      for (int b = 0; b < G; ++b) {
        const int* p = Sk + b * NSp;
        int m = p[m_lo];
        for (int q = m_lo + 1; q <= m_hi; ++q) m = min(m, p[q]);
        const float S = __int_as_float(p[tid + W]), N = __int_as_float(m);
        const float g = (S + e0) / (beta * N + e0);
        float t = 0.f;
        if (g > 1.0f) t = (g - 1.0f) - logf(g);
        else if (g != g) t = g;
        acc += t;
      }
    __syncthreads();                                      // the next group of bands overwrites both arrays
  }
  if (live) {
    const float L = acc * (1.0f / TA_VAD_BANDS);
    stat[(long)r * ld + i] = L;
    flags[(long)r * ld + i] = L > theta ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
namespace {
bool vad_max_n_ok(long max_n) { return max_n >= 1 && max_n <= (long)TA_CUT_HOP * TA_CUT_MAX_POSITIONS; }
bool vad_options_ok(const ta_vad_options* o) {
  return o && o->smooth >= 0 && o->smooth <= TA_VAD_MAX_SMOOTH && o->noise_window >= 1 && o->noise_window <= TA_VAD_MAX_NOISE_WINDOW &&
         o->noise_bias >= 1.f && o->noise_bias < INFINITY && o->threshold > 0.f && o->threshold < INFINITY && o->floor > 0.f &&
         o->floor < INFINITY;
}
}  // namespace

extern "C" long ta_vad_frames(long n) { return vad_frames(n); }

extern "C" long ta_vad_workspace_bytes(int R, long max_n) {
  if (R <= 0 || R > TA_CUT_MAX_RECORDINGS || !vad_max_n_ok(max_n)) return 0;
  return (long)R * vad_frames(max_n) * TA_VAD_BANDS * (long)sizeof(float);
}

extern "C" int ta_vad_f32(const float* wav, const long* offsets, int R, long max_n, const ta_vad_options* opt, float* stat,
                          unsigned char* flags, long ld, int* n_frames, void* ws, long ws_bytes, hipStream_t st) {
  if (R < 0 || R > TA_CUT_MAX_RECORDINGS || !vad_options_ok(opt)) return TA_ERR_ARG;
  if (R == 0) return TA_OK;
  if (!vad_max_n_ok(max_n) || !wav || !offsets || !n_frames) return TA_ERR_ARG;
  const long maxF = vad_frames(max_n), need = ta_vad_workspace_bytes(R, max_n);
  if (ld < maxF) return TA_ERR_ARG;
  if (maxF > 0 && (!stat || !flags || !ws || ws_bytes < need)) return TA_ERR_ARG;
  float* E = (float*)ws;
  const int h = opt->smooth, W = opt->noise_window;
  const int NFp = (VAD_TILE + 2 * (W + h)) | 1, NSp = (VAD_TILE + 2 * W) | 1;      // odd rows: the staging writes spread over the banks
  int lgG = 4;
  while (lgG > 0 && (long)sizeof(float) * (NFp + NSp) * (1L << lgG) > VAD_LDS_MAX) --lgG;
  const unsigned lds = (unsigned)(sizeof(float) * (NFp + NSp)) << lgG;
  if (lds > VAD_LDS_MAX) return TA_ERR_ARG;                // (unreachable within the option ranges: one band needs 18.5 KB at most)
  if (maxF > 0) {
    TA_LAUNCH(vad_energy_kernel, dim3((unsigned)((maxF + VAD_EF - 1) / VAD_EF), R), dim3(VAD_T), 0, st, wav, offsets, max_n, E, maxF);
    TA_CHECK_LAUNCH();
  }
  const unsigned tiles = maxF > 0 ? (unsigned)((maxF + VAD_TILE - 1) / VAD_TILE) : 1u;      // tile 0 also writes n_frames
  TA_LAUNCH(vad_stat_kernel, dim3(tiles, R), dim3(VAD_T), lds, st, offsets, max_n, E, maxF, h, W, opt->noise_bias, opt->threshold,
            opt->floor, lgG, NFp, NSp, stat, flags, ld, n_frames);
  TA_CHECK_LAUNCH();
  return TA_OK;
}
