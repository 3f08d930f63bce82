// ta355 device-side waveform augmentation: the numeric stages of the reference's production recipe that sit between the raw
// audio and the log-mel (configs/training/production.yaml:67-140; tiny_audio/augmentation.py:71-223, wired at
// scripts/train.py:530-587), in the reference's order: RIR convolution, background noise at an SNR, Gaussian floor at an SNR,
// percentile clipping.  The reference runs them in CPU dataloader workers through audiomentations; here the waveforms [B, Ls] are
// already on the device when they would run.  The semantics are defined by tests/augment_ref.py (float64 numpy).
//
// Every stage acts on clip b over [0, n), n = lens[b]; a stage that is off for a clip leaves the clip untouched.
//
// ---- RIR convolution: uniformly partitioned overlap-save, f32, hop H = 2048, complex FFT of N = 2 H = 4096 points held in LDS.
//   * the twiddles exp(-2 pi i k / N) are rounded once from float64 (ta_wave_fft_twiddles) and staged into LDS by every workgroup;
//   * the forward transform is decimation in frequency (natural order in, bit-reversed out), the inverse decimation in time
//     (bit-reversed in, natural out), so no transform ever permutes: spectra live in memory in bit-reversed order, and products of
//     spectra do not care;
//   * the inputs are real, so a spectrum is stored as N/2 + 1 bins: bins 0 .. N/2 - 1 are the EVEN positions of the bit-reversed
//     array (bin k at position 2 rev11(k)), bin N/2 is position 1; the inverse rebuilds bin N - k as conj(bin k);
//   * impulse-response partition p (taps [p H, (p + 1) H), zero padded to N) is transformed once per pool (ta_wave_ir_spectra);
//   * input block j of a clip is the window [(j - 1) H, (j + 1) H) (zero outside [0, n)), transformed once into the workspace;
//   * output block o = samples [o H, (o + 1) H) = the last H points of IFFT(sum_p X[o - p] H[p]);  every block of the FULL
//     convolution [0, n + m - 1) is formed (the peak may lie in the tail that is not kept) and leaves its maximum |y|;
//   * the finishing pass reduces a clip's block maxima to the peak P and writes  y * rir_peak / P  on [0, n) -- or the plain
//     copy of the input for a clip without an impulse response.
//   LDS: 32 KB data + 16 KB twiddles per 256-thread workgroup = 3 workgroups per CU (160 KB), 12 waves.
//   * a clip or a response of at most WA_DIRECT = 32 samples takes the direct form instead: each sample of the full convolution is a
//     sum of <= 32 products, formed in double (the products of two floats are exact there) and rounded once.  That is less work per
//     sample than three 4096-point transforms, and it is what a single-transform f32 reference does not beat: scipy.signal.fftconvolve
//     multiplies directly when an input has one sample, so on such inputs only a correctly rounded result stays within a small
//     multiple of its error.  The direct clips use neither the spectra nor the workspace's X / yraw; their block maxima go through
//     the same bmax list (held in double, so that the scale of a direct clip is not rounded through f32).
#include "common.h"
#include "philox.h"

#define WA_N 4096
#define WA_H 2048
#define WA_LOGN 12
#define WA_BINS (WA_N / 2 + 1)
#define WA_T 256
#define WA_E (WA_N / 2 / WA_T)          // butterflies (and stored bins) per thread: 8
#define WA_DIRECT 32                    // min(n, m) <= this: direct form in double

__device__ __forceinline__ float2 wa_cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 wa_cmulc(float2 a, float2 b) { return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }   // a conj(b)

// s[N] natural order -> bit-reversed order.  Ends with a barrier.
__device__ __forceinline__ void wa_fft_fwd(float2* s, const float2* tw) {
  for (int lh = WA_LOGN - 1; lh >= 0; --lh) {
    const int half = 1 << lh;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < WA_E; ++e) {
      const int j = threadIdx.x + e * WA_T, pos = j & (half - 1);
      const int i0 = ((j >> lh) << (lh + 1)) + pos, i1 = i0 + half;
      const float2 a = s[i0], b = s[i1], w = tw[pos << (WA_LOGN - 1 - lh)];
      s[i0] = make_float2(a.x + b.x, a.y + b.y);
      s[i1] = wa_cmul(make_float2(a.x - b.x, a.y - b.y), w);
    }
  }
  __syncthreads();
}
// s[N] bit-reversed order -> natural order, scaled by N.  Ends with a barrier.
__device__ __forceinline__ void wa_fft_inv(float2* s, const float2* tw) {
  for (int lh = 0; lh < WA_LOGN; ++lh) {
    const int half = 1 << lh;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < WA_E; ++e) {
      const int j = threadIdx.x + e * WA_T, pos = j & (half - 1);
      const int i0 = ((j >> lh) << (lh + 1)) + pos, i1 = i0 + half;
      const float2 a = s[i0], b = wa_cmulc(s[i1], tw[pos << (WA_LOGN - 1 - lh)]);
      s[i0] = make_float2(a.x + b.x, a.y + b.y);
      s[i1] = make_float2(a.x - b.x, a.y - b.y);
    }
  }
  __syncthreads();
}
__device__ __forceinline__ void wa_stage_twiddles(float2* tws, const float2* __restrict__ tw) {
  for (int i = threadIdx.x; i < WA_N / 2; i += WA_T) tws[i] = tw[i];
}
// the N/2 + 1 stored bins of a transformed block: S[q] = position 2 q (bin rev11(q)), S[N/2] = position 1 (bin N/2)
__device__ __forceinline__ void wa_store_spectrum(const float2* s, float2* __restrict__ S) {
#pragma unroll
  for (int e = 0; e < WA_E; ++e) { const int q = threadIdx.x + e * WA_T; S[q] = s[2 * q]; }
  if (threadIdx.x == 0) S[WA_N / 2] = s[1];
}
__device__ __forceinline__ long wa_clip_len(const long* lens, int b, int Ls) {
  const long n = lens[b];
  return n < 0 ? 0 : (n > Ls ? Ls : n);
}

__device__ __forceinline__ bool wa_direct(long n, long m) { return n <= WA_DIRECT || m <= WA_DIRECT; }
// sample t of the full convolution of x[0, n) with h[0, m), min(n, m) <= WA_DIRECT: the loop runs over the shorter of the two
__device__ __forceinline__ double wa_direct_at(const float* __restrict__ x, long n, const float* __restrict__ h, long m, long t) {
  const float* s = m <= n ? h : x;      // the short one, indexed by k; the long one by t - k
  const float* l = m <= n ? x : h;
  const long ns = m <= n ? m : n, nl = m <= n ? n : m;
  const long k_lo = t - (nl - 1) > 0 ? t - (nl - 1) : 0, k_hi = t < ns - 1 ? t : ns - 1;
  double a = 0.0;
  for (long k = k_lo; k <= k_hi; ++k) a = fma((double)s[k], (double)l[t - k], a);
  return a;
}
__device__ __forceinline__ double wa_wave_maxd(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ __launch_bounds__(WA_T) void wave_twiddle_kernel(float2* __restrict__ tw) {
  const int k = blockIdx.x * WA_T + threadIdx.x;
  if (k >= WA_N / 2) return;
  double sn, cs;
  sincospi(-2.0 * (double)k / (double)WA_N, &sn, &cs);
  tw[k] = make_float2((float)cs, (float)sn);
}

// grid (max_parts, n_ir): partition p of impulse response r
__global__ __launch_bounds__(WA_T) void wave_ir_fft_kernel(const float* __restrict__ ir, const long* __restrict__ ir_off,
                                                           const int* __restrict__ part_off, const float2* __restrict__ tw,
                                                           float2* __restrict__ spectra) {
  __shared__ float2 s[WA_N];
  __shared__ float2 tws[WA_N / 2];
  const int r = blockIdx.y, p = blockIdx.x;
  const long m = ir_off[r + 1] - ir_off[r];
  if (p >= part_off[r + 1] - part_off[r]) return;
  const float* h = ir + ir_off[r] + (long)p * WA_H;
  const long left = m - (long)p * WA_H;
  for (int i = threadIdx.x; i < WA_N; i += WA_T) s[i] = make_float2((i < WA_H && i < left) ? h[i] : 0.f, 0.f);
  wa_stage_twiddles(tws, tw);
  wa_fft_fwd(s, tws);
  wa_store_spectrum(s, spectra + (long)(part_off[r] + p) * WA_BINS);
}

// grid (nbx_max, B): input block j of clip b
__global__ __launch_bounds__(WA_T) void wave_block_fft_kernel(const float* __restrict__ wav, const long* __restrict__ lens,
                                                              const int* __restrict__ ir_idx, int n_ir,
                                                              const long* __restrict__ ir_off, int Ls, int nbx_max,
                                                              const float2* __restrict__ tw, float2* __restrict__ X) {
  __shared__ float2 s[WA_N];
  __shared__ float2 tws[WA_N / 2];
  const int b = blockIdx.y, j = blockIdx.x, r = ir_idx[b];
  if (r < 0 || r >= n_ir) return;
  const long n = wa_clip_len(lens, b, Ls);
  if (n <= 0 || j >= (n - 1) / WA_H + 2 || wa_direct(n, ir_off[r + 1] - ir_off[r])) return;
  const float* x = wav + (long)b * Ls;
  const long base = (long)(j - 1) * WA_H;
  for (int i = threadIdx.x; i < WA_N; i += WA_T) { const long t = base + i; s[i] = make_float2((t >= 0 && t < n) ? x[t] : 0.f, 0.f); }
  wa_stage_twiddles(tws, tw);
  wa_fft_fwd(s, tws);
  wa_store_spectrum(s, X + ((long)b * nbx_max + j) * WA_BINS);
}

// grid (nout_max, B): output block o of clip b -> yraw[b, o H .. ) (kept part only) and bmax[b, o]; of a direct clip bmax alone
__global__ __launch_bounds__(WA_T) void wave_conv_block_kernel(const float* __restrict__ wav, const long* __restrict__ lens,
                                                               const int* __restrict__ ir_idx, int n_ir, const float* __restrict__ ir,
                                                               const long* __restrict__ ir_off, const int* __restrict__ part_off, int Ls,
                                                               int nbx_max, int nout_max, const float2* __restrict__ tw,
                                                               const float2* __restrict__ X, const float2* __restrict__ Hs,
                                                               float* __restrict__ yraw, double* __restrict__ bmax) {
  __shared__ float2 s[WA_N];
  __shared__ float2 tws[WA_N / 2];
  __shared__ double red[WA_T / 64];
  const int b = blockIdx.y, o = blockIdx.x, r = ir_idx[b];
  if (r < 0 || r >= n_ir) return;
  const long n = wa_clip_len(lens, b, Ls);
  if (n <= 0) return;
  const long m = ir_off[r + 1] - ir_off[r], Lf = n + m - 1;
  if ((long)o * WA_H >= Lf) return;
  if (wa_direct(n, m)) {
    const float *x = wav + (long)b * Ls, *h = ir + ir_off[r];
    double dmx = 0.0;
    for (int i = threadIdx.x; i < WA_H; i += WA_T) {
      const long t = (long)o * WA_H + i;
      if (t < Lf) dmx = fmax(dmx, fabs(wa_direct_at(x, n, h, m, t)));
    }
    dmx = wa_wave_maxd(dmx);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = dmx;
    __syncthreads();
    if (threadIdx.x == 0) bmax[(long)b * nout_max + o] = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    return;
  }
  const int P = part_off[r + 1] - part_off[r], nbx = (int)((n - 1) / WA_H) + 2;
  const int p_lo = o - (nbx - 1) > 0 ? o - (nbx - 1) : 0, p_hi = o < P - 1 ? o : P - 1;
  float2 acc[WA_E], accn = make_float2(0.f, 0.f);
#pragma unroll
  for (int e = 0; e < WA_E; ++e) acc[e] = make_float2(0.f, 0.f);
  for (int p = p_lo; p <= p_hi; ++p) {
    const float2* Xp = X + ((long)b * nbx_max + (o - p)) * WA_BINS;
    const float2* Hp = Hs + (long)(part_off[r] + p) * WA_BINS;
#pragma unroll
    for (int e = 0; e < WA_E; ++e) {
      const int q = threadIdx.x + e * WA_T;
      const float2 v = wa_cmul(Xp[q], Hp[q]);
      acc[e].x += v.x; acc[e].y += v.y;
    }
    if (threadIdx.x == 0) { const float2 v = wa_cmul(Xp[WA_N / 2], Hp[WA_N / 2]); accn.x += v.x; accn.y += v.y; }
  }
#pragma unroll
  for (int e = 0; e < WA_E; ++e) {
    const int q = threadIdx.x + e * WA_T;
    const unsigned k = __brev((unsigned)q) >> (32 - (WA_LOGN - 1));             // the bin at even position 2 q
    s[2 * q] = acc[e];
    if (k != 0) s[__brev((unsigned)WA_N - k) >> (32 - WA_LOGN)] = make_float2(acc[e].x, -acc[e].y);   // bin N - k = conj(bin k)
  }
  if (threadIdx.x == 0) s[1] = accn;
  wa_stage_twiddles(tws, tw);
  wa_fft_inv(s, tws);
  float mx = 0.f;
  float* y = yraw + (long)b * Ls;
  for (int i = threadIdx.x; i < WA_H; i += WA_T) {
    const long t = (long)o * WA_H + i;
    const float v = s[WA_H + i].x * (1.0f / WA_N);
    if (t < Lf) mx = fmaxf(mx, fabsf(v));
    if (t < n) y[t] = v;
  }
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = (double)mx;
  __syncthreads();
  if (threadIdx.x == 0) bmax[(long)b * nout_max + o] = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// grid (cdiv(Ls, 1024), B): the only pass that writes `out` -- the scaled convolution, or the copy
__global__ __launch_bounds__(WA_T) void wave_conv_finish_kernel(const float* __restrict__ wav, const long* __restrict__ lens,
                                                                const int* __restrict__ ir_idx, int n_ir, const float* __restrict__ ir,
                                                                const long* __restrict__ ir_off, int Ls, int nout_max,
                                                                const float* __restrict__ yraw, const double* __restrict__ bmax,
                                                                float rir_peak, float* __restrict__ out) {
  const int b = blockIdx.y;
  const long n = wa_clip_len(lens, b, Ls);
  const int r = ir_idx ? ir_idx[b] : -1;
  const bool conv = r >= 0 && r < n_ir && n > 0;
  double scale = 1.0;                 // applied in double and rounded once: a sample equal to the peak comes out as rir_peak exactly
  long m = 0;
  if (conv) {
    m = ir_off[r + 1] - ir_off[r];
    const long Lf = n + m - 1;
    long nout = (Lf + WA_H - 1) / WA_H;
    if (nout > nout_max) nout = nout_max;
    double P = 0.0;
    for (int o = 0; o < nout; ++o) P = fmax(P, bmax[(long)b * nout_max + o]);      // uniform loads: every thread walks the same list
    if (rir_peak > 0.f && P > 0.0) scale = (double)rir_peak / P;
  }
  const bool direct = conv && wa_direct(n, m);
  const float *x = wav + (long)b * Ls, *src = (conv ? yraw : wav) + (long)b * Ls, *h = conv ? ir + ir_off[r] : nullptr;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const long t = (long)blockIdx.x * 1024 + e * WA_T + threadIdx.x;
    if (t >= Ls) continue;
    float v = 0.f;
    if (t < n) v = direct ? (float)(wa_direct_at(x, n, h, m, t) * scale) : conv ? (float)((double)src[t] * scale) : src[t];
    out[(long)b * Ls + t] = v;
  }
}

namespace {
inline long wa_nbx_max(int Ls) { return Ls > 0 ? (Ls - 1) / WA_H + 2 : 0; }
inline long wa_nout_max(int Ls, int max_taps) { return ((long)Ls + max_taps - 1 + WA_H - 1) / WA_H; }
inline size_t wa_align(size_t x) { return (x + 255) & ~(size_t)255; }
}  // namespace

extern "C" int ta_wave_fft_twiddles(float* tw, hipStream_t st) {
  if (!tw) return TA_ERR_ARG;
  TA_LAUNCH(wave_twiddle_kernel, dim3(WA_N / 2 / WA_T), dim3(WA_T), 0, st, (float2*)tw);
  TA_CHECK_LAUNCH();
  return TA_OK;
}

extern "C" int ta_wave_ir_spectra(const float* ir, const long* ir_off, const int* part_off, int n_ir, int max_parts, const float* tw,
                                  float* spectra, hipStream_t st) {
  if (n_ir <= 0 || max_parts <= 0) return TA_OK;
  if (!ir || !ir_off || !part_off || !tw || !spectra || max_parts > 65535 || n_ir > 65535) return TA_ERR_ARG;
  TA_LAUNCH(wave_ir_fft_kernel, dim3(max_parts, n_ir), dim3(WA_T), 0, st, ir, ir_off, part_off, (const float2*)tw, (float2*)spectra);
  TA_CHECK_LAUNCH();
  return TA_OK;
}

extern "C" long ta_wave_conv_ws_bytes(int B, int Ls, int max_taps) {
  if (B <= 0 || Ls <= 0 || max_taps <= 0) return 0;
  return (long)(wa_align((size_t)B * wa_nbx_max(Ls) * WA_BINS * sizeof(float2)) + wa_align((size_t)B * Ls * sizeof(float)) +
                wa_align((size_t)B * wa_nout_max(Ls, max_taps) * sizeof(double)));
}

extern "C" int ta_wave_conv_f32(const float* wav, const long* lens, int B, int Ls, const int* ir_idx, const float* ir, const long* ir_off,
                                const int* part_off, int n_ir, int max_taps, const float* tw, const float* spectra, float rir_peak,
                                float* out, void* ws, long ws_bytes, hipStream_t st) {
  if (B <= 0 || Ls <= 0) return TA_OK;
  if (!wav || !lens || !out || wav == out || B > 65535) return TA_ERR_ARG;
  const bool conv = ir_idx && n_ir > 0;
  float* yraw = nullptr;
  double* bmax = nullptr;
  const int nout_max = conv ? (int)wa_nout_max(Ls, max_taps) : 0;
  if (conv) {
    if (!ir || !ir_off || !part_off || !tw || !spectra || !ws || max_taps <= 0 || ws_bytes < ta_wave_conv_ws_bytes(B, Ls, max_taps) ||
        nout_max > 65535)
      return TA_ERR_ARG;
    const int nbx_max = (int)wa_nbx_max(Ls);
    float2* X = (float2*)ws;
    yraw = (float*)((char*)ws + wa_align((size_t)B * nbx_max * WA_BINS * sizeof(float2)));
    bmax = (double*)((char*)yraw + wa_align((size_t)B * Ls * sizeof(float)));
    TA_LAUNCH(wave_block_fft_kernel, dim3(nbx_max, B), dim3(WA_T), 0, st, wav, lens, ir_idx, n_ir, ir_off, Ls, nbx_max, (const float2*)tw, X);
    TA_CHECK_LAUNCH();
    TA_LAUNCH(wave_conv_block_kernel, dim3(nout_max, B), dim3(WA_T), 0, st, wav, lens, ir_idx, n_ir, ir, ir_off, part_off, Ls,
              nbx_max, nout_max, (const float2*)tw, (const float2*)X, (const float2*)spectra, yraw, bmax);
    TA_CHECK_LAUNCH();
  }
  TA_LAUNCH(wave_conv_finish_kernel, dim3(ta_cdiv(Ls, 1024), B), dim3(WA_T), 0, st, wav, lens, conv ? ir_idx : nullptr, n_ir, ir, ir_off, Ls,
            nout_max, yraw, bmax, rir_peak, out);
  TA_CHECK_LAUNCH();
  return TA_OK;
}

// ---- background noise + Gaussian floor.  Three launches over (chunk of 4096 samples, clip); the per-clip sums of squares go
// through per-chunk partials (f32 tree inside a chunk, the <= 118 chunk partials of a clip summed in one fixed order in double by
// whoever needs them), so nothing depends on the order in which workgroups run and there are no atomics.
//   partial[b][c] = {sum x^2, sum v^2, sum y^2} of chunk c  (x: the input, v: the noise window, y: after the background stage)
// noise_amp[b] = 10^(-snr / 20) of the background stage (read when noise_idx[b] >= 0); gauss_amp[b] the same for the Gaussian stage,
// <= 0 = off.  The Gaussian draws: see philox.h.
#define WM_CHUNK 4096
#define WM_G (WM_CHUNK / 4 / WA_T)      // groups of 4 consecutive samples per thread: 4

__device__ __forceinline__ float wm_block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
struct WmClip {
  long n, nlen, nstart;
  const float* v;      // the noise clip, or nullptr when the background stage is off for this clip
  bool gauss;
};
__device__ __forceinline__ WmClip wm_clip(const long* lens, int b, int Ls, const int* noise_idx, const long* noise_start,
                                          const float* noise, const long* noise_off, int n_noise, const float* gauss_amp) {
  WmClip c;
  c.n = wa_clip_len(lens, b, Ls);
  c.v = nullptr; c.nlen = 0; c.nstart = 0;
  const int j = noise_idx ? noise_idx[b] : -1;
  if (j >= 0 && j < n_noise) {
    c.nlen = noise_off[j + 1] - noise_off[j];
    if (c.nlen > 0) {
      c.v = noise + noise_off[j];
      c.nstart = ((noise_start[b] % c.nlen) + c.nlen) % c.nlen;
    }
  }
  c.gauss = gauss_amp && gauss_amp[b] > 0.f;
  return c;
}
__device__ __forceinline__ double wm_total(const float* partial, int nchunk_b, int which) {
  double t = 0.0;
  for (int c = 0; c < nchunk_b; ++c) t += (double)partial[c * 3 + which];
  return t;
}

__global__ __launch_bounds__(WA_T) void wave_mix_sums_kernel(const float* __restrict__ wav, const long* __restrict__ lens, int Ls,
                                                             const int* __restrict__ noise_idx, const long* __restrict__ noise_start,
                                                             const float* __restrict__ noise, const long* __restrict__ noise_off,
                                                             int n_noise, const float* __restrict__ gauss_amp, int nchunk,
                                                             float* __restrict__ partial) {
  __shared__ float red[WA_T / 64];
  const int b = blockIdx.y;
  const WmClip c = wm_clip(lens, b, Ls, noise_idx, noise_start, noise, noise_off, n_noise, gauss_amp);
  const long t0 = (long)blockIdx.x * WM_CHUNK;
  if ((!c.v && !c.gauss) || t0 >= c.n) return;
  const float* x = wav + (long)b * Ls;
  float sx = 0.f, sv = 0.f;
#pragma unroll
  for (int g = 0; g < WM_G; ++g) {
    const long tg = t0 + 4 * (threadIdx.x + g * WA_T);
    long iv = (c.v && tg < c.n) ? (c.nstart + tg) % c.nlen : 0;      // one division per 4 samples; the window wraps by increment
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long t = tg + i;
      if (t < c.n) {
        const float xv = x[t];
        sx += xv * xv;
        if (c.v) { const float vv = c.v[iv]; sv += vv * vv; iv = iv + 1 == c.nlen ? 0 : iv + 1; }
      }
    }
  }
  sx = wm_block_sum(sx, red);
  sv = wm_block_sum(sv, red);
  if (threadIdx.x == 0) {
    float* p = partial + ((long)b * nchunk + blockIdx.x) * 3;
    p[0] = sx; p[1] = sv; p[2] = sx;
  }
}

__global__ __launch_bounds__(WA_T) void wave_mix_bg_kernel(float* __restrict__ wav, const long* __restrict__ lens, int Ls,
                                                           const int* __restrict__ noise_idx, const long* __restrict__ noise_start,
                                                           const float* __restrict__ noise_amp, const float* __restrict__ noise,
                                                           const long* __restrict__ noise_off, int n_noise, int nchunk,
                                                           float* __restrict__ partial) {
  __shared__ float red[WA_T / 64];
  const int b = blockIdx.y;
  const WmClip c = wm_clip(lens, b, Ls, noise_idx, noise_start, noise, noise_off, n_noise, nullptr);
  const long t0 = (long)blockIdx.x * WM_CHUNK;
  if (!c.v || t0 >= c.n) return;
  float* pb = partial + (long)b * nchunk * 3;
  const int ncb = (int)((c.n + WM_CHUNK - 1) / WM_CHUNK);
  const double sx = wm_total(pb, ncb, 0), sv = wm_total(pb, ncb, 1);
  if (sqrt(sv / (double)c.n) < 1e-9) return;                 // a silent noise window: the stage is skipped
  const float g = (float)(sqrt(sx / sv) * (double)noise_amp[b]);
  float* x = wav + (long)b * Ls;
  float sy = 0.f;
#pragma unroll
  for (int gq = 0; gq < WM_G; ++gq) {
    const long tg = t0 + 4 * (threadIdx.x + gq * WA_T);
    long iv = tg < c.n ? (c.nstart + tg) % c.nlen : 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long t = tg + i;
      if (t < c.n) {
        const float y = x[t] + g * c.v[iv];
        iv = iv + 1 == c.nlen ? 0 : iv + 1;
        x[t] = y;
        sy += y * y;
      }
    }
  }
  sy = wm_block_sum(sy, red);
  if (threadIdx.x == 0) pb[blockIdx.x * 3 + 2] = sy;
}

__global__ __launch_bounds__(WA_T) void wave_mix_gauss_kernel(float* __restrict__ wav, const long* __restrict__ lens, int Ls,
                                                              const float* __restrict__ gauss_amp, unsigned k0, unsigned k1, unsigned o0,
                                                              unsigned o1, int nchunk, const float* __restrict__ partial) {
  const int b = blockIdx.y;
  const long n = wa_clip_len(lens, b, Ls);
  const long t0 = (long)blockIdx.x * WM_CHUNK;
  const float amp = gauss_amp[b];
  if (!(amp > 0.f) || t0 >= n) return;
  const int ncb = (int)((n + WM_CHUNK - 1) / WM_CHUNK);
  const float sigma = (float)(sqrt(wm_total(partial + (long)b * nchunk * 3, ncb, 2) / (double)n) * (double)amp);
  float* x = wav + (long)b * Ls;
#pragma unroll
  for (int g = 0; g < WM_G; ++g) {
    const long q = t0 / 4 + threadIdx.x + g * WA_T;
    if (4 * q >= n) continue;
    float z[4];
    wave_normal4(philox4x32_10((unsigned)q, (unsigned)b, o0, o1, k0, k1), z);
#pragma unroll
    for (int i = 0; i < 4; ++i) { const long t = 4 * q + i; if (t < n) x[t] = x[t] + sigma * z[i]; }
  }
}

extern "C" long ta_wave_mix_scratch_floats(int B, int Ls) {
  if (B <= 0 || Ls <= 0) return 0;
  return (long)B * ta_cdiv(Ls, WM_CHUNK) * 3;
}

extern "C" int ta_wave_mix_f32(float* wav, const long* lens, int B, int Ls, const int* noise_idx, const long* noise_start,
                               const float* noise_amp, const float* noise, const long* noise_off, int n_noise, const float* gauss_amp,
                               unsigned long long seed, unsigned long long offset, float* scratch, hipStream_t st) {
  if (B <= 0 || Ls <= 0) return TA_OK;
  const bool bg = noise_idx && n_noise > 0;
  if (!bg && !gauss_amp) return TA_OK;
  if (!wav || !lens || !scratch || B > 65535 || (bg && (!noise_start || !noise_amp || !noise || !noise_off))) return TA_ERR_ARG;
  const int nchunk = ta_cdiv(Ls, WM_CHUNK);
  const dim3 grid(nchunk, B);
  TA_LAUNCH(wave_mix_sums_kernel, grid, dim3(WA_T), 0, st, wav, lens, Ls, bg ? noise_idx : nullptr, noise_start, noise, noise_off, n_noise,
            gauss_amp, nchunk, scratch);
  TA_CHECK_LAUNCH();
  if (bg) {
    TA_LAUNCH(wave_mix_bg_kernel, grid, dim3(WA_T), 0, st, wav, lens, Ls, noise_idx, noise_start, noise_amp, noise, noise_off, n_noise,
              nchunk, scratch);
    TA_CHECK_LAUNCH();
  }
  if (gauss_amp) {
    TA_LAUNCH(wave_mix_gauss_kernel, grid, dim3(WA_T), 0, st, wav, lens, Ls, gauss_amp, (unsigned)seed, (unsigned)(seed >> 32),
              (unsigned)offset, (unsigned)(offset >> 32), nchunk, scratch);
    TA_CHECK_LAUNCH();
  }
  return TA_OK;
}

// ---- percentile clipping (audiomentations ClippingDistortion): lo, hi = numpy.percentile(x[0:n], [q, 100 - q]) with linear
// interpolation, q = pct / 2; y = clip(x, lo, hi).  One 1024-thread workgroup per clip with pct > 0.  The two percentiles need the
// order statistics floor(v) and floor(v) + 1 of v = (n - 1) q / 100 each.  They are found exactly, without a sort, by bisection on
// the order-preserving integer image of the floats (the technique of ta_logits_warp's top-k): the k-th smallest (0-based) is the
// smallest o with count(x <= o) >= k + 1; both bisections share their <= 32 counting passes over the clip (which stays in L2), and
// one more pass gives each statistic's successor (itself when count(x <= o) >= k + 2, else the smallest value above it).
__device__ __forceinline__ int wc_f2ord(float f) { const int i = __float_as_int(f); return i >= 0 ? i : i ^ 0x7fffffff; }
__device__ __forceinline__ float wc_ord2f(int o) { return __int_as_float(o >= 0 ? o : o ^ 0x7fffffff); }
__device__ __forceinline__ int wc_wave_isum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wc_wave_imin(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const int u = __shfl_xor(v, o, 64); v = u < v ? u : v; }
  return v;
}
// block-wide {sum, sum} (MIN = false) or {min, min} (MIN = true) of two ints; red: [2][16]
template <bool MIN>
__device__ __forceinline__ void wc_block2(int& a, int& b, int (*red)[16]) {
  a = MIN ? wc_wave_imin(a) : wc_wave_isum(a);
  b = MIN ? wc_wave_imin(b) : wc_wave_isum(b);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; }
  __syncthreads();
  a = red[0][0]; b = red[1][0];
#pragma unroll
  for (int w = 1; w < 16; ++w) {
    if (MIN) { a = red[0][w] < a ? red[0][w] : a; b = red[1][w] < b ? red[1][w] : b; }
    else { a += red[0][w]; b += red[1][w]; }
  }
}
__device__ __forceinline__ float wc_lerp(float a, float b, double g) {          // numpy's _lerp, in double, rounded once
  const double d = (double)b - (double)a;
  return (float)(g >= 0.5 ? (double)b - d * (1.0 - g) : (double)a + d * g);
}

__global__ __launch_bounds__(1024) void wave_clip_kernel(float* __restrict__ wav, const long* __restrict__ lens, int Ls,
                                                         const int* __restrict__ pct) {
  __shared__ int red[2][16];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int q = pct[b] / 2;
  const int n = (int)wa_clip_len(lens, b, Ls);
  if (pct[b] <= 0 || q <= 0 || n <= 1) return;       // q = 0: the thresholds are the minimum and the maximum; nothing changes
  float* x = wav + (long)b * Ls;
  const double vl = (double)(n - 1) * ((double)q / 100.0), vh = (double)(n - 1) * ((double)(100 - q) / 100.0);
  const int kl = (int)floor(vl), kh = (int)floor(vh);
  const double gl = vl - (double)kl, gh = vh - (double)kh;
  int mn = 0x7fffffff, mxn = 0x7fffffff;                // min of ord, min of -ord - 1 (= ~ord: order-reversing, no overflow)
  for (int t = tid; t < n; t += 1024) { const int o = wc_f2ord(x[t]); mn = o < mn ? o : mn; mxn = ~o < mxn ? ~o : mxn; }
  wc_block2<true>(mn, mxn, red);
  long lo0 = mn, hi0 = ~mxn, lo1 = lo0, hi1 = hi0;
  while (lo0 < hi0 || lo1 < hi1) {
    const long m0 = lo0 + (hi0 - lo0) / 2, m1 = lo1 + (hi1 - lo1) / 2;
    int c0 = 0, c1 = 0;
    for (int t = tid; t < n; t += 1024) { const long o = wc_f2ord(x[t]); c0 += o <= m0; c1 += o <= m1; }
    wc_block2<false>(c0, c1, red);
    if (lo0 < hi0) { if (c0 >= kl + 1) hi0 = m0; else lo0 = m0 + 1; }
    if (lo1 < hi1) { if (c1 >= kh + 1) hi1 = m1; else lo1 = m1 + 1; }
  }
  int c0 = 0, c1 = 0, nx0 = 0x7fffffff, nx1 = 0x7fffffff;
  for (int t = tid; t < n; t += 1024) {
    const int o = wc_f2ord(x[t]);
    c0 += o <= lo0; c1 += o <= lo1;
    if (o > lo0 && o < nx0) nx0 = o;
    if (o > lo1 && o < nx1) nx1 = o;
  }
  wc_block2<false>(c0, c1, red);
  wc_block2<true>(nx0, nx1, red);
  const int a0 = (int)lo0, a1 = (int)lo1;
  const int b0 = (kl + 1 > n - 1 || c0 >= kl + 2) ? a0 : nx0, b1 = (kh + 1 > n - 1 || c1 >= kh + 2) ? a1 : nx1;
  const float lo = wc_lerp(wc_ord2f(a0), wc_ord2f(b0), gl), hi = wc_lerp(wc_ord2f(a1), wc_ord2f(b1), gh);
  __syncthreads();
  for (int t = tid; t < n; t += 1024) { const float v = x[t]; x[t] = fminf(fmaxf(v, lo), hi); }
}

extern "C" int ta_wave_clip_f32(float* wav, const long* lens, int B, int Ls, const int* pct, hipStream_t st) {
  if (B <= 0 || Ls <= 0 || !pct) return TA_OK;
  if (!wav || !lens) return TA_ERR_ARG;
  TA_LAUNCH(wave_clip_kernel, dim3(B), dim3(1024), 0, st, wav, lens, Ls, pct);
  TA_CHECK_LAUNCH();
  return TA_OK;
}

// ---- short noises (audiomentations AddShortNoises): per clip a list of <= WE_MAX events, each a window [o, o + l) of a pool clip laid
// at t0 with a fade in / out that is linear in dB from -D to 0, at an SNR against the rms R of the stage's input over [0, n), taken
// once before any event.  Three launches, no atomics: the per-chunk sums of x^2, the per-(event, chunk) sums of the event's own
// samples (both f32 trees inside a chunk of 4096, the chunk partials summed in one fixed order in double by whoever needs them), then
// one pass over (chunk, clip) that adds, in list order, the events touching the chunk.  Descriptor arrays are [B, ev_stride].
// An event that names no pool clip, reaches outside it, starts before 0, is empty or is longer than max_event_len is skipped.
#define WE_MAX 64

struct WeEvent {
  const float* v;      // pool_j + o, or nullptr when the event is not valid
  long l, t0;
  int fin, fout;
};
__device__ __forceinline__ WeEvent we_event(int idx, const int* ev_pool, const long* ev_off, const long* ev_len, const long* ev_t0,
                                            const int* ev_fin, const int* ev_fout, const float* pool, const long* pool_off, int n_pool,
                                            long max_event_len) {
  WeEvent e;
  e.v = nullptr; e.l = ev_len[idx]; e.t0 = ev_t0[idx]; e.fin = ev_fin[idx]; e.fout = ev_fout[idx];
  const int j = ev_pool[idx];
  const long o = ev_off[idx];
  if (j < 0 || j >= n_pool || o < 0 || e.l < 1 || e.l > max_event_len || e.t0 < 0 || e.fin < 0 || e.fout < 0) return e;
  if (o + e.l > pool_off[j + 1] - pool_off[j]) return e;
  e.v = pool + pool_off[j] + o;
  return e;
}
__device__ __forceinline__ int we_count(const int* ev_count, int b, int ev_stride) {
  const int c = ev_count[b], m = ev_stride < WE_MAX ? ev_stride : WE_MAX;
  return c < 0 ? 0 : (c > m ? m : c);
}

// grid (nchunk, B): xpart[b][c] = sum x^2 of chunk c, for the clips that have events
__global__ __launch_bounds__(WA_T) void wave_events_xsum_kernel(const float* __restrict__ wav, const long* __restrict__ lens, int Ls,
                                                                const int* __restrict__ ev_count, int ev_stride, int nchunk,
                                                                float* __restrict__ xpart) {
  __shared__ float red[WA_T / 64];
  const int b = blockIdx.y;
  const long n = wa_clip_len(lens, b, Ls), t0 = (long)blockIdx.x * WM_CHUNK;
  if (we_count(ev_count, b, ev_stride) <= 0 || t0 >= n) return;
  const float* x = wav + (long)b * Ls;
  float sx = 0.f;
  for (int i = threadIdx.x; i < WM_CHUNK; i += WA_T) { const long t = t0 + i; if (t < n) { const float xv = x[t]; sx += xv * xv; } }
  sx = wm_block_sum(sx, red);
  if (threadIdx.x == 0) xpart[(long)b * nchunk + blockIdx.x] = sx;
}

// grid (nchunk_e, events, B): epart[b][e][c] = sum v^2 of chunk c of event e's own window
__global__ __launch_bounds__(WA_T) void wave_events_rms_kernel(const int* __restrict__ ev_count, int ev_stride, const int* __restrict__ ev_pool,
                                                               const long* __restrict__ ev_off, const long* __restrict__ ev_len,
                                                               const long* __restrict__ ev_t0, const int* __restrict__ ev_fin,
                                                               const int* __restrict__ ev_fout, const float* __restrict__ pool,
                                                               const long* __restrict__ pool_off, int n_pool, long max_event_len,
                                                               int nchunk_e, float* __restrict__ epart) {
  __shared__ float red[WA_T / 64];
  const int b = blockIdx.z, e = blockIdx.y;
  if (e >= we_count(ev_count, b, ev_stride)) return;
  const WeEvent ev = we_event(b * ev_stride + e, ev_pool, ev_off, ev_len, ev_t0, ev_fin, ev_fout, pool, pool_off, n_pool, max_event_len);
  const long i0 = (long)blockIdx.x * WM_CHUNK;
  if (!ev.v || i0 >= ev.l) return;
  float sv = 0.f;
  for (int i = threadIdx.x; i < WM_CHUNK; i += WA_T) { const long q = i0 + i; if (q < ev.l) { const float vv = ev.v[q]; sv += vv * vv; } }
  sv = wm_block_sum(sv, red);
  if (threadIdx.x == 0) epart[((long)b * ev_stride + e) * nchunk_e + blockIdx.x] = sv;
}

// grid (nchunk, B): y[t] = x[t] + sum over the events e in list order of g_e a_in a_out v_e[t - t0_e]
__global__ __launch_bounds__(WA_T) void wave_events_add_kernel(float* __restrict__ wav, const long* __restrict__ lens, int Ls,
                                                               const int* __restrict__ ev_count, int ev_stride, const int* __restrict__ ev_pool,
                                                               const long* __restrict__ ev_off, const long* __restrict__ ev_len,
                                                               const long* __restrict__ ev_t0, const int* __restrict__ ev_fin,
                                                               const int* __restrict__ ev_fout, const float* __restrict__ ev_amp,
                                                               const float* __restrict__ pool, const long* __restrict__ pool_off, int n_pool,
                                                               long max_event_len, float fade_k, int nchunk, int nchunk_e,
                                                               const float* __restrict__ xpart, const float* __restrict__ epart) {
  const int b = blockIdx.y;
  const long n = wa_clip_len(lens, b, Ls), c0 = (long)blockIdx.x * WM_CHUNK;
  const int cnt = we_count(ev_count, b, ev_stride);
  if (cnt <= 0 || c0 >= n) return;
  const long c1 = c0 + WM_CHUNK < n ? c0 + WM_CHUNK : n;
  const int ncb = (int)((n + WM_CHUNK - 1) / WM_CHUNK);
  double sx = 0.0;
  for (int c = 0; c < ncb; ++c) sx += (double)xpart[(long)b * nchunk + c];
  const double R = sqrt(sx / (double)n);
  float* x = wav + (long)b * Ls;
  float acc[WM_CHUNK / WA_T];
#pragma unroll
  for (int q = 0; q < WM_CHUNK / WA_T; ++q) { const long t = c0 + threadIdx.x + q * WA_T; acc[q] = t < n ? x[t] : 0.f; }
  for (int e = 0; e < cnt; ++e) {
    const WeEvent ev = we_event(b * ev_stride + e, ev_pool, ev_off, ev_len, ev_t0, ev_fin, ev_fout, pool, pool_off, n_pool, max_event_len);
    if (!ev.v || ev.t0 >= c1 || ev.t0 + ev.l <= c0) continue;
    const float* ep = epart + ((long)b * ev_stride + e) * nchunk_e;
    const int nce = (int)((ev.l + WM_CHUNK - 1) / WM_CHUNK);
    double se = 0.0;
    for (int c = 0; c < nce; ++c) se += (double)ep[c];
    const double re = sqrt(se / (double)ev.l);
    if (re < 1e-9) continue;                                   // a silent event: skipped
    const float g = (float)(R * (double)ev_amp[b * ev_stride + e] / re);
    const float rin = ev.fin > 0 ? 1.0f / (float)ev.fin : 0.f, rout = ev.fout > 0 ? 1.0f / (float)ev.fout : 0.f;
#pragma unroll
    for (int q = 0; q < WM_CHUNK / WA_T; ++q) {
      const long t = c0 + threadIdx.x + q * WA_T, i = t - ev.t0;
      if (i < 0 || i >= ev.l || t >= n) continue;
      float a = g;
      if (i < ev.fin) a *= exp2f(fade_k * (1.0f - (float)(i + 1) * rin));
      if (i >= ev.l - ev.fout) a *= exp2f(fade_k * (1.0f - (float)(ev.l - i) * rout));
      acc[q] += a * ev.v[i];
    }
  }
#pragma unroll
  for (int q = 0; q < WM_CHUNK / WA_T; ++q) { const long t = c0 + threadIdx.x + q * WA_T; if (t < n) x[t] = acc[q]; }
}

extern "C" long ta_wave_events_scratch_floats(int B, int Ls, int ev_stride, long max_event_len) {
  if (B <= 0 || Ls <= 0 || ev_stride <= 0 || max_event_len <= 0) return 0;
  return (long)B * ta_cdiv(Ls, WM_CHUNK) + (long)B * ev_stride * ta_cdiv(max_event_len, WM_CHUNK);
}

extern "C" int ta_wave_events_f32(float* wav, const long* lens, int B, int Ls, const int* ev_count, int ev_stride, const int* ev_pool,
                                  const long* ev_off, const long* ev_len, const long* ev_t0, const int* ev_fade_in, const int* ev_fade_out,
                                  const float* ev_amp, const float* pool, const long* pool_off, int n_pool, long max_event_len,
                                  float fade_floor_db, float* scratch, hipStream_t st) {
  if (B <= 0 || Ls <= 0 || !ev_count || ev_stride <= 0 || n_pool <= 0 || max_event_len <= 0) return TA_OK;
  if (!wav || !lens || !ev_pool || !ev_off || !ev_len || !ev_t0 || !ev_fade_in || !ev_fade_out || !ev_amp || !pool || !pool_off || !scratch ||
      B > 65535 || ev_stride > WE_MAX || !(fade_floor_db >= 0.f))
    return TA_ERR_ARG;
  const int nchunk = ta_cdiv(Ls, WM_CHUNK), nchunk_e = ta_cdiv(max_event_len, WM_CHUNK);
  if (nchunk_e > 65535) return TA_ERR_ARG;
  float *xpart = scratch, *epart = scratch + (long)B * nchunk;
  const float fade_k = (float)(-(double)fade_floor_db / 20.0 * 3.321928094887362);      // a = 2^(fade_k (1 - position)), log2(10)
  TA_LAUNCH(wave_events_xsum_kernel, dim3(nchunk, B), dim3(WA_T), 0, st, wav, lens, Ls, ev_count, ev_stride, nchunk, xpart);
  TA_CHECK_LAUNCH();
  TA_LAUNCH(wave_events_rms_kernel, dim3(nchunk_e, ev_stride, B), dim3(WA_T), 0, st, ev_count, ev_stride, ev_pool, ev_off, ev_len, ev_t0,
            ev_fade_in, ev_fade_out, pool, pool_off, n_pool, max_event_len, nchunk_e, epart);
  TA_CHECK_LAUNCH();
  TA_LAUNCH(wave_events_add_kernel, dim3(nchunk, B), dim3(WA_T), 0, st, wav, lens, Ls, ev_count, ev_stride, ev_pool, ev_off, ev_len, ev_t0,
            ev_fade_in, ev_fade_out, ev_amp, pool, pool_off, n_pool, max_event_len, fade_k, nchunk, nchunk_e, xpart, epart);
  TA_CHECK_LAUNCH();
  return TA_OK;
}

// ---- exact time-parallel cascade of second-order sections (the EQ and the band-limit): clip b is filtered by n_sec[b] <= WI_S
// sections (b0, b1, b2, a1, a2), a0 = 1, given in float64; the recurrence is carried in f64 (direct form II transposed, as
// scipy.signal.sosfilt), reads and writes f32 in place, and rounds each output sample once.
// A cascade of S sections is ONE linear system with 2 S states, so the state after a chunk of T samples is
//     s[c + 1] = M s[c] + z[c],   M = the chunk's zero-input map (2S x 2S),  z[c] = the final state of chunk c run from a zero state.
//   phase 1, grid (chunk groups + 1, B), one thread per chunk: z[c] of every chunk that has a successor; the extra workgroup builds M,
//            column j = T zero-input steps from the unit state e_j;
//   phase 2, grid (B), one wave per clip, lane r = row r of M: the entry state of every chunk, sequentially over chunks (z is
//            prefetched eight chunks ahead; the state is passed between lanes by v_readlane);
//   phase 3, as phase 1: every chunk reruns from its entry state and writes.
// This is the recurrence itself, refactored: no warm-up, no overlap.  No atomics; nothing depends on launch order.
// A thread walks its own chunk, so neighbouring lanes are a whole chunk apart in memory: the workgroup moves tiles of 64 chunks x 32
// samples between memory and LDS in 128-byte rows, and a thread reads its row of the tile (row stride 33 floats: no bank conflict).
// The state array of a chunk is 2 WI_S doubles; rows [2 k, 2 k + 1] are the two delays of section k.
#define WI_S 8
#define WI_NS (2 * WI_S)
#define WI_WG 64
#define WI_TILE 32
#define WI_LD (WI_TILE + 1)

template <int S>
__device__ __forceinline__ double wi_step(double x, const double (&cf)[WI_S][5], double (&s)[WI_NS]) {
#pragma unroll
  for (int k = 0; k < S; ++k) {
    const double y = fma(cf[k][0], x, s[2 * k]);
    s[2 * k] = fma(-cf[k][3], y, fma(cf[k][1], x, s[2 * k + 1]));
    s[2 * k + 1] = fma(-cf[k][4], y, cf[k][2] * x);
    x = y;
  }
  return x;
}
__device__ __forceinline__ void wi_load_tile(float* lds, const float* __restrict__ x, long n, long group0, long T, int k) {
  for (int idx = threadIdx.x; idx < WI_WG * WI_TILE; idx += WI_WG) {
    const int row = idx / WI_TILE, col = idx % WI_TILE;
    const long t = (group0 + row) * T + (long)k * WI_TILE + col;
    lds[row * WI_LD + col] = t < n ? x[t] : 0.f;
  }
}
template <int S>
__device__ __forceinline__ void wi_load_coef(const double* __restrict__ sos, int b, double (&cf)[WI_S][5]) {
#pragma unroll
  for (int k = 0; k < S; ++k)
#pragma unroll
    for (int q = 0; q < 5; ++q) cf[k][q] = sos[((long)b * WI_S + k) * 5 + q];
}

template <int S>
__device__ __forceinline__ void wi_phase1(float* lds, const float* __restrict__ x, long n, int b, long T, int nck, bool build_m,
                                          const double* __restrict__ sos, double* __restrict__ Z, double* __restrict__ M) {
  double cf[WI_S][5], s[WI_NS];
  wi_load_coef<S>(sos, b, cf);
#pragma unroll
  for (int r = 0; r < WI_NS; ++r) s[r] = 0.0;
  if (build_m) {
    const int j = threadIdx.x;
    if (n <= T || j >= 2 * S) return;
#pragma unroll
    for (int r = 0; r < 2 * S; ++r) s[r] = r == j ? 1.0 : 0.0;
    for (long i = 0; i < T; ++i) wi_step<S>(0.0, cf, s);
#pragma unroll
    for (int r = 0; r < 2 * S; ++r) M[(long)b * WI_NS * WI_NS + j * WI_NS + r] = s[r];
    return;
  }
  const long group0 = (long)blockIdx.x * WI_WG, ck = group0 + threadIdx.x;
  if (group0 * T >= n) return;
  const bool active = (ck + 1) * T < n;            // only a chunk with a successor needs its final state
  for (int k = 0; k < T / WI_TILE; ++k) {
    __syncthreads();
    wi_load_tile(lds, x, n, group0, T, k);
    __syncthreads();
    if (active)
      for (int i = 0; i < WI_TILE; ++i) wi_step<S>((double)lds[threadIdx.x * WI_LD + i], cf, s);
  }
  if (active)
#pragma unroll
    for (int r = 0; r < 2 * S; ++r) Z[((long)b * nck + ck) * WI_NS + r] = s[r];
}

template <int S>
__device__ __forceinline__ void wi_phase3(float* lds, float* __restrict__ x, long n, int b, long T, int nck,
                                          const double* __restrict__ sos, const double* __restrict__ Z) {
  double cf[WI_S][5], s[WI_NS];
  wi_load_coef<S>(sos, b, cf);
  const long group0 = (long)blockIdx.x * WI_WG, ck = group0 + threadIdx.x;
  if (group0 * T >= n) return;
  const bool active = ck * T < n;
#pragma unroll
  for (int r = 0; r < WI_NS; ++r) s[r] = 0.0;
  if (active && ck > 0)
#pragma unroll
    for (int r = 0; r < 2 * S; ++r) s[r] = Z[((long)b * nck + ck) * WI_NS + r];
  for (int k = 0; k < T / WI_TILE; ++k) {
    if (group0 * T + (long)k * WI_TILE >= n && (group0 + 1) * T >= n) break;      // one chunk in this group, and it has ended
    __syncthreads();
    wi_load_tile(lds, x, n, group0, T, k);
    __syncthreads();
    if (active)
      for (int i = 0; i < WI_TILE; ++i) {
        float* p = lds + threadIdx.x * WI_LD + i;
        *p = (float)wi_step<S>((double)*p, cf, s);
      }
    __syncthreads();
    for (int idx = threadIdx.x; idx < WI_WG * WI_TILE; idx += WI_WG) {
      const int row = idx / WI_TILE, col = idx % WI_TILE;
      const long t = (group0 + row) * T + (long)k * WI_TILE + col;
      if (t < n) x[t] = lds[row * WI_LD + col];
    }
  }
}

#define WI_DISPATCH(S, CALL)   \
  switch (S) {                 \
    case 1: CALL(1); break;    \
    case 2: CALL(2); break;    \
    case 3: CALL(3); break;    \
    case 4: CALL(4); break;    \
    case 5: CALL(5); break;    \
    case 6: CALL(6); break;    \
    case 7: CALL(7); break;    \
    case 8: CALL(8); break;    \
    default: break;            \
  }

__device__ __forceinline__ int wi_sections(const int* n_sec, int b) { const int S = n_sec[b]; return (S < 0 || S > WI_S) ? 0 : S; }

// grid (cdiv(nck, 64) + 1, B); the last workgroup of a clip builds M
__global__ __launch_bounds__(WI_WG) void wave_sos_local_kernel(const float* __restrict__ wav, const long* __restrict__ lens, int Ls,
                                                               const int* __restrict__ n_sec, const double* __restrict__ sos, long T, int nck,
                                                               double* __restrict__ Z, double* __restrict__ M) {
  __shared__ float lds[WI_WG * WI_LD];
  const int b = blockIdx.y, S = wi_sections(n_sec, b);
  const long n = wa_clip_len(lens, b, Ls);
  if (S <= 0 || n <= T) return;                    // a single chunk has no successor: nothing to prepare
  const bool build_m = blockIdx.x == gridDim.x - 1;
  const float* x = wav + (long)b * Ls;
#define WI_CALL(SS) wi_phase1<SS>(lds, x, n, b, T, nck, build_m, sos, Z, M)
  WI_DISPATCH(S, WI_CALL)
#undef WI_CALL
}

__device__ __forceinline__ double wi_readlane(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// grid (B), one wave: Z[b][c] (the final state of chunk c from zero) is replaced by the entry state of chunk c
#define WI_PF 8
__global__ __launch_bounds__(WI_WG) void wave_sos_carry_kernel(const long* __restrict__ lens, int Ls, const int* __restrict__ n_sec, long T,
                                                               int nck, double* __restrict__ Z, const double* __restrict__ M) {
  const int b = blockIdx.x, S = wi_sections(n_sec, b), r = threadIdx.x;
  const long n = wa_clip_len(lens, b, Ls);
  if (S <= 0 || n <= T) return;
  const int nchunks = (int)((n + T - 1) / T);
  const bool lane_on = r < 2 * S;
  double mrow[WI_NS];
#pragma unroll
  for (int j = 0; j < WI_NS; ++j) mrow[j] = (lane_on && j < 2 * S) ? M[(long)b * WI_NS * WI_NS + j * WI_NS + r] : 0.0;
  double* zb = Z + (long)b * nck * WI_NS + (lane_on ? r : 0);
  double s = 0.0, zcur[WI_PF], znext[WI_PF];
  // z[c] exists for c < nchunks - 1
#pragma unroll
  for (int q = 0; q < WI_PF; ++q) zcur[q] = (lane_on && q < nchunks - 1) ? zb[(long)q * WI_NS] : 0.0;
  for (int c0 = 0; c0 < nchunks; c0 += WI_PF) {
#pragma unroll
    for (int q = 0; q < WI_PF; ++q) { const int c = c0 + WI_PF + q; znext[q] = (lane_on && c < nchunks - 1) ? zb[(long)c * WI_NS] : 0.0; }
#pragma unroll
    for (int q = 0; q < WI_PF; ++q) {
      const int c = c0 + q;
      if (c < nchunks) {                                      // (uniform)
        if (lane_on) zb[(long)c * WI_NS] = s;
        double acc = zcur[q];
#pragma unroll
        for (int j = 0; j < WI_NS; ++j) acc = fma(mrow[j], wi_readlane(s, j), acc);
        s = acc;
      }
    }
#pragma unroll
    for (int q = 0; q < WI_PF; ++q) zcur[q] = znext[q];
  }
}

// grid (cdiv(nck, 64), B)
__global__ __launch_bounds__(WI_WG) void wave_sos_apply_kernel(float* __restrict__ wav, const long* __restrict__ lens, int Ls,
                                                               const int* __restrict__ n_sec, const double* __restrict__ sos, long T, int nck,
                                                               const double* __restrict__ Z) {
  __shared__ float lds[WI_WG * WI_LD];
  const int b = blockIdx.y, S = wi_sections(n_sec, b);
  const long n = wa_clip_len(lens, b, Ls);
  if (S <= 0 || n <= 0) return;
  float* x = wav + (long)b * Ls;
#define WI_CALL(SS) wi_phase3<SS>(lds, x, n, b, T, nck, sos, Z)
  WI_DISPATCH(S, WI_CALL)
#undef WI_CALL
}

namespace {
inline long wi_chunk(int chunk) { return chunk > 0 ? chunk : 256; }
}

extern "C" long ta_wave_sos_ws_bytes(int B, int Ls, int chunk) {
  if (B <= 0 || Ls <= 0 || chunk < 0 || wi_chunk(chunk) % WI_TILE) return 0;
  return (long)B * ((long)ta_cdiv(Ls, wi_chunk(chunk)) * WI_NS + WI_NS * WI_NS) * (long)sizeof(double);
}

extern "C" int ta_wave_sos_f32(float* wav, const long* lens, int B, int Ls, const int* n_sec, const double* sos, int chunk, void* ws,
                               long ws_bytes, hipStream_t st) {
  if (B <= 0 || Ls <= 0 || !n_sec) return TA_OK;
  if (!wav || !lens || !sos || !ws || B > 65535 || chunk < 0 || wi_chunk(chunk) % WI_TILE || ws_bytes < ta_wave_sos_ws_bytes(B, Ls, chunk))
    return TA_ERR_ARG;
  const long T = wi_chunk(chunk);
  const int nck = ta_cdiv(Ls, T), ngroup = ta_cdiv(nck, WI_WG);
  if (ngroup + 1 > 65535) return TA_ERR_ARG;
  double* Z = (double*)ws;
  double* M = Z + (long)B * nck * WI_NS;
  if (nck > 1) {
    TA_LAUNCH(wave_sos_local_kernel, dim3(ngroup + 1, B), dim3(WI_WG), 0, st, wav, lens, Ls, n_sec, sos, T, nck, Z, M);
    TA_CHECK_LAUNCH();
    TA_LAUNCH(wave_sos_carry_kernel, dim3(B), dim3(WI_WG), 0, st, lens, Ls, n_sec, T, nck, Z, M);
    TA_CHECK_LAUNCH();
  }
  TA_LAUNCH(wave_sos_apply_kernel, dim3(ngroup, B), dim3(WI_WG), 0, st, wav, lens, Ls, n_sec, sos, T, nck, Z);
  TA_CHECK_LAUNCH();
  return TA_OK;
}
