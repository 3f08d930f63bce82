// ta355 -- frozen ECAPA-TDNN speaker-embedding model (the hot path of speaker diarization): windows of 16 kHz audio -> one embedding
// per window.  Replaces the one-window-per-call SpeechBrain encode_batch loop of the reference (tiny_audio/diarization.py:457-517);
// arithmetic of the published ECAPA-TDNN at SpeechBrain's spkrec-ecapa-voxceleb hyper-parameters, defined by tests/ecapa_ref.py.
//
// New kernels here: the filter bank (400-point FFT, mel, dB floor, sentence mean; one workgroup per window), the Res2Net chain on MFMA
// (one workgroup per window, the seven dilated convolutions in sequence through LDS), and the per-(window, channel) passes: ReLU +
// BatchNorm materialisation with the window statistics, the SE gate and residual, the attention activation and the attentive
// statistics pooling.  Every 1x1 convolution (and block0, over the overlapping rows of the haloed feature slab) is ta_gemm_bf16_nt.
// "ReLU, then the folded BatchNorm (scale, shift)" sits in the CONSUMER's load of a GEMM's pre-activation output wherever the consumer
// is one of these kernels; it is materialised once where the consumer is a GEMM.
#include "common.h"
#include "host_util.h"
#include "fft400.h"

namespace {
constexpr int EC_NFFT = 400, EC_HOP = 160, EC_NBIN = 201, EC_MELS = TA_ECAPA_N_MELS, EC_FS = TA_ECAPA_FEAT_STRIDE;
constexpr int EC_G = 2;                          // frame pairs per wave at once (two real frames ride in one complex transform)
constexpr int EC_MB = 5;                         // MFMA row blocks (16 frames each) a wave accumulates at once: T = 76 is one group

inline int ec_frames(int Lw) { return Lw / EC_HOP + 1; }

// ---------------------------------------------------------------------------- filter bank
// One workgroup = one window.  Window n is samples start .. start + len of the shared audio buffer, extended on the right to Lw
// samples by reflection (sample len + i = sample len - 2 - i) while it is read; the STFT is centred with ZERO padding, so frame t
// covers window samples 160 t - 200 .. 160 t + 199 and what lies outside [0, Lw) is 0.  A wave transforms EC_G frame pairs at a time
// (stage A: 16-point FFTs on 25 lanes per pair, stage B: 25-point FFTs on 16 lanes per pair, as logmel.hip), turns them into powers
// and applies the mel filters over their own bins; the raw dB values go to `feat`, which the same workgroup reads back for the window
// maximum (floor at max - 80 dB) and the per-mel mean over the T frames -- reductions inside the workgroup, no atomics.
__global__ __launch_bounds__(256) void ecapa_fbank_kernel(const float* __restrict__ audio, long n_audio, const int* __restrict__ starts,
                                                          const int* __restrict__ lens, int Lw, int T, const float* __restrict__ window,
                                                          const float* __restrict__ twiddle, const float* __restrict__ melfb,
                                                          const int* __restrict__ mrange_g, float* feat, bf16_t* __restrict__ slab) {
  __shared__ float win[EC_NFFT], tw[2 * EC_NFFT];
  __shared__ __attribute__((aligned(16))) float scr[4][EC_G * EC_NFFT * 2];
  __shared__ float pwv[4][2 * EC_G][EC_NBIN];
  __shared__ int mrange[2 * EC_MELS];
  __shared__ float wred[4], mean_s[EC_MELS];
  const int n = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long start = starts[n];
  int len = lens[n];
  len = len > Lw ? Lw : len;
  for (int j = tid; j < 2 * EC_NFFT; j += 256) tw[j] = twiddle[j];
  for (int j = tid; j < EC_NFFT; j += 256) win[j] = window[j];
  for (int j = tid; j < 2 * EC_MELS; j += 256) mrange[j] = mrange_g[j];
  __syncthreads();
  auto sample = [&](int idx) -> float {
    if (idx < 0 || idx >= Lw) return 0.f;
    if (idx >= len) idx = 2 * len - 2 - idx;
    const long g = start + idx;
    return (idx >= 0 && g >= 0 && g < n_audio) ? audio[g] : 0.f;       // (the host refuses windows that would get here out of range)
  };
  float* my = scr[wave];
  float* fo = feat + (long)n * T * EC_MELS;
  const int npairs = (T + 1) / 2, niter = (npairs + 4 * EC_G - 1) / (4 * EC_G);     // workgroup-uniform
  float lmax = -INFINITY;
  for (int it = 0; it < niter; ++it) {
    const int pair0 = (it * 4 + wave) * EC_G;
    // ---- stage A: lane = (pair g, n2)
    if (lane < EC_G * 25) {
      const int g = lane / 25, n2 = lane - g * 25;
      const int fa = 2 * (pair0 + g);
      const bool va = fa < T, vb = fa + 1 < T;
      cpx a[16];
#pragma unroll
      for (int n1 = 0; n1 < 16; ++n1) {
        const int j = 25 * n1 + n2;
        const float wv = win[j];
        a[n1].re = va ? sample(fa * EC_HOP - EC_NFFT / 2 + j) * wv : 0.f;
        a[n1].im = vb ? sample((fa + 1) * EC_HOP - EC_NFFT / 2 + j) * wv : 0.f;
      }
      fft16(a);
      float* dst = my + ((g * 16) * 25 + n2) * 2;
#pragma unroll
      for (int k1 = 0; k1 < 16; ++k1) {
        cpx v = a[k1];
        if (k1 > 0) {
          const int j = n2 * k1;                                  // < 400
          v = cmul(v, tw[2 * j], tw[2 * j + 1]);
        }
        *(float2*)(dst + k1 * 50) = make_float2(v.re, v.im);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // ---- stage B: lane = (pair g, k1)
    if (lane < EC_G * 16) {
      const int g = lane >> 4, k1 = lane & 15;
      const float* src = my + ((g * 16 + k1) * 25) * 2;
      cpx y[25];
#pragma unroll
      for (int n2 = 0; n2 < 25; ++n2) { const float2 v = *(const float2*)(src + 2 * n2); y[n2] = {v.x, v.y}; }
      fft25(y);                                                   // (every active lane holds its inputs: in-order LDS per wave)
      float* dst = my + (g * EC_NFFT + k1) * 2;
#pragma unroll
      for (int k2 = 0; k2 < 25; ++k2) *(float2*)(dst + 32 * k2) = make_float2(y[k2].re, y[k2].im);     // k = k1 + 16 k2
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // ---- combine: powers of the two real frames of every pair
    for (int id = lane; id < EC_G * EC_NBIN; id += 64) {
      const int g = id / EC_NBIN, k = id - g * EC_NBIN;
      const float2 z = *(const float2*)(my + (g * EC_NFFT + k) * 2);
      const float2 c = *(const float2*)(my + (g * EC_NFFT + (k == 0 ? 0 : EC_NFFT - k)) * 2);
      const float ar = 0.5f * (z.x + c.x), ai = 0.5f * (z.y - c.y);
      const float br = 0.5f * (z.y + c.y), bi = 0.5f * (c.x - z.x);
      pwv[wave][2 * g][k] = ar * ar + ai * ai;
      pwv[wave][2 * g + 1][k] = br * br + bi * bi;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // ---- mel + dB: item = (frame of this iteration, filter), every filter over its own bins only
    for (int item = lane; item < 2 * EC_G * EC_MELS; item += 64) {
      const int f = item / EC_MELS, m = item - f * EC_MELS, t = 2 * pair0 + f;
      float acc = 0.f;
      for (int k = mrange[2 * m]; k < mrange[2 * m + 1]; ++k) acc = fmaf(melfb[k * EC_MELS + m], pwv[wave][f][k], acc);
      const float v = 10.0f * log10f(fmaxf(acc, 1e-10f));
      if (t < T) { fo[(long)t * EC_MELS + m] = v; lmax = fmaxf(lmax, v); }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();                              // the next iteration overwrites the scratch and the powers
  }
  lmax = wave_max(lmax);
  if (lane == 0) wred[wave] = lmax;
  __syncthreads();                                                // (also: the raw dB values of every wave are visible)
  const float floorv = fmaxf(fmaxf(wred[0], wred[1]), fmaxf(wred[2], wred[3])) - 80.0f;
  if (tid < EC_MELS) {
    double s = 0.0;
    for (int t = 0; t < T; ++t) s += (double)fmaxf(fo[(long)t * EC_MELS + tid], floorv);
    mean_s[tid] = (float)(s / (double)T);
  }
  __syncthreads();
  // normalised features (in place) and the bf16 slab: rows 2 .. T + 1 the frames, two reflected halo rows per side (row 2 - j = frame
  // j, row T + 1 + j = frame T - 1 - j), channels 80 .. 127 zero
  bf16_t* so = slab + (long)n * (T + 4) * EC_FS;
  for (int i = tid; i < T * EC_FS; i += 256) {
    const int t = i / EC_FS, m = i - t * EC_FS;
    float v = 0.f;
    if (m < EC_MELS) {
      v = fmaxf(fo[(long)t * EC_MELS + m], floorv) - mean_s[m];
      fo[(long)t * EC_MELS + m] = v;
    }
    const bf16_t b = f2bf(v);
    so[(t + 2) * EC_FS + m] = b;
    if (t == 1 || t == 2) so[(2 - t) * EC_FS + m] = b;
    if (t == T - 2 || t == T - 3) so[(2 * T - t) * EC_FS + m] = b;
  }
}

// ---------------------------------------------------------------------------- Res2Net chain (MFMA)
// One workgroup = one window.  z1 is tdnn1's PRE-activation output; x_i = BN1(relu(z1[:, i w : (i + 1) w])).
//   y_0 = x_0,  y_1 = TDNN_0(x_1),  y_i = TDNN_{i-1}(x_i + y_{i-1}),  TDNN = BN(relu(conv_{k=3, dilation d, reflect}(.) + bias))
// Sub-band i's operand u = bf16(x_i + y_{i-1}) (f32 arithmetic, one rounding) is staged into LDS rows d .. d + T - 1 with its d
// reflected halo rows on each side written in the same pass; y_{i-1} is read back from the global rows this workgroup wrote one
// barrier earlier (bf16: the same bits a copy kept in LDS would hold, and the LDS footprint stays one buffer).  Output frame t,
// channel co = sum over k = tap w + ci of U[t + tap d][ci] wp[i - 1][co][k]: lane (lr, lk) of an A fragment holds 8 consecutive k,
// which never straddle a tap (w % 8 == 0); k >= 3 w (K rounded up to 32) meets zero weights and a zero A.  LDS rows are w + 8
// elements apart: 16 consecutive rows of a 16-byte fragment read land on distinct banks.
// A wave takes (column block, group of EC_MB row blocks) units round-robin; both barriers of a sub-band are outside that loop and
// every loop that holds one is bounded by kernel arguments.
__global__ __launch_bounds__(256) void ecapa_res2net_kernel(const bf16_t* __restrict__ z1, long ldz, long z_rpw, const float* __restrict__ s1,
                                                            const float* __restrict__ t1, const bf16_t* __restrict__ wp,
                                                            const float* __restrict__ rb, const float* __restrict__ rs,
                                                            const float* __restrict__ rt, bf16_t* y, long ldy, long y_rpw, int T, int w,
                                                            int d, int nsub) {
  extern __shared__ __attribute__((aligned(16))) bf16_t U[];
  const int n = blockIdx.x, tid = threadIdx.x;
  const int S = w + 8, vpr = w >> 3, nrb = (T + 15) >> 4, nbw = w >> 4, Kp = (3 * w + 31) / 32 * 32;
  const bf16_t* zr = z1 + (long)n * z_rpw * ldz;
  bf16_t* yr = y + (long)n * y_rpw * ldy;
  const int wave = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
  for (int i = 0; i < nsub; ++i) {
    // ---- stage (i >= 1) or copy (i == 0)
    for (int idx = tid; idx < T * vpr; idx += 256) {
      const int t = idx / vpr, cv = idx - t * vpr, c0 = i * w + cv * 8;
      const bf16x8 zv = *(const bf16x8*)(zr + (long)t * ldz + c0);
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = fmaf(fmaxf(bf2f((bf16_t)zv[j]), 0.f), s1[c0 + j], t1[c0 + j]);
      if (i >= 2) {
        const bf16x8 yv = *(const bf16x8*)(yr + (long)t * ldy + c0 - w);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += bf2f((bf16_t)yv[j]);
      }
      bf16x8 u;
#pragma unroll
      for (int j = 0; j < 8; j += 2) {
        const uint32_t p = pack2bf(v[j], v[j + 1]);
        u[j] = (short)(p & 0xffff); u[j + 1] = (short)(p >> 16);
      }
      if (i == 0) { *(bf16x8*)(yr + (long)t * ldy + c0) = u; continue; }
      *(bf16x8*)(U + (t + d) * S + cv * 8) = u;
      if (t >= 1 && t <= d) *(bf16x8*)(U + (d - t) * S + cv * 8) = u;                              // frame -t = frame t
      if (t <= T - 2 && t >= T - 1 - d) *(bf16x8*)(U + (d + 2 * (T - 1) - t) * S + cv * 8) = u;    // frame T - 1 + j = frame T - 1 - j
    }
    if (i == 0) continue;                                          // (uniform)
    __syncthreads();
    const int nmg = (nrb + EC_MB - 1) / EC_MB;
    for (int unit = wave; unit < nbw * nmg; unit += 4) {
      const int nb = unit % nbw, rb0 = (unit / nbw) * EC_MB;
      f32x4 acc[EC_MB];
#pragma unroll
      for (int mi = 0; mi < EC_MB; ++mi) acc[mi] = f32x4{0.f, 0.f, 0.f, 0.f};
      const bf16_t* b_base = wp + ((long)(i - 1) * w + nb * 16 + lr) * Kp + lk * 8;
      for (int k0 = 0; k0 < Kp; k0 += 32) {
        const int k = k0 + lk * 8;
        const bool kin = k < 3 * w;
        const int tap = kin ? k / w : 0, ci = kin ? k - tap * w : 0;
        const bf16x8 bf = *(const bf16x8*)(b_base + k0);
        const bf16_t* a_base = U + (rb0 * 16 + lr + tap * d) * S + ci;
#pragma unroll
        for (int mi = 0; mi < EC_MB; ++mi) {
          if (rb0 + mi < nrb) {                                    // (wave-uniform)
            bf16x8 a = {0, 0, 0, 0, 0, 0, 0, 0};
            if (kin) a = *(const bf16x8*)(a_base + mi * 16 * S);
            acc[mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bf, acc[mi], 0, 0, 0);
          }
        }
      }
      // C/D map: column (channel) = lane & 15, row (frame) = 4 (lane >> 4) + register
      const int co = nb * 16 + lr, ch = (i - 1) * w + co;
      const float bv = rb[ch], sc = rs[ch], sh = rt[ch];
#pragma unroll
      for (int mi = 0; mi < EC_MB; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int t = (rb0 + mi) * 16 + lk * 4 + r;
          if (rb0 + mi < nrb && t < T) yr[(long)t * ldy + i * w + co] = f2bf(fmaf(fmaxf(acc[mi][r] + bv, 0.f), sc, sh));
        }
    }
    __syncthreads();                                               // U is free again and y_i is visible to the whole workgroup
  }
}

// ---------------------------------------------------------------------------- per-(window, channel pair) passes
// thread = (window blockIdx.y, channels c, c + 1), serial over the window's T frames; a wave reads 256 contiguous bytes of a row.
__device__ __forceinline__ void relu_bn2(uint32_t z, float s0, float t0, float s1, float t1, float& v0, float& v1) {
  v0 = fmaf(fmaxf(bf2f((bf16_t)(z & 0xffff)), 0.f), s0, t0);
  v1 = fmaf(fmaxf(bf2f((bf16_t)(z >> 16)), 0.f), s1, t1);
}

// out = bf16(BN(relu(z))); with STATS also the window's mean and standard deviation over time of the ROUNDED values (what the
// consumers read), two passes: stats [N, 2 Cw] = (mean | sqrt(max(var, 1e-12))), f32 and / or bf16.
template <bool STATS>
__global__ __launch_bounds__(256) void ecapa_relu_bn_kernel(const bf16_t* __restrict__ z, const float* __restrict__ s, const float* __restrict__ sh,
                                                            bf16_t* out, float* __restrict__ stats_f32, bf16_t* __restrict__ stats_bf16,
                                                            int T, int Cw) {
  const int n = blockIdx.y, c = 2 * (blockIdx.x * 256 + threadIdx.x);
  if (c >= Cw) return;
  const float s0 = s[c], s1 = s[c + 1], t0 = sh[c], t1 = sh[c + 1];
  const long base = (long)n * T * Cw + c;
  float sum0 = 0.f, sum1 = 0.f;
#pragma unroll 4
  for (int t = 0; t < T; ++t) {
    float v0, v1;
    relu_bn2(*(const uint32_t*)(z + base + (long)t * Cw), s0, t0, s1, t1, v0, v1);
    const uint32_t p = pack2bf(v0, v1);
    *(uint32_t*)(out + base + (long)t * Cw) = p;
    if (STATS) { sum0 += bf2f((bf16_t)(p & 0xffff)); sum1 += bf2f((bf16_t)(p >> 16)); }
  }
  if (STATS) {
    const float m0 = sum0 / (float)T, m1 = sum1 / (float)T;
    float q0 = 0.f, q1 = 0.f;
#pragma unroll 4
    for (int t = 0; t < T; ++t) {
      const uint32_t p = *(const uint32_t*)(out + base + (long)t * Cw);                  // this thread's own stores
      const float d0 = bf2f((bf16_t)(p & 0xffff)) - m0, d1 = bf2f((bf16_t)(p >> 16)) - m1;
      q0 = fmaf(d0, d0, q0); q1 = fmaf(d1, d1, q1);
    }
    const float sd0 = sqrtf(fmaxf(q0 / (float)T, 1e-12f)), sd1 = sqrtf(fmaxf(q1 / (float)T, 1e-12f));
    const long o = (long)n * 2 * Cw + c;
    if (stats_f32) { stats_f32[o] = m0; stats_f32[o + 1] = m1; stats_f32[o + Cw] = sd0; stats_f32[o + Cw + 1] = sd1; }
    if (stats_bf16) { *(uint32_t*)(stats_bf16 + o) = pack2bf(m0, m1); *(uint32_t*)(stats_bf16 + o + Cw) = pack2bf(sd0, sd1); }
  }
}

// SE pass 1: mean over time of BN(relu(z2)) -> f32 [N, C]
__global__ __launch_bounds__(256) void ecapa_se_mean_kernel(const bf16_t* __restrict__ z, const float* __restrict__ s, const float* __restrict__ sh,
                                                            float* __restrict__ mean, int T, int Cw) {
  const int n = blockIdx.y, c = 2 * (blockIdx.x * 256 + threadIdx.x);
  if (c >= Cw) return;
  const float s0 = s[c], s1 = s[c + 1], t0 = sh[c], t1 = sh[c + 1];
  const long base = (long)n * T * Cw + c;
  float sum0 = 0.f, sum1 = 0.f;
#pragma unroll 4
  for (int t = 0; t < T; ++t) {
    float v0, v1;
    relu_bn2(*(const uint32_t*)(z + base + (long)t * Cw), s0, t0, s1, t1, v0, v1);
    sum0 += v0; sum1 += v1;
  }
  mean[(long)n * Cw + c] = sum0 / (float)T;
  mean[(long)n * Cw + c + 1] = sum1 / (float)T;
}

// The two SE matrices for one window per workgroup, a thread per output with the weights stored input-major (w1t [C, se],
// w2t [se, C]): consecutive threads read consecutive floats.  gate = sigmoid(W2 relu(W1 mean + b1) + b2), f32 [N, C].
__global__ __launch_bounds__(256) void ecapa_se_gate_kernel(const float* __restrict__ mean, const float* __restrict__ w1t, const float* __restrict__ b1,
                                                            const float* __restrict__ w2t, const float* __restrict__ b2, float* __restrict__ gate,
                                                            int Cw, int se) {
  extern __shared__ float se_lds[];
  float* m = se_lds;                 // [Cw]
  float* h = se_lds + Cw;            // [se]
  const int n = blockIdx.x;
  for (int c = threadIdx.x; c < Cw; c += 256) m[c] = mean[(long)n * Cw + c];
  __syncthreads();
  for (int j = threadIdx.x; j < se; j += 256) {
    float a = b1[j];
    for (int c = 0; c < Cw; ++c) a = fmaf(m[c], w1t[(long)c * se + j], a);
    h[j] = fmaxf(a, 0.f);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < Cw; c += 256) {
    float a = b2[c];
    for (int j = 0; j < se; ++j) a = fmaf(h[j], w2t[(long)j * Cw + c], a);
    gate[(long)n * Cw + c] = 1.0f / (1.0f + expf(-a));
  }
}

// SE pass 2: out = bf16(BN(relu(z2)) * gate + residual), written into the block's column slice of the concat buffer
__global__ __launch_bounds__(256) void ecapa_se_apply_kernel(const bf16_t* __restrict__ z, const float* __restrict__ s, const float* __restrict__ sh,
                                                             const float* __restrict__ gate, const bf16_t* __restrict__ res, long ldres,
                                                             bf16_t* __restrict__ out, long ldout, int T, int Cw) {
  const int n = blockIdx.y, c = 2 * (blockIdx.x * 256 + threadIdx.x);
  if (c >= Cw) return;
  const float s0 = s[c], s1 = s[c + 1], t0 = sh[c], t1 = sh[c + 1];
  const float g0 = gate[(long)n * Cw + c], g1 = gate[(long)n * Cw + c + 1];
  const long row0 = (long)n * T;
#pragma unroll 4
  for (int t = 0; t < T; ++t) {
    float v0, v1;
    relu_bn2(*(const uint32_t*)(z + (row0 + t) * Cw + c), s0, t0, s1, t1, v0, v1);
    const uint32_t r = *(const uint32_t*)(res + (row0 + t) * ldres + c);
    *(uint32_t*)(out + (row0 + t) * ldout + c) = pack2bf(fmaf(v0, g0, bf2f((bf16_t)(r & 0xffff))), fmaf(v1, g1, bf2f((bf16_t)(r >> 16))));
  }
}

// attention activation: out = bf16(tanh(BN(relu(g + per-window term)))) on the A-wide rows; g f32 [N T, A], pw f32 [N, A]
__global__ __launch_bounds__(256) void ecapa_attn_act_kernel(const float* __restrict__ g, const float* __restrict__ pw, const float* __restrict__ s,
                                                             const float* __restrict__ sh, bf16_t* __restrict__ out, long rows, int T, int A) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * A) return;
  const long row = i / A;
  const int c = (int)(i - row * A);
  const float v = g[i] + pw[(row / T) * A + c];
  out[i] = f2bf(tanhf(fmaf(fmaxf(v, 0.f), s[c], sh[c])));
}

// attentive statistics pooling: per (window, channel) softmax over the T frames of the f32 logits (two-pass maximum), the weighted
// mean and standard deviation of h (sqrt(max(var, 1e-12))), then asp_bn: out bf16 [N, 2 Cw] = BN([mean | std]).  attn_w (or NULL):
// the softmax weights f32 [N T, Cw]; pooled_f32 (or NULL): [N, 2 Cw] before asp_bn.
__global__ __launch_bounds__(256) void ecapa_asp_pool_kernel(const float* __restrict__ lg, const bf16_t* __restrict__ h, const float* __restrict__ s,
                                                             const float* __restrict__ sh, bf16_t* __restrict__ out, float* __restrict__ attn_w,
                                                             float* __restrict__ pooled_f32, int T, int Cw) {
  const int n = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= Cw) return;
  const long base = (long)n * T * Cw + c;
  float mx = -INFINITY;
#pragma unroll 4
  for (int t = 0; t < T; ++t) mx = fmaxf(mx, lg[base + (long)t * Cw]);
  // the mean is taken of h - h[0]: a channel that is constant over time then has mean == h[0] and a variance of exactly 0
  const float h0 = bf2f(h[base]);
  float se = 0.f, sx = 0.f;
#pragma unroll 4
  for (int t = 0; t < T; ++t) {
    const float e = expf(lg[base + (long)t * Cw] - mx);
    se += e;
    sx = fmaf(e, bf2f(h[base + (long)t * Cw]) - h0, sx);
  }
  const float inv = 1.0f / se, mean = h0 + sx * inv;
  float q = 0.f;
#pragma unroll 4
  for (int t = 0; t < T; ++t) {
    const float a = expf(lg[base + (long)t * Cw] - mx) * inv, dd = bf2f(h[base + (long)t * Cw]) - mean;
    q = fmaf(a, dd * dd, q);
    if (attn_w) attn_w[base + (long)t * Cw] = a;
  }
  const float sd = sqrtf(fmaxf(q, 1e-12f));
  const long o = (long)n * 2 * Cw + c;
  if (pooled_f32) { pooled_f32[o] = mean; pooled_f32[o + Cw] = sd; }
  out[o] = f2bf(fmaf(mean, s[c], sh[c]));
  out[o + Cw] = f2bf(fmaf(sd, s[Cw + c], sh[Cw + c]));
}

bool ec_geom_ok(int T, int Cw) { return T >= TA_ECAPA_MIN_T && T <= TA_ECAPA_MAX_T && Cw > 0 && Cw % 2 == 0; }

struct EcWs {
  float *feat, *lg, *ga, *se_mean, *se_gate, *pwa;
  bf16_t *slab, *za, *x0, *yb, *cat, *h, *ta, *ms, *pooled;
  size_t bytes;
};
EcWs ec_carve(const ta_ecapa_weights* w, int nw, int T, void* base) {
  const size_t C = w->channels, A = w->attn_channels, R = (size_t)nw * T;
  Carver c(base);
  EcWs e;
  e.feat = c.take<float>(R * EC_MELS);
  e.slab = c.take<bf16_t>((size_t)nw * (T + 4) * EC_FS);
  e.za = c.take<bf16_t>(R * C);                // the pre-activation output of block0, tdnn1, tdnn2 in turn
  e.x0 = c.take<bf16_t>(R * C);
  e.yb = c.take<bf16_t>(R * C);
  e.cat = c.take<bf16_t>(R * 3 * C);
  e.h = c.take<bf16_t>(R * 3 * C);
  e.lg = c.take<float>(R * 3 * C);             // first mfa's bf16 pre-activation output (dead behind relu_bn), then the f32 attention logits
  e.ga = c.take<float>(R * A);
  e.ta = c.take<bf16_t>(R * A);
  e.se_mean = c.take<float>((size_t)nw * C);
  e.se_gate = c.take<float>((size_t)nw * C);
  e.ms = c.take<bf16_t>((size_t)nw * 6 * C);
  e.pwa = c.take<float>((size_t)nw * A);
  e.pooled = c.take<bf16_t>((size_t)nw * 6 * C);
  e.bytes = c.total();
  return e;
}
bool ec_weights_ok(const ta_ecapa_weights* w) {
  if (!w) return false;
  const int C = w->channels;
  if (C < 128 || C > TA_ECAPA_MAX_CHANNELS || C % 128) return false;                  // w = C / 8: a multiple of 16 up to 128
  if (w->se_channels < 1 || w->se_channels > TA_ECAPA_MAX_SE) return false;
  if (w->attn_channels < 64 || w->attn_channels > TA_ECAPA_MAX_ATTN || w->attn_channels % 64) return false;
  if (w->emb_dim < 4 || w->emb_dim > TA_ECAPA_MAX_EMB || w->emb_dim % 4) return false;
  if (!w->fb_window || !w->fb_twiddle || !w->fb_mel || !w->fb_mel_range || !w->w0 || !w->b0 || !w->bn0_s || !w->bn0_t || !w->mfa_w ||
      !w->mfa_b || !w->mfa_s || !w->mfa_t || !w->att_wh || !w->att_wms || !w->att_b || !w->att_s || !w->att_t || !w->att_conv_w ||
      !w->att_conv_b || !w->aspbn_s || !w->aspbn_t || !w->fc_w || !w->fc_b)
    return false;
  for (int b = 0; b < 3; ++b) {
    const ta_ecapa_block& k = w->blocks[b];
    if (k.dilation < 1 || k.dilation > TA_ECAPA_MAX_DILATION) return false;
    if (!k.w1 || !k.b1 || !k.bn1_s || !k.bn1_t || !k.res_w || !k.res_b || !k.res_s || !k.res_t || !k.w2 || !k.b2 || !k.bn2_s ||
        !k.bn2_t || !k.se_w1t || !k.se_b1 || !k.se_w2t || !k.se_b2)
      return false;
  }
  return true;
}
}  // namespace

extern "C" int ta_ecapa_fbank(const float* audio, long n_audio, const int* starts_dev, const int* lens_dev, int N, int window_samples,
                              const float* fb_window, const float* fb_twiddle, const float* fb_mel, const int* fb_mel_range,
                              float* feat, void* slab_bf16, hipStream_t st) {
  if (N <= 0) return TA_OK;
  if (!audio || n_audio <= 0 || !starts_dev || !lens_dev || !fb_window || !fb_twiddle || !fb_mel || !fb_mel_range || !feat || !slab_bf16)
    return TA_ERR_ARG;
  const int T = ec_frames(window_samples);
  if (window_samples <= 0 || T < TA_ECAPA_MIN_T || T > TA_ECAPA_MAX_T) return TA_ERR_ARG;
  TA_LAUNCH(ecapa_fbank_kernel, dim3(N), dim3(256), 0, st, audio, n_audio, starts_dev, lens_dev, window_samples, T, fb_window, fb_twiddle,
            fb_mel, fb_mel_range, feat, (bf16_t*)slab_bf16);
  TA_CHECK_LAUNCH();
  return TA_OK;
}

extern "C" int ta_ecapa_res2net(const void* z1, long ldz, long z_rpw, const float* bn1_s, const float* bn1_t, const void* res_w,
                                const float* res_b, const float* res_s, const float* res_t, void* y, long ldy, long y_rpw, int N, int T,
                                int w, int dilation, hipStream_t st) {
  if (N <= 0) return TA_OK;
  if (!z1 || !bn1_s || !bn1_t || !res_w || !res_b || !res_s || !res_t || !y || z1 == y) return TA_ERR_ARG;
  if (w < 16 || w > 128 || w % 16 || dilation < 1 || dilation > TA_ECAPA_MAX_DILATION || T <= dilation || T < TA_ECAPA_MIN_T ||
      T > TA_ECAPA_MAX_T)
    return TA_ERR_ARG;
  const long Cw = (long)TA_ECAPA_SCALE * w;
  if (ldz < Cw || ldy < Cw || ldz % 8 || ldy % 8 || z_rpw < T || y_rpw < T || (((size_t)z1 | (size_t)y) & 15)) return TA_ERR_ARG;
  const size_t lds = (size_t)(((T + 15) / 16) * 16 + 2 * dilation) * (w + 8) * sizeof(bf16_t);
  static bool attr = false;
  if (!attr) {
    const size_t most = (size_t)(((TA_ECAPA_MAX_T + 15) / 16) * 16 + 2 * TA_ECAPA_MAX_DILATION) * (128 + 8) * sizeof(bf16_t);
    if (hipFuncSetAttribute((const void*)ecapa_res2net_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)most) != hipSuccess)
      return TA_ERR_LAUNCH;
    attr = true;
  }
  TA_LAUNCH(ecapa_res2net_kernel, dim3(N), dim3(256), lds, st, (const bf16_t*)z1, ldz, z_rpw, bn1_s, bn1_t, (const bf16_t*)res_w, res_b,
            res_s, res_t, (bf16_t*)y, ldy, y_rpw, T, w, dilation, TA_ECAPA_SCALE);
  TA_CHECK_LAUNCH();
  return TA_OK;
}

extern "C" int ta_ecapa_relu_bn(const void* z, const float* scale, const float* shift, void* out, float* stats_f32, void* stats_bf16,
                                int N, int T, int Cw, hipStream_t st) {
  if (N <= 0) return TA_OK;
  if (!z || !scale || !shift || !out || !ec_geom_ok(T, Cw) || N > 65535) return TA_ERR_ARG;
  const dim3 grid(ta_cdiv(Cw / 2, 256), N);
  if (stats_f32 || stats_bf16)
    TA_LAUNCH((ecapa_relu_bn_kernel<true>), grid, dim3(256), 0, st, (const bf16_t*)z, scale, shift, (bf16_t*)out, stats_f32, (bf16_t*)stats_bf16, T, Cw);
  else
    TA_LAUNCH((ecapa_relu_bn_kernel<false>), grid, dim3(256), 0, st, (const bf16_t*)z, scale, shift, (bf16_t*)out, (float*)nullptr, (bf16_t*)nullptr, T, Cw);
  TA_CHECK_LAUNCH();
  return TA_OK;
}

extern "C" long ta_ecapa_se_ws_floats(int N, int Cw) { return N > 0 && Cw > 0 ? 2L * N * Cw : 0; }

extern "C" int ta_ecapa_se_residual(const void* z2, const float* bn2_s, const float* bn2_t, const float* se_w1t, const float* se_b1,
                                    const float* se_w2t, const float* se_b2, const void* residual, long ldres, void* out, long ldout,
                                    int N, int T, int Cw, int se, float* ws, hipStream_t st) {
  if (N <= 0) return TA_OK;
  if (!z2 || !bn2_s || !bn2_t || !se_w1t || !se_b1 || !se_w2t || !se_b2 || !residual || !out || !ws || !ec_geom_ok(T, Cw) || N > 65535)
    return TA_ERR_ARG;
  if (Cw > TA_ECAPA_MAX_CHANNELS || se < 1 || se > TA_ECAPA_MAX_SE || ldres < Cw || ldout < Cw || ldres % 2 || ldout % 2) return TA_ERR_ARG;
  float* mean = ws;
  float* gate = ws + (long)N * Cw;
  const dim3 grid(ta_cdiv(Cw / 2, 256), N);
  TA_LAUNCH(ecapa_se_mean_kernel, grid, dim3(256), 0, st, (const bf16_t*)z2, bn2_s, bn2_t, mean, T, Cw);
  TA_CHECK_LAUNCH();
  TA_LAUNCH(ecapa_se_gate_kernel, dim3(N), dim3(256), (size_t)(Cw + se) * sizeof(float), st, (const float*)mean, se_w1t, se_b1, se_w2t, se_b2,
            gate, Cw, se);
  TA_CHECK_LAUNCH();
  TA_LAUNCH(ecapa_se_apply_kernel, grid, dim3(256), 0, st, (const bf16_t*)z2, bn2_s, bn2_t, (const float*)gate, (const bf16_t*)residual, ldres,
            (bf16_t*)out, ldout, T, Cw);
  TA_CHECK_LAUNCH();
  return TA_OK;
}

extern "C" int ta_ecapa_attn_act(const float* g, const float* per_window, const float* scale, const float* shift, void* out, int N, int T,
                                 int A, hipStream_t st) {
  if (N <= 0) return TA_OK;
  if (!g || !per_window || !scale || !shift || !out || !ec_geom_ok(T, A)) return TA_ERR_ARG;
  const long rows = (long)N * T;
  if (rows * A > 0x7fffffffL * 256) return TA_ERR_ARG;
  TA_LAUNCH(ecapa_attn_act_kernel, dim3(ta_cdiv(rows * A, 256)), dim3(256), 0, st, g, per_window, scale, shift, (bf16_t*)out, rows, T, A);
  TA_CHECK_LAUNCH();
  return TA_OK;
}

extern "C" int ta_ecapa_asp_pool(const float* logits, const void* h, const float* aspbn_s, const float* aspbn_t, void* out, float* attn_w,
                                 float* pooled_f32, int N, int T, int Cw, hipStream_t st) {
  if (N <= 0) return TA_OK;
  if (!logits || !h || !aspbn_s || !aspbn_t || !out || !ec_geom_ok(T, Cw) || N > 65535) return TA_ERR_ARG;
  TA_LAUNCH(ecapa_asp_pool_kernel, dim3(ta_cdiv(Cw, 256), N), dim3(256), 0, st, logits, (const bf16_t*)h, aspbn_s, aspbn_t, (bf16_t*)out, attn_w,
            pooled_f32, T, Cw);
  TA_CHECK_LAUNCH();
  return TA_OK;
}

extern "C" long ta_ecapa_workspace_bytes(const ta_ecapa_weights* w, int n_windows, int T) {
  if (!ec_weights_ok(w) || n_windows <= 0 || T < TA_ECAPA_MIN_T || T > TA_ECAPA_MAX_T) return 0;
  return (long)ec_carve(w, n_windows, T, nullptr).bytes;
}

extern "C" int ta_ecapa_forward(const ta_ecapa_weights* w, const float* audio, long n_audio, const int* starts_host, const int* lens_host,
                                const int* starts_dev, const int* lens_dev, int N, int window_samples, int chunk_windows, float* emb,
                                void* ws, long ws_bytes, hipStream_t st) {
  if (N <= 0) return TA_OK;
  if (!ec_weights_ok(w) || !audio || n_audio <= 0 || !starts_host || !lens_host || !starts_dev || !lens_dev || !emb || !ws ||
      chunk_windows <= 0 || window_samples <= 0)
    return TA_ERR_ARG;
  const int T = ec_frames(window_samples);
  if (T < TA_ECAPA_MIN_T || T > TA_ECAPA_MAX_T) return TA_ERR_ARG;
  for (int i = 0; i < N; ++i) {
    // np.pad(mode="reflect") needs pad <= len - 1; the window must lie inside the audio buffer
    const long s = starts_host[i], l = lens_host[i];
    if (s < 0 || l < 1 || l > window_samples || s + l > n_audio || window_samples - l > l - 1) return TA_ERR_ARG;
  }
  const int chunk = chunk_windows < N ? chunk_windows : N;
  const int C = w->channels, A = w->attn_channels, D = w->emb_dim, wd = C / TA_ECAPA_SCALE;
  if ((long)chunk * T * 3 * C > 0x7fffffffL || chunk > 65535) return TA_ERR_ARG;
  EcWs e = ec_carve(w, chunk, T, ws);
  if ((long)e.bytes > ws_bytes) return TA_ERR_ARG;
  for (int c0 = 0; c0 < N; c0 += chunk) {
    const int nw = N - c0 < chunk ? N - c0 : chunk, R = nw * T;
    RC(ta_ecapa_fbank(audio, n_audio, starts_dev + c0, lens_dev + c0, nw, window_samples, w->fb_window, w->fb_twiddle, w->fb_mel,
                      w->fb_mel_range, e.feat, e.slab, st));
    // block0: frame t's operand row is the contiguous 5 x stride run from slab row t (the two halo rows per side are in the slab)
    RC(ta_gemm_bf16_nt(e.slab, w->w0, e.za, R, C, 5 * EC_FS, EC_FS, T, (long)(T + 4) * EC_FS, C, 0, 0, 0, w->b0, nullptr, 0, 1, 1, nullptr, st));
    RC(ta_ecapa_relu_bn(e.za, w->bn0_s, w->bn0_t, e.x0, nullptr, nullptr, nw, T, C, st));
    const bf16_t* xin = e.x0;
    long ldx = C;
    for (int b = 0; b < 3; ++b) {
      const ta_ecapa_block& k = w->blocks[b];
      RC(ta_gemm_bf16_nt(xin, k.w1, e.za, R, C, C, ldx, 0, 0, C, 0, 0, 0, k.b1, nullptr, 0, 1, 1, nullptr, st));
      RC(ta_ecapa_res2net(e.za, C, T, k.bn1_s, k.bn1_t, k.res_w, k.res_b, k.res_s, k.res_t, e.yb, C, T, nw, T, wd, k.dilation, st));
      RC(gemm(e.yb, k.w2, e.za, R, C, C, k.b2, nullptr, 0, 1, st));
      // the block's output lands in its column slice of the concat buffer and nowhere else
      RC(ta_ecapa_se_residual(e.za, k.bn2_s, k.bn2_t, k.se_w1t, k.se_b1, k.se_w2t, k.se_b2, xin, ldx, e.cat + (long)b * C, 3L * C, nw, T, C,
                              w->se_channels, e.se_mean, st));
      xin = e.cat + (long)b * C;
      ldx = 3L * C;
    }
    bf16_t* zm = (bf16_t*)e.lg;
    RC(gemm(e.cat, w->mfa_w, zm, R, 3 * C, 3 * C, w->mfa_b, nullptr, 0, 1, st));
    RC(ta_ecapa_relu_bn(zm, w->mfa_s, w->mfa_t, e.h, nullptr, e.ms, nw, T, 3 * C, st));
    // attention: [m; s] is constant over a window's frames, so its share of the 9C -> A convolution is one [nw, 6C] x [6C, A] product
    RC(gemm(e.h, w->att_wh, e.ga, R, A, 3 * C, nullptr, nullptr, 0, 0, st));
    RC(gemm(e.ms, w->att_wms, e.pwa, nw, A, 6 * C, w->att_b, nullptr, 0, 0, st));
    RC(ta_ecapa_attn_act(e.ga, e.pwa, w->att_s, w->att_t, e.ta, nw, T, A, st));
    RC(gemm(e.ta, w->att_conv_w, e.lg, R, 3 * C, A, w->att_conv_b, nullptr, 0, 0, st));
    RC(ta_ecapa_asp_pool(e.lg, e.h, w->aspbn_s, w->aspbn_t, e.pooled, nullptr, nullptr, nw, T, 3 * C, st));
    RC(gemm(e.pooled, w->fc_w, emb + (long)c0 * D, nw, D, 6 * C, w->fc_b, nullptr, 0, 0, st));
  }
  return TA_OK;
}
