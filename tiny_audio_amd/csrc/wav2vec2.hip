// ta355 -- frozen wav2vec2-base CTC acoustic model (the front half of forced alignment): waveform -> log-softmax emissions for a
// ragged batch, every clip as if alone.  Replaces the torchaudio bundle the reference runs through PyTorch
// (tiny_audio/alignment.py:206-211); arithmetic of Wav2Vec2ForCTC, TF:models/wav2vec2/modeling_wav2vec2.py, with
// feat_extract_norm="group", conv_bias=False, do_stable_layer_norm=False, no attention mask.
//
// New kernels here: conv layer 0 + GroupNorm + GELU (three launches: chunk statistics, their merge, apply), the grouped positional
// convolution on MFMA, and the head's bias + log-softmax.  Conv layers 1-6, the projections, the attention and the LayerNorms are
// the library's existing kernels (ta_gemm_bf16_nt over overlapping time-major rows, ta_attention_enc_fwd_varlen, ta_layernorm_*).
//
// Second half of the file: the layer-norm / stable family (feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True:
// wav2vec2-large-lv60, XLSR-53, XLS-R 300M, MMS 300M) -- input normalisation, conv 0 + bias + channel LayerNorm + GELU in one
// kernel, and the composite ta_wav2vec2_sln_forward; the LayerNorm + GELU behind conv 1-6 is norm.hip's ta_layernorm_gelu_bf16.
#include "common.h"
#include "host_util.h"

namespace {
constexpr int W2V_K0 = 10, W2V_S0 = 5;            // conv layer 0: kernel, stride
constexpr int W2V_CHUNK = 256;                    // frames of conv 0 per workgroup (statistics and apply)
constexpr int W2V_POS_K = 128, W2V_POS_PAD = 64, W2V_POS_GROUPS = 16;
constexpr int W2V_POS_TILE = 256;                 // frames per workgroup of the positional conv: 4 waves x 64 rows
constexpr int W2V_HEAD_PAD = 64;                  // lm_head rows after zero padding (one wave = one emission row)
const int W2V_KS[7] = {10, 3, 3, 3, 3, 2, 2};
const int W2V_ST[7] = {5, 2, 2, 2, 2, 2, 2};

inline int w2v_t0(int L) { return L >= W2V_K0 ? (L - W2V_K0) / W2V_S0 + 1 : 0; }
inline int w2v_frames(int L, int upto = 7) {     // frames behind conv layer upto - 1
  int T = L;
  for (int l = 0; l < upto; ++l) T = T >= W2V_KS[l] ? (T - W2V_KS[l]) / W2V_ST[l] + 1 : 0;
  return T;
}

// ---------------------------------------------------------------------------- conv 0 + GroupNorm(C groups) + GELU
// One workgroup = W2V_CHUNK frames of one clip, every channel (a thread walks channels tid, tid + 256, ...).  The clip's samples of
// the chunk sit in LDS; all lanes read the same sample at a time (a broadcast), each with its own 10 taps in registers.
__device__ __forceinline__ float conv0_at(const float* s, const float (&w)[W2V_K0], int t) {
  float v = 0.f;
#pragma unroll
  for (int j = 0; j < W2V_K0; ++j) v = fmaf(w[j], s[t * W2V_S0 + j], v);
  return v;
}

// MODE 0: per-chunk statistics -> part [B, nchunk, C, 2] = (mean of the chunk, sum of squared deviations from THAT mean): two passes
//         over the chunk's 10-MAC conv, so no E[x^2] - E[x]^2 anywhere.
// MODE 1: recompute the conv, normalise with the clip's merged statistics, GELU, bf16 time-major rows [t, C] of the clip's slab.
template <int MODE>
__global__ __launch_bounds__(256) void w2v_conv0_kernel(const float* __restrict__ wav, int Ls, const int* __restrict__ lens,
                                                        const float* __restrict__ w, int C, int nchunk, float* __restrict__ part,
                                                        const float* __restrict__ stats, const float* __restrict__ gn_w,
                                                        const float* __restrict__ gn_b, bf16_t* __restrict__ out, long out_rpb) {
  __shared__ float s[W2V_CHUNK * W2V_S0 + W2V_K0];
  const int b = blockIdx.y, chunk = blockIdx.x;
  int L = lens[b];
  L = L > Ls ? Ls : L;
  const int T0 = L >= W2V_K0 ? (L - W2V_K0) / W2V_S0 + 1 : 0;
  const int t0 = chunk * W2V_CHUNK;
  if (t0 >= T0) return;
  const int n = min(W2V_CHUNK, T0 - t0);
  const int ns = (n - 1) * W2V_S0 + W2V_K0;       // last sample read: (t0 + n - 1) * 5 + 9 <= L - 1
  const float* src = wav + (long)b * Ls + (long)t0 * W2V_S0;
  for (int i = threadIdx.x; i < ns; i += 256) s[i] = src[i];
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    float wr[W2V_K0];
#pragma unroll
    for (int j = 0; j < W2V_K0; ++j) wr[j] = w[c * W2V_K0 + j];
    if (MODE == 0) {
      float sum = 0.f;
      for (int t = 0; t < n; ++t) sum += conv0_at(s, wr, t);
      const float mean = sum / (float)n;
      float m2 = 0.f;
      for (int t = 0; t < n; ++t) { const float d = conv0_at(s, wr, t) - mean; m2 = fmaf(d, d, m2); }
      float* p = part + (((long)b * nchunk + chunk) * C + c) * 2;
      p[0] = mean; p[1] = m2;
    } else {
      const float mean = stats[((long)b * C + c) * 2], scale = stats[((long)b * C + c) * 2 + 1] * gn_w[c], beta = gn_b[c];
      bf16_t* o = out + ((long)b * out_rpb + t0) * C + c;
      for (int t = 0; t < n; ++t) o[(long)t * C] = f2bf(gelu_erf(fmaf(conv0_at(s, wr, t) - mean, scale, beta)));
    }
  }
}

// The chunks of one (clip, channel) merged in chunk order by the pairwise update of Chan et al. (n, mean, M2), in double:
// stats [B, C, 2] = (mean, 1 / sqrt(M2 / T0 + eps)) -- the biased variance GroupNorm uses.
__global__ __launch_bounds__(256) void w2v_conv0_merge_kernel(const float* __restrict__ part, const int* __restrict__ lens, int Ls, int C,
                                                              int nchunk, float eps, float* __restrict__ stats) {
  const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  int L = lens[b];
  L = L > Ls ? Ls : L;
  const int T0 = L >= W2V_K0 ? (L - W2V_K0) / W2V_S0 + 1 : 0;
  double n = 0., mean = 0., m2 = 0.;
  for (int k = 0; k * W2V_CHUNK < T0; ++k) {
    const float* p = part + (((long)b * nchunk + k) * C + c) * 2;
    const double nb = (double)min(W2V_CHUNK, T0 - k * W2V_CHUNK), d = (double)p[0] - mean, nn = n + nb;
    mean += d * nb / nn;
    m2 += (double)p[1] + d * d * n * nb / nn;
    n = nn;
  }
  stats[((long)b * C + c) * 2] = (float)mean;
  stats[((long)b * C + c) * 2 + 1] = n > 0. ? (float)(1.0 / sqrt(m2 / n + (double)eps)) : 0.f;
}

// ---------------------------------------------------------------------------- grouped positional convolution (MFMA)
// out[t, g cg + co] = x[t, g cg + co] + gelu(b[g cg + co] + sum_{tap < 128, ci < cg} x[t + tap - 64, g cg + ci] w[co, ci, tap]),
// t in [0, T) of the clip alone: zeros outside its rows, frame T (the 129th-tap output of the even kernel) never produced.
// One workgroup = (256-frame tile, group, clip).  The group's [256 + 127, cg] window of x is staged ONCE in LDS as bf16, rows
// cg elements apart with no padding: output frame t's whole K = 128 cg operand row (k = tap cg + ci) is then the CONTIGUOUS run
// starting at slab row t, so walking the taps is walking k along the slab and no tap re-reads x.  A wave owns 64 frames (4 MFMA
// row blocks) x every output channel of the group (NB column blocks of 16); B fragments come straight from the packed weight
// image wp [16][NB 16][128 cg] (rows co >= cg zero), 16 bytes per lane.
template <int NB, bool XF32>
__global__ __launch_bounds__(256) void w2v_pos_conv_kernel(const void* __restrict__ xv, void* __restrict__ yv, const bf16_t* __restrict__ wp,
                                                           const float* __restrict__ bias, const int* __restrict__ cu, int H, int cg) {
  extern __shared__ __attribute__((aligned(16))) bf16_t slab[];
  const int g = blockIdx.y, b = blockIdx.z;
  const int r0 = cu[b], T = cu[b + 1] - r0, t0 = blockIdx.x * W2V_POS_TILE;
  if (t0 >= T) return;
  const int vpr = cg >> 3;                                   // 8-channel vectors per slab row
  const int nvec = (W2V_POS_TILE + W2V_POS_K - 1) * vpr;
  for (int i = threadIdx.x; i < nvec; i += 256) {
    const int j = i / vpr, cv = i - j * vpr, t = t0 - W2V_POS_PAD + j;
    bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (t >= 0 && t < T) {
      const long off = (long)(r0 + t) * H + g * cg + cv * 8;
      if (XF32) {
        const float4 lo = *(const float4*)((const float*)xv + off), hi = *(const float4*)((const float*)xv + off + 4);
        const uint32_t p0 = pack2bf(lo.x, lo.y), p1 = pack2bf(lo.z, lo.w), p2 = pack2bf(hi.x, hi.y), p3 = pack2bf(hi.z, hi.w);
        v[0] = (short)(p0 & 0xffff); v[1] = (short)(p0 >> 16); v[2] = (short)(p1 & 0xffff); v[3] = (short)(p1 >> 16);
        v[4] = (short)(p2 & 0xffff); v[5] = (short)(p2 >> 16); v[6] = (short)(p3 & 0xffff); v[7] = (short)(p3 >> 16);
      } else {
        v = *(const bf16x8*)((const bf16_t*)xv + off);
      }
    }
    *(bf16x8*)(slab + (long)i * 8) = v;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
  const int m0 = wave * 64;
  if (t0 + m0 >= T) return;                                  // (behind the only barrier)
  const int K = W2V_POS_K * cg;
  f32x4 acc[4][NB];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[mi][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bf16_t* a_base = slab + (m0 + lr) * cg + lk * 8;
  const bf16_t* b_base = wp + ((long)g * NB * 16 + lr) * K + lk * 8;
#pragma unroll 2
  for (int k0 = 0; k0 < K; k0 += 32) {
    bf16x8 bf[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) bf[nb] = *(const bf16x8*)(b_base + (long)nb * 16 * K + k0);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      const bf16x8 a = *(const bf16x8*)(a_base + mi * 16 * cg + k0);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[mi][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bf[nb], acc[mi][nb], 0, 0, 0);
    }
  }
  // C/D map: column (channel) = lane & 15, row (frame) = 4 (lane >> 4) + register
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int co = nb * 16 + lr;
    if (co >= cg) continue;
    const int col = g * cg + co;
    const float bv = bias[col];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int t = t0 + m0 + mi * 16 + lk * 4 + r;
        if (t >= T) continue;
        const long off = (long)(r0 + t) * H + col;
        const float pe = gelu_erf(acc[mi][nb][r] + bv);
        if (XF32) ((float*)yv)[off] = ((const float*)xv)[off] + pe;
        else ((bf16_t*)yv)[off] = f2bf(bf2f(((const bf16_t*)xv)[off]) + pe);
      }
  }
}

// ---------------------------------------------------------------------------- head: bias + log-softmax over n_classes <= 64
// One wave per emission row, lane = class.  logits [rows, ld] are the lm_head GEMM's f32 output at its padded width: the lanes
// at and beyond n_classes hold -inf and enter neither the maximum nor the sum.
__global__ __launch_bounds__(256) void w2v_head_kernel(const float* __restrict__ logits, long ld, const float* __restrict__ bias, int nc,
                                                       float* __restrict__ out, int rows) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const bool live = lane < nc;
  const float v = live ? logits[(long)row * ld + lane] + bias[lane] : -INFINITY;
  const float m = wave_max(v);
  const float e = live ? expf(v - m) : 0.f;
  const float lse = logf(wave_sum(e));
  if (live) out[(long)row * nc + lane] = v - m - lse;
}

// ============================================================================ the "layer-norm / stable" family (wav2vec2-large-lv60, XLSR-53,
// XLS-R 300M, MMS 300M): feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True, optional input normalisation.
//
// ---------------------------------------------------------------------------- input normalisation: (x - mean) / sqrt(var + eps) per clip
constexpr int W2V_NORM_CHUNK = 4096;              // samples per workgroup of the statistics pass: 256 threads x 16

__device__ __forceinline__ float w2v_block_sum(float v, float* red) {          // 256 threads, the same bits on every run
  v = wave_sum(v);
  __syncthreads();                                                               // (red may still be read from the call before)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// part [B, nchunk, 2] = (mean of the chunk, sum of squared deviations from THAT mean); the chunk's samples stay in registers
__global__ __launch_bounds__(256) void w2v_norm_stats_kernel(const float* __restrict__ wav, int Ls, const int* __restrict__ lens, int nchunk,
                                                             float* __restrict__ part) {
  __shared__ float red[4];
  const int b = blockIdx.y, k = blockIdx.x;
  int L = lens[b];
  L = L > Ls ? Ls : L;
  const long s0 = (long)k * W2V_NORM_CHUNK;
  if (s0 >= L) return;
  const int n = (int)min((long)W2V_NORM_CHUNK, (long)L - s0);
  const float* src = wav + (long)b * Ls + s0;
  float x[W2V_NORM_CHUNK / 256];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < W2V_NORM_CHUNK / 256; ++i) {
    const int idx = threadIdx.x + i * 256;
    x[i] = idx < n ? src[idx] : 0.f;
    sum += x[i];
  }
  const float mean = w2v_block_sum(sum, red) / (float)n;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < W2V_NORM_CHUNK / 256; ++i) {
    const float d = x[i] - mean;
    if (threadIdx.x + i * 256 < n) q = fmaf(d, d, q);
  }
  q = w2v_block_sum(q, red);
  if (threadIdx.x == 0) {
    float* p = part + ((long)b * nchunk + k) * 2;
    p[0] = mean; p[1] = q;
  }
}

// (n, mean, M2) of two disjoint sets -> of their union (Chan et al.), in double
__device__ __forceinline__ void w2v_chan(double& n, double& mean, double& m2, double nb, double mb, double qb) {
  if (nb <= 0.) return;
  const double d = mb - mean, nn = n + nb;
  mean += d * nb / nn;
  m2 += qb + d * d * n * nb / nn;
  n = nn;
}

// One wave per clip: lane l merges chunks l, l + 64, ... in order, then the 64 lanes merge as a tree.  stats [B, 2] = (mean, rstd).
__global__ __launch_bounds__(64) void w2v_norm_merge_kernel(const float* __restrict__ part, const int* __restrict__ lens, int Ls, int nchunk,
                                                            float eps, float* __restrict__ stats) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int L = lens[b];
  L = L > Ls ? Ls : L;
  double n = 0., mean = 0., m2 = 0.;
  for (long k = lane; k * W2V_NORM_CHUNK < L; k += 64) {
    const float* p = part + ((long)b * nchunk + k) * 2;
    w2v_chan(n, mean, m2, (double)min((long)W2V_NORM_CHUNK, (long)L - k * W2V_NORM_CHUNK), (double)p[0], (double)p[1]);
  }
  for (int o = 1; o < 64; o <<= 1) {
    const double nb = __shfl_xor(n, o, 64), mb = __shfl_xor(mean, o, 64), qb = __shfl_xor(m2, o, 64);
    // both partners must produce the same bits: merge (lower lane's set, upper lane's set) in that order on both
    if (lane & o) { double n2 = nb, me2 = mb, q2 = qb; w2v_chan(n2, me2, q2, n, mean, m2); n = n2; mean = me2; m2 = q2; }
    else w2v_chan(n, mean, m2, nb, mb, qb);
  }
  if (lane == 0) {
    stats[b * 2] = (float)mean;
    stats[b * 2 + 1] = n > 0. ? (float)(1.0 / sqrt(m2 / n + (double)eps)) : 0.f;
  }
}

// out[b, i] = (wav[b, i] - mean_b) * rstd_b for i < len_b; the samples behind a clip's end are not written (out may be wav)
__global__ __launch_bounds__(256) void w2v_norm_apply_kernel(const float* wav, int Ls, const int* __restrict__ lens,
                                                             const float* __restrict__ stats, float* out) {
  const int b = blockIdx.y;
  int L = lens[b];
  L = L > Ls ? Ls : L;
  const float mean = stats[b * 2], rstd = stats[b * 2 + 1];
  const long base = (long)b * Ls;
  for (int i = blockIdx.x * 1024 + threadIdx.x; i < min(L, (int)(blockIdx.x + 1) * 1024); i += 256) out[base + i] = (wav[base + i] - mean) * rstd;
}

// ---------------------------------------------------------------------------- conv 0 + bias + LayerNorm over the channels + GELU
// The statistics are local to a frame, so this is ONE pass: one wave = one frame at a time, lane l owning the CPL = C / 64 CONTIGUOUS
// channels l CPL .. l CPL + CPL - 1 with their 10 taps, bias, gain and shift in registers.  The frame's 10 samples come from LDS
// at one address for the whole wave (a broadcast); the two reductions (mean, then squared deviations from it) are 64-lane
// shuffles, 12 steps per frame against 10 CPL FMAs + CPL erff per lane; and a wave's store is the frame's whole row, 2 C
// contiguous bytes (16 per lane at C = 512).  The f32 conv is never stored.  One workgroup = W2V_CHUNK frames of one clip, its
// four waves taking frames w, w + 4, ...
template <int CPL>
__global__ __launch_bounds__(256) void w2v_conv0_ln_kernel(const float* __restrict__ wav, int Ls, const int* __restrict__ lens,
                                                           const float* __restrict__ w, const float* __restrict__ bias,
                                                           const float* __restrict__ ln_w, const float* __restrict__ ln_b, float eps,
                                                           bf16_t* __restrict__ out, long out_rpb) {
  constexpr int C = CPL * 64;
  __shared__ float s[W2V_CHUNK * W2V_S0 + W2V_K0];
  const int b = blockIdx.y, chunk = blockIdx.x;
  int L = lens[b];
  L = L > Ls ? Ls : L;
  const int T0 = L >= W2V_K0 ? (L - W2V_K0) / W2V_S0 + 1 : 0;
  const int t0 = chunk * W2V_CHUNK;
  if (t0 >= T0) return;
  const int n = min(W2V_CHUNK, T0 - t0);
  const int ns = (n - 1) * W2V_S0 + W2V_K0;       // last sample read: (t0 + n - 1) * 5 + 9 <= L - 1
  const float* src = wav + (long)b * Ls + (long)t0 * W2V_S0;
  for (int i = threadIdx.x; i < ns; i += 256) s[i] = src[i];
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c0 = lane * CPL;
  float wr[CPL][W2V_K0], bs[CPL], g[CPL], be[CPL];
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
#pragma unroll
    for (int j = 0; j < W2V_K0; ++j) wr[i][j] = w[(c0 + i) * W2V_K0 + j];
    bs[i] = bias[c0 + i]; g[i] = ln_w[c0 + i]; be[i] = ln_b[c0 + i];
  }
  bf16_t* orow = out + ((long)b * out_rpb + t0) * C + c0;
#pragma unroll 2
  for (int t = wave; t < n; t += 4) {
    float x[W2V_K0], v[CPL];
#pragma unroll
    for (int j = 0; j < W2V_K0; ++j) x[j] = s[t * W2V_S0 + j];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      float a = bs[i];
#pragma unroll
      for (int j = 0; j < W2V_K0; ++j) a = fmaf(wr[i][j], x[j], a);
      v[i] = a;
      sum += a;
    }
    const float mean = wave_sum(sum) * (1.0f / (float)C);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i) { v[i] -= mean; q = fmaf(v[i], v[i], q); }
    const float rstd = rsqrtf(wave_sum(q) * (1.0f / (float)C) + eps);
    float o[CPL];
#pragma unroll
    for (int i = 0; i < CPL; ++i) o[i] = gelu_erf(fmaf(v[i] * rstd, g[i], be[i]));
    bf16_t* p = orow + (long)t * C;
    if constexpr (CPL == 8) {
      *(uint4*)p = make_uint4(pack2bf(o[0], o[1]), pack2bf(o[2], o[3]), pack2bf(o[4], o[5]), pack2bf(o[6], o[7]));
    } else if constexpr (CPL == 4) {
      *(uint2*)p = make_uint2(pack2bf(o[0], o[1]), pack2bf(o[2], o[3]));
    } else if constexpr (CPL == 2) {
      *(uint32_t*)p = pack2bf(o[0], o[1]);
    } else {
      p[0] = f2bf(o[0]);
    }
  }
}

struct W2vWs {
  float *part, *stats, *xr, *xr2, *logits;
  bf16_t *xa, *xb, *cc, *cn, *xn, *qkv, *ao, *hf;
  size_t bytes;
};
W2vWs w2v_carve(const ta_wav2vec2_weights* w, int B, int Ls, long rows, void* base) {
  const int C = w->conv_dim, H = w->hidden;
  const long T0 = w2v_frames(Ls, 1), T1 = w2v_frames(Ls, 2);
  const long nchunk = (T0 + W2V_CHUNK - 1) / W2V_CHUNK;
  Carver c(base);
  W2vWs e;
  e.part = c.take<float>((size_t)B * nchunk * C * 2);
  e.stats = c.take<float>((size_t)B * C * 2);
  // the conv stack ping-pongs between two equal-stride slab buffers: layer l's output is [B, Tmax_l, C], Tmax_l from Ls.  A valid
  // output row of a clip reads only that clip's valid input rows (no padding in these convolutions); the rows between a clip's
  // own length and Tmax_l are computed from rows nobody wrote and never consumed.  Every read stays inside the slab of its clip.
  e.xa = c.take<bf16_t>((size_t)B * T0 * C);
  e.xb = c.take<bf16_t>((size_t)B * T1 * C);
  e.cc = c.take<bf16_t>((size_t)rows * C);
  e.cn = c.take<bf16_t>((size_t)rows * C);
  e.xr = c.take<float>((size_t)rows * H);        // the fp32 size whatever the mode: sizes do not depend on res_f32
  e.xr2 = c.take<float>((size_t)rows * H);
  e.xn = c.take<bf16_t>((size_t)rows * H);
  e.qkv = c.take<bf16_t>((size_t)rows * 3 * H + (size_t)64 * 3 * H);
  e.ao = c.take<bf16_t>((size_t)rows * H);
  e.hf = c.take<bf16_t>((size_t)rows * w->ffn);
  e.logits = c.take<float>((size_t)rows * W2V_HEAD_PAD);
  e.bytes = c.total();
  return e;
}
}  // namespace

extern "C" long ta_w2v_conv0_ws_bytes(int B, int Ls, int C) {
  if (B <= 0 || Ls <= 0 || C <= 0) return 0;
  const long nchunk = (w2v_t0(Ls) + W2V_CHUNK - 1) / W2V_CHUNK;
  return ((long)B * nchunk * C * 2 + (long)B * C * 2) * 4 + 256;
}

extern "C" int ta_w2v_conv0_gn_gelu(const float* wav, const int* lens_dev, int B, int Ls, const float* w, const float* gn_w,
                                    const float* gn_b, int C, float eps, void* out_bf16, long out_rpb, void* ws, long ws_bytes,
                                    hipStream_t st) {
  if (B <= 0) return TA_OK;
  if (!wav || !lens_dev || !w || !gn_w || !gn_b || !out_bf16 || !ws || C <= 0 || B > 65535 || Ls < W2V_K0) return TA_ERR_ARG;
  const int T0 = w2v_t0(Ls);
  if (out_rpb < T0 || ws_bytes < ta_w2v_conv0_ws_bytes(B, Ls, C)) return TA_ERR_ARG;
  const int nchunk = (T0 + W2V_CHUNK - 1) / W2V_CHUNK;
  float* part = (float*)ws;
  float* stats = part + (long)B * nchunk * C * 2;
  TA_LAUNCH((w2v_conv0_kernel<0>), dim3(nchunk, B), dim3(256), 0, st, wav, Ls, lens_dev, w, C, nchunk, part, (const float*)nullptr,
            (const float*)nullptr, (const float*)nullptr, (bf16_t*)nullptr, 0L);
  TA_CHECK_LAUNCH();
  TA_LAUNCH(w2v_conv0_merge_kernel, dim3(ta_cdiv(C, 256), B), dim3(256), 0, st, (const float*)part, lens_dev, Ls, C, nchunk, eps, stats);
  TA_CHECK_LAUNCH();
  TA_LAUNCH((w2v_conv0_kernel<1>), dim3(nchunk, B), dim3(256), 0, st, wav, Ls, lens_dev, w, C, nchunk, (float*)nullptr,
            (const float*)stats, gn_w, gn_b, (bf16_t*)out_bf16, out_rpb);
  TA_CHECK_LAUNCH();
  return TA_OK;
}

extern "C" int ta_w2v_pos_conv(const void* x, int x_f32, const void* wp, const float* bias, void* y, const int* cu_rows, int B,
                               int max_rows, int H, hipStream_t st) {
  if (B <= 0 || max_rows <= 0) return TA_OK;
  if (!x || !wp || !bias || !y || !cu_rows || x == y || H <= 0 || H % W2V_POS_GROUPS || B > 65535) return TA_ERR_ARG;
  const int cg = H / W2V_POS_GROUPS;
  if (cg % 8 || cg > 64) return TA_ERR_ARG;
  const int nb = (cg + 15) / 16;
  const dim3 grid(ta_cdiv(max_rows, W2V_POS_TILE), W2V_POS_GROUPS, B);
  const size_t lds = (size_t)(W2V_POS_TILE + W2V_POS_K - 1) * cg * sizeof(bf16_t);
  with_const<1, 2, 3, 4>(nb, [&](auto n) {
    with_bool(x_f32 != 0, [&](auto f) {
      TA_LAUNCH((w2v_pos_conv_kernel<decltype(n)::value, decltype(f)::value>), grid, dim3(256), lds, st, x, y, (const bf16_t*)wp, bias,
                cu_rows, H, cg);
    });
  });
  TA_CHECK_LAUNCH();
  return TA_OK;
}

extern "C" int ta_w2v_head_logsoftmax(const float* logits, long ld, const float* bias, int n_classes, float* out, int rows,
                                      hipStream_t st) {
  if (rows <= 0) return TA_OK;
  if (!logits || !bias || !out || n_classes < 1 || n_classes > W2V_HEAD_PAD || ld < n_classes) return TA_ERR_ARG;
  TA_LAUNCH(w2v_head_kernel, dim3(ta_cdiv(rows, 4)), dim3(256), 0, st, logits, ld, bias, n_classes, out, rows);
  TA_CHECK_LAUNCH();
  return TA_OK;
}

extern "C" long ta_wav2vec2_workspace_bytes(const ta_wav2vec2_weights* w, int B, int Ls, long rows) {
  if (!w || B <= 0 || Ls < 400) return 0;
  return (long)w2v_carve(w, B, Ls, rows < 0 ? 0 : rows, nullptr).bytes;
}

extern "C" int ta_wav2vec2_forward(const ta_wav2vec2_weights* w, const float* wav, const int* lens_host, const int* lens_dev,
                                   const int* cu_frames_dev, int B, int Ls, float* emissions, void* ws, long ws_bytes, hipStream_t st) {
  if (B <= 0) return TA_OK;
  if (!w || !wav || !lens_host || !lens_dev || !cu_frames_dev || !emissions || !ws || B > 65535) return TA_ERR_ARG;
  const int C = w->conv_dim, H = w->hidden, F = w->ffn, nh = w->heads, NC = w->n_classes;
  if (C <= 0 || C % 64 || H % 128 || F % 128 || nh <= 0 || H != nh * 64 || NC < 1 || NC > W2V_HEAD_PAD || w->n_layers < 0) return TA_ERR_ARG;
  if ((H / W2V_POS_GROUPS) % 8 || H / W2V_POS_GROUPS > 64) return TA_ERR_ARG;
  if (!w->conv0_w || !w->gn_w || !w->gn_b || !w->fp_ln_w || !w->fp_ln_b || !w->fp_w || !w->fp_b || !w->pos_w || !w->pos_b ||
      !w->enc_ln_w || !w->enc_ln_b || !w->head_w || !w->head_b || (w->n_layers > 0 && !w->layers))
    return TA_ERR_ARG;
  for (int l = 0; l < 6; ++l) if (!w->conv_w[l]) return TA_ERR_ARG;
  for (int l = 0; l < w->n_layers; ++l) {
    const ta_enc_layer& L = w->layers[l];
    if (!(L.wqkv_fa && L.bqkv_fa && L.wo && L.bo && L.w1 && L.b1 && L.w2 && L.b2 && L.ln1_w && L.ln1_b && L.ln2_w && L.ln2_b)) return TA_ERR_ARG;
  }
  long rows_l = 0; int max_rows = 0;
  for (int b = 0; b < B; ++b) {
    if (lens_host[b] < 400 || lens_host[b] > Ls) return TA_ERR_ARG;       // fewer than 400 samples leave no frame behind conv 6
    const int Tb = w2v_frames(lens_host[b]);
    rows_l += Tb; max_rows = Tb > max_rows ? Tb : max_rows;
  }
  const long widest = 3L * H > F ? 3L * H : F;
  if (rows_l > 0x7fffffffL / widest) return TA_ERR_ARG;
  int Tm[7];
  for (int l = 0; l < 7; ++l) Tm[l] = w2v_frames(Ls, l + 1);
  if ((long)B * Tm[1] > 0x7fffffffL) return TA_ERR_ARG;
  const int M = (int)rows_l;
  W2vWs e = w2v_carve(w, B, Ls, M, ws);
  if ((long)e.bytes > ws_bytes) return TA_ERR_ARG;
  // 1. feature extractor (TF:models/wav2vec2/modeling_wav2vec2.py Wav2Vec2GroupNormConvLayer, Wav2Vec2NoLayerNormConvLayer)
  RC(ta_w2v_conv0_gn_gelu(wav, lens_dev, B, Ls, w->conv0_w, w->gn_w, w->gn_b, C, 1e-5f, e.xa, Tm[0], e.part,
                          ta_w2v_conv0_ws_bytes(B, Ls, C), st));
  bf16_t *src = e.xa, *dst = e.xb;
  for (int l = 1; l < 7; ++l) {
    // output row t of a clip = the contiguous k C elements from its input row t s: one GEMM per layer, GELU in the epilogue
    RC(ta_gemm_bf16_nt(src, w->conv_w[l - 1], dst, B * Tm[l], C, W2V_KS[l] * C, (long)W2V_ST[l] * C, Tm[l], (long)Tm[l - 1] * C, C, Tm[l],
                       (long)Tm[l] * C, 0, nullptr, nullptr, 1, 1, 1, nullptr, st));
    bf16_t* t = src; src = dst; dst = t;
  }
  // 2. feature projection on the compact rows (Wav2Vec2FeatureProjection: LayerNorm(C) -> Linear(C -> H))
  RC(ta_i_compact_rows(src, e.cc, cu_frames_dev, B, Tm[6], M, C * 2, st));
  RC(ta_layernorm_bf16(e.cc, w->fp_ln_w, w->fp_ln_b, e.cn, nullptr, nullptr, M, C, w->ln_eps, st));
  const bool res_f32 = w->res_f32 != 0;
  const int rb = res_f32 ? 0 : 1;
  RC(gemm(e.cn, w->fp_w, e.xr, M, H, C, w->fp_b, nullptr, 0, rb, st));
  // 3. positional convolution + GELU + residual, then encoder.layer_norm (Wav2Vec2PositionalConvEmbedding, Wav2Vec2Encoder.forward)
  RC(ta_w2v_pos_conv(e.xr, res_f32 ? 1 : 0, w->pos_w, w->pos_b, e.xr2, cu_frames_dev, B, max_rows, H, st));
  // LayerNorm of stream buffer `in` into stream buffer `out`; the GEMM operand image is `out` itself on a bf16 stream, xn otherwise
  auto ln = [&](void* in, const float* gw, const float* gb, void* out) -> int {
    return rb ? ta_layernorm_bf16(in, gw, gb, out, nullptr, nullptr, M, H, w->ln_eps, st)
              : ta_layernorm_f32((const float*)in, gw, gb, e.xn, (float*)out, nullptr, M, H, w->ln_eps, st);
  };
  auto res_gemm = [&](const void* A, const void* Wm, int K, const float* bias, void* x) -> int {      // x += A Wm^T + bias
    if (rb) { ta_gemm_opts o = opts_none(); o.residual_bf16 = x; return gemm_opt(A, Wm, x, M, H, K, bias, nullptr, 0, 1, o, st); }
    return gemm(A, Wm, x, M, H, K, bias, (const float*)x, 0, 0, st);
  };
  void *cur = e.xr, *oth = e.xr2;
  RC(ln(oth, w->enc_ln_w, w->enc_ln_b, cur));
  // 4. post-LN layers (Wav2Vec2EncoderLayer): x = LN(x + out_proj(attn(x))); x = LN(x + W2 gelu(W1 x))
  for (int l = 0; l < w->n_layers; ++l) {
    const ta_enc_layer& L = w->layers[l];
    const void* a = rb ? cur : (void*)e.xn;
    RC(gemm(a, L.wqkv_fa, e.qkv, M, 3 * H, H, L.bqkv_fa, nullptr, 0, 1, st));
    RC(ta_attention_enc_fwd_varlen(e.qkv, e.ao, cu_frames_dev, B, nh, max_rows, st));
    RC(res_gemm(e.ao, L.wo, H, L.bo, cur));
    RC(ln(cur, L.ln1_w, L.ln1_b, oth));
    a = rb ? oth : (void*)e.xn;
    RC(gemm(a, L.w1, e.hf, M, F, H, L.b1, nullptr, 1, 1, st));
    RC(res_gemm(e.hf, L.w2, F, L.b2, oth));
    RC(ln(oth, L.ln2_w, L.ln2_b, cur));
  }
  // 5. lm_head at its zero-padded width, then bias + log-softmax over the real classes
  RC(gemm(rb ? cur : (void*)e.xn, w->head_w, e.logits, M, W2V_HEAD_PAD, H, nullptr, nullptr, 0, 0, st));
  RC(ta_w2v_head_logsoftmax(e.logits, W2V_HEAD_PAD, w->head_b, NC, emissions, M, st));
  return TA_OK;
}

// ============================================================================ the "layer-norm / stable" family: C ABI
namespace {
inline long w2v_norm_chunks(int Ls) { return ((long)Ls + W2V_NORM_CHUNK - 1) / W2V_NORM_CHUNK; }

struct W2vSlnWs {
  float *norm_ws, *wavn, *xr, *xr2, *logits;
  bf16_t *xa, *xb, *cc, *cn, *xn, *qkv, *ao, *hf;
  size_t bytes;
};
W2vSlnWs w2v_sln_carve(const ta_wav2vec2_sln_weights* w, int B, int Ls, long rows, void* base) {
  const int C = w->conv_dim, H = w->hidden;
  const long T0 = w2v_frames(Ls, 1), T1 = w2v_frames(Ls, 2);
  Carver c(base);
  W2vSlnWs e;
  e.norm_ws = c.take<float>((size_t)ta_w2v_input_norm_ws_bytes(B, Ls) / 4);      // chunk partials, then the clips' (mean, rstd)
  e.wavn = c.take<float>((size_t)B * Ls);        // taken whatever input_norm_eps says: sizes do not depend on it
  // conv layer l writes its GEMM into xb and its LayerNorm + GELU back into xa, both as [B, Tmax_l, C] slabs (Tmax_l from Ls):
  // a valid row of a clip reads only that clip's valid rows, and the rows behind a clip's own length are row-local garbage.
  e.xa = c.take<bf16_t>((size_t)B * T0 * C);
  e.xb = c.take<bf16_t>((size_t)B * T1 * C);
  e.cc = c.take<bf16_t>((size_t)rows * C);
  e.cn = c.take<bf16_t>((size_t)rows * C);
  e.xr = c.take<float>((size_t)rows * H);
  e.xr2 = c.take<float>((size_t)rows * H);
  e.xn = c.take<bf16_t>((size_t)rows * H);
  e.qkv = c.take<bf16_t>((size_t)rows * 3 * H + (size_t)64 * 3 * H);
  e.ao = c.take<bf16_t>((size_t)rows * H);
  e.hf = c.take<bf16_t>((size_t)rows * w->ffn);
  e.logits = c.take<float>((size_t)rows * W2V_HEAD_PAD);
  e.bytes = c.total();
  return e;
}
inline bool w2v_sln_geometry_ok(const ta_wav2vec2_sln_weights* w) {
  const int C = w->conv_dim, H = w->hidden, F = w->ffn, nh = w->heads, NC = w->n_classes;
  if (!(C == 64 || C == 128 || C == 256 || C == 512)) return false;
  if (H <= 0 || H % 128 || F <= 0 || F % 128 || nh <= 0 || H != nh * 64 || NC < 1 || NC > W2V_HEAD_PAD || w->n_layers < 0) return false;
  if ((H / W2V_POS_GROUPS) % 8 || H / W2V_POS_GROUPS > 64) return false;
  return w->input_norm_eps >= 0.f;
}
}  // namespace

extern "C" long ta_w2v_input_norm_ws_bytes(int B, int Ls) {
  if (B <= 0 || Ls <= 0) return 0;
  return ((long)B * w2v_norm_chunks(Ls) * 2 + (long)B * 2) * 4 + 256;
}

extern "C" int ta_w2v_input_norm(const float* wav, const int* lens_dev, int B, int Ls, float eps, float* out, void* ws, long ws_bytes,
                                 hipStream_t st) {
  if (B <= 0) return TA_OK;
  if (!wav || !lens_dev || !out || !ws || Ls <= 0 || B > 65535 || !(eps > 0.f) || ws_bytes < ta_w2v_input_norm_ws_bytes(B, Ls)) return TA_ERR_ARG;
  const long nchunk = w2v_norm_chunks(Ls);
  if (nchunk > 0x7fffffffL) return TA_ERR_ARG;
  float* part = (float*)ws;
  float* stats = part + (long)B * nchunk * 2;
  TA_LAUNCH(w2v_norm_stats_kernel, dim3((unsigned)nchunk, B), dim3(256), 0, st, wav, Ls, lens_dev, (int)nchunk, part);
  TA_CHECK_LAUNCH();
  TA_LAUNCH(w2v_norm_merge_kernel, dim3(B), dim3(64), 0, st, (const float*)part, lens_dev, Ls, (int)nchunk, eps, stats);
  TA_CHECK_LAUNCH();
  TA_LAUNCH(w2v_norm_apply_kernel, dim3(ta_cdiv(Ls, 1024), B), dim3(256), 0, st, wav, Ls, lens_dev, (const float*)stats, out);
  TA_CHECK_LAUNCH();
  return TA_OK;
}

extern "C" int ta_w2v_conv0_ln_gelu(const float* wav, const int* lens_dev, int B, int Ls, const float* w, const float* bias,
                                    const float* ln_w, const float* ln_b, int C, float eps, void* out_bf16, long out_rpb, hipStream_t st) {
  if (B <= 0) return TA_OK;
  if (!wav || !lens_dev || !w || !bias || !ln_w || !ln_b || !out_bf16 || B > 65535 || Ls < W2V_K0) return TA_ERR_ARG;
  if (!(C == 64 || C == 128 || C == 256 || C == 512)) return TA_ERR_ARG;
  const int T0 = w2v_t0(Ls);
  if (out_rpb < T0) return TA_ERR_ARG;
  const int nchunk = (T0 + W2V_CHUNK - 1) / W2V_CHUNK;
  with_const<1, 2, 4, 8>(C / 64, [&](auto cpl) {
    TA_LAUNCH((w2v_conv0_ln_kernel<decltype(cpl)::value>), dim3(nchunk, B), dim3(256), 0, st, wav, Ls, lens_dev, w, bias, ln_w, ln_b, eps,
              (bf16_t*)out_bf16, out_rpb);
  });
  TA_CHECK_LAUNCH();
  return TA_OK;
}

extern "C" long ta_wav2vec2_sln_workspace_bytes(const ta_wav2vec2_sln_weights* w, int B, int Ls, long rows) {
  if (!w || B <= 0 || Ls < 400) return 0;
  return (long)w2v_sln_carve(w, B, Ls, rows < 0 ? 0 : rows, nullptr).bytes;
}

extern "C" int ta_wav2vec2_sln_ws_offsets(const ta_wav2vec2_sln_weights* w, int B, int Ls, long rows, long* feat_off, long* stream_off) {
  if (!w || B <= 0 || Ls < 400 || rows < 0 || !feat_off || !stream_off) return TA_ERR_ARG;
  char* const origin = (char*)4096;                      // (the carver hands out null pointers from a null base)
  const W2vSlnWs e = w2v_sln_carve(w, B, Ls, rows, origin);
  *feat_off = (long)((char*)e.cc - origin);
  *stream_off = (long)((char*)e.xr2 - origin);
  return TA_OK;
}

extern "C" int ta_wav2vec2_sln_forward(const ta_wav2vec2_sln_weights* w, const float* wav, const int* lens_host, const int* lens_dev,
                                       const int* cu_frames_dev, int B, int Ls, float* emissions, void* ws, long ws_bytes, hipStream_t st) {
  if (B <= 0) return TA_OK;
  if (!w || !wav || !lens_host || !lens_dev || !cu_frames_dev || !emissions || !ws || B > 65535) return TA_ERR_ARG;
  if (!w2v_sln_geometry_ok(w)) return TA_ERR_ARG;
  const int C = w->conv_dim, H = w->hidden, F = w->ffn, nh = w->heads, NC = w->n_classes;
  if (!w->conv0_w || !w->fp_ln_w || !w->fp_ln_b || !w->fp_w || !w->fp_b || !w->pos_w || !w->pos_b || !w->enc_ln_w || !w->enc_ln_b ||
      !w->head_w || !w->head_b || (w->n_layers > 0 && !w->layers))
    return TA_ERR_ARG;
  for (int l = 0; l < 7; ++l) if (!w->conv_b[l] || !w->conv_ln_w[l] || !w->conv_ln_b[l] || (l < 6 && !w->conv_w[l])) return TA_ERR_ARG;
  for (int l = 0; l < w->n_layers; ++l) {
    const ta_enc_layer& L = w->layers[l];
    if (!(L.wqkv_fa && L.bqkv_fa && L.wo && L.bo && L.w1 && L.b1 && L.w2 && L.b2 && L.ln1_w && L.ln1_b && L.ln2_w && L.ln2_b)) return TA_ERR_ARG;
  }
  long rows_l = 0; int max_rows = 0;
  for (int b = 0; b < B; ++b) {
    if (lens_host[b] < 400 || lens_host[b] > Ls) return TA_ERR_ARG;
    const int Tb = w2v_frames(lens_host[b]);
    rows_l += Tb; max_rows = Tb > max_rows ? Tb : max_rows;
  }
  const long widest = 3L * H > F ? 3L * H : F;
  if (rows_l > 0x7fffffffL / widest) return TA_ERR_ARG;
  int Tm[7];
  for (int l = 0; l < 7; ++l) Tm[l] = w2v_frames(Ls, l + 1);
  if ((long)B * Tm[1] > 0x7fffffffL) return TA_ERR_ARG;
  const int M = (int)rows_l;
  W2vSlnWs e = w2v_sln_carve(w, B, Ls, M, ws);
  if ((long)e.bytes > ws_bytes) return TA_ERR_ARG;
  // 0. Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm / torchaudio's layer_norm(waveform, waveform.shape), each clip's own samples
  const float* x0 = wav;
  if (w->input_norm_eps > 0.f) {
    RC(ta_w2v_input_norm(wav, lens_dev, B, Ls, w->input_norm_eps, e.wavn, e.norm_ws, ta_w2v_input_norm_ws_bytes(B, Ls), st));
    x0 = e.wavn;
  }
  // 1. feature extractor (TF:models/wav2vec2/modeling_wav2vec2.py Wav2Vec2LayerNormConvLayer x 7); nn.LayerNorm's own eps, not ln_eps
  RC(ta_w2v_conv0_ln_gelu(x0, lens_dev, B, Ls, w->conv0_w, w->conv_b[0], w->conv_ln_w[0], w->conv_ln_b[0], C, 1e-5f, e.xa, Tm[0], st));
  for (int l = 1; l < 7; ++l) {
    // output row t of a clip = the contiguous k C elements from its input row t s: one GEMM per layer with the bias in its
    // epilogue, then LayerNorm + GELU as one row-wise pass back into xa at this layer's slab stride
    RC(ta_gemm_bf16_nt(e.xa, w->conv_w[l - 1], e.xb, B * Tm[l], C, W2V_KS[l] * C, (long)W2V_ST[l] * C, Tm[l], (long)Tm[l - 1] * C, C, Tm[l],
                       (long)Tm[l] * C, 0, w->conv_b[l], nullptr, 0, 1, 1, nullptr, st));
    RC(ta_layernorm_gelu_bf16(e.xb, w->conv_ln_w[l], w->conv_ln_b[l], e.xa, B * Tm[l], C, 1e-5f, st));
  }
  // 2. feature projection on the compact rows (Wav2Vec2FeatureProjection: LayerNorm(C) -> Linear(C -> H))
  RC(ta_i_compact_rows(e.xa, e.cc, cu_frames_dev, B, Tm[6], M, C * 2, st));
  RC(ta_layernorm_bf16(e.cc, w->fp_ln_w, w->fp_ln_b, e.cn, nullptr, nullptr, M, C, w->ln_eps, st));
  const bool res_f32 = w->res_f32 != 0;
  const int rb = res_f32 ? 0 : 1;
  RC(gemm(e.cn, w->fp_w, e.xr, M, H, C, w->fp_b, nullptr, 0, rb, st));
  // 3. x = x + gelu(pos_conv(x)): no LayerNorm here (Wav2Vec2EncoderStableLayerNorm.forward)
  void* x = e.xr2;
  RC(ta_w2v_pos_conv(e.xr, res_f32 ? 1 : 0, w->pos_w, w->pos_b, x, cu_frames_dev, B, max_rows, H, st));
  auto ln = [&](const float* gw, const float* gb) -> int {                     // xn = LayerNorm(x): the next GEMM's bf16 operand
    return rb ? ta_layernorm_bf16(x, gw, gb, e.xn, nullptr, nullptr, M, H, w->ln_eps, st)
              : ta_layernorm_f32((const float*)x, gw, gb, e.xn, nullptr, nullptr, M, H, w->ln_eps, st);
  };
  auto res_gemm = [&](const void* A, const void* Wm, int K, const float* bias) -> int {               // x += A Wm^T + bias
    if (rb) { ta_gemm_opts o = opts_none(); o.residual_bf16 = x; return gemm_opt(A, Wm, x, M, H, K, bias, nullptr, 0, 1, o, st); }
    return gemm(A, Wm, x, M, H, K, bias, (const float*)x, 0, 0, st);
  };
  // 4. pre-LN layers (Wav2Vec2EncoderLayerStableLayerNorm): x += out_proj(attn(LN(x))); x += W2 gelu(W1 LN(x))
  for (int l = 0; l < w->n_layers; ++l) {
    const ta_enc_layer& L = w->layers[l];
    RC(ln(L.ln1_w, L.ln1_b));
    RC(gemm(e.xn, L.wqkv_fa, e.qkv, M, 3 * H, H, L.bqkv_fa, nullptr, 0, 1, st));
    RC(ta_attention_enc_fwd_varlen(e.qkv, e.ao, cu_frames_dev, B, nh, max_rows, st));
    RC(res_gemm(e.ao, L.wo, H, L.bo));
    RC(ln(L.ln2_w, L.ln2_b));
    RC(gemm(e.xn, L.w1, e.hf, M, F, H, L.b1, nullptr, 1, 1, st));
    RC(res_gemm(e.hf, L.w2, F, L.b2));
  }
  // 5. encoder.layer_norm behind the last layer, lm_head at its zero-padded width, bias + log-softmax over the real classes
  RC(ln(w->enc_ln_w, w->enc_ln_b));
  RC(gemm(e.xn, w->head_w, e.logits, M, W2V_HEAD_PAD, H, nullptr, nullptr, 0, 0, st));
  RC(ta_w2v_head_logsoftmax(e.logits, W2V_HEAD_PAD, w->head_b, NC, emissions, M, st));
  return TA_OK;
}
