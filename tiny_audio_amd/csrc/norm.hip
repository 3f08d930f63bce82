// ta355 row-normalisation kernels (HBM-bound): one 64-lane wave per row, the row held in
// registers (float4 per lane, up to 5120 columns), wave-shuffle reductions, 16-byte accesses.
//
//   layernorm_kernel     nn.LayerNorm of the GLM-ASR encoder  (TF:models/glmasr/modeling_glmasr.py:246-247,305)
//   rmsnorm_fwd_kernel   Qwen3RMSNorm / LlamaRMSNorm            (TF:models/qwen3/modeling_qwen3.py:50-64;
//                        tiny_audio/projectors.py:43,50), optionally fused with the projector's erf-GELU
//   rmsnorm_bwd_kernel   its backward (dx, optional dw, optional GELU' prologue, optional residual add)
//
// The *_x8_kernel variants give HALF a wave to a row (8 columns per lane and chunk) and are templated on the row's element type;
// how a row of that type is read is RowLoad<T>'s business.
#include <cstdlib>
#include <type_traits>
#include "common.h"
#include "internal.h"

#define MAXV_LIMIT 20   // float4 per lane -> rows up to 64*4*20 = 5120 columns
// MAXV (float4 per lane held in registers) is a template parameter: 4 (H<=1024), 8 (<=2048), 20 (<=5120)

// ----------------------------------------------------------------------------- row loaders
// RowLoad<T>: how a lane reads its columns of a row of T (bf16_t or float).
//   load4(row, c)          the 4-column chunk c of the row -> float4 (the wave-per-row kernels)
//   raw8(row, c, raw)      the 16-byte load(s) of the 8-column chunk c, still packed (Raw8): a kernel that requests the next row early
//                          keeps these registers
//   unpack8(raw, v)        -> float[8];  bf16 only: unpack2(raw, j, v), the pair in 32-bit word j -> float[2]
//   PAIR_SUMS              the order in which a half-wave forward kernel adds a lane's eight values (or their squares) to its running
//                          sum: bf16 pair by pair, each pair as it is unpacked; f32 one element at a time, which also contracts to FMAs
//                          differently.  The kernels these loaders were factored out of differed in this, and both orders are kept so
//                          that every output keeps its bits.  The kernels write the two loops out under `if constexpr` instead of calling
//                          a member: which of the variance's multiply-adds the compiler vectorises (packed multiply + add) and which
//                          it contracts to FMAs follows the order of the instructions it is given, and a call around the running sum or
//                          a bf16 row unpacked ahead of its sum changes that order and with it the last bit (profiles/norm_refactor.md).
template <typename T> struct RowLoad;

template <> struct RowLoad<float> {
  typedef float4 Raw8[2];
  static __device__ __forceinline__ float4 load4(const float* row, int c) { return ((const float4*)row)[c]; }
  static __device__ __forceinline__ void raw8(const float* row, int c, Raw8& r) { r[0] = ((const float4*)row)[c * 2]; r[1] = ((const float4*)row)[c * 2 + 1]; }
  static __device__ __forceinline__ void unpack8(const Raw8& r, float* v) {
    v[0] = r[0].x; v[1] = r[0].y; v[2] = r[0].z; v[3] = r[0].w; v[4] = r[1].x; v[5] = r[1].y; v[6] = r[1].z; v[7] = r[1].w;
  }
  static constexpr bool PAIR_SUMS = false;
};

template <> struct RowLoad<bf16_t> {
  typedef uint4 Raw8;
  static __device__ __forceinline__ float4 load4(const bf16_t* row, int c) {
    const uint2 u = ((const uint2*)row)[c];
    return make_float4(bf2f((bf16_t)(u.x & 0xffff)), bf2f((bf16_t)(u.x >> 16)), bf2f((bf16_t)(u.y & 0xffff)), bf2f((bf16_t)(u.y >> 16)));
  }
  static __device__ __forceinline__ void raw8(const bf16_t* row, int c, Raw8& r) { r = ((const uint4*)row)[c]; }
  static __device__ __forceinline__ void unpack2(const Raw8& r, int j, float* v) {      // the pair in 32-bit word j -> float[2]
    const uint32_t t = j == 0 ? r.x : (j == 1 ? r.y : (j == 2 ? r.z : r.w));
    v[0] = bf2f((bf16_t)(t & 0xffff)); v[1] = bf2f((bf16_t)(t >> 16));
  }
  static __device__ __forceinline__ void unpack8(const Raw8& r, float* v) {
#pragma unroll
    for (int j = 0; j < 4; ++j) unpack2(r, j, v + 2 * j);
  }
  static constexpr bool PAIR_SUMS = true;
};

// the element type behind a kernel's "this operand is bf16" flag
template <bool BF16> using elem_t = std::conditional_t<BF16, bf16_t, float>;

// eight consecutive f32 of a per-column vector (gamma, beta, the RMSNorm weight) -> float[8]
__device__ __forceinline__ void load_cols8(const float* p, float* o) {
  const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
  o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
}

__device__ __forceinline__ uint4 pack8bf(const float* o) {
  return make_uint4(pack2bf(o[0], o[1]), pack2bf(o[2], o[3]), pack2bf(o[4], o[5]), pack2bf(o[6], o[7]));
}

// ----------------------------------------------------------------------------- LayerNorm
// IN_BF16: the row is read as bf16 (the encoder's bf16 residual stream, as the reference's bf16 model keeps it)
// ACT: what is applied to the normalised row before it is stored -- 0 nothing, 1 exact-erf GELU (wav2vec2's LayerNorm conv layers:
// LayerNorm over the channels, then GELU, as one pass over the rows)
template <int MAXV, bool OUT_BF16, bool OUT_F32, bool IN_BF16 = false, int ACT = 0>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ b, bf16_t* __restrict__ yb,
                                                        float* __restrict__ yf, const float* __restrict__ rowscale,
                                                        int M, int H, float eps) {
  using X = elem_t<IN_BF16>;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int lane = threadIdx.x & 63;
  const int nv = H >> 2;
  const X* xr = (const X*)x + (long)row * H;
  float4 v[MAXV];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = lane + i * 64;
    if (c < nv) {
      v[i] = RowLoad<X>::load4(xr, c);
      s += v[i].x + v[i].y + v[i].z + v[i].w;
    }
  }
  const float mean = wave_sum(s) / (float)H;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = lane + i * 64;
    if (c < nv) {
      const float a = v[i].x - mean, bq = v[i].y - mean, cq = v[i].z - mean, d = v[i].w - mean;
      q += a * a + bq * bq + cq * cq + d * d;
    }
  }
  const float rstd = rsqrtf(wave_sum(q) / (float)H + eps);
  const float rs = rowscale ? rowscale[row] : 1.0f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = lane + i * 64;
    if (c < nv) {
      const float4 ww = ((const float4*)w)[c], bb = ((const float4*)b)[c];
      float4 o;
      o.x = ((v[i].x - mean) * rstd * ww.x + bb.x) * rs;
      o.y = ((v[i].y - mean) * rstd * ww.y + bb.y) * rs;
      o.z = ((v[i].z - mean) * rstd * ww.z + bb.z) * rs;
      o.w = ((v[i].w - mean) * rstd * ww.w + bb.w) * rs;
      if constexpr (ACT == 1) { o.x = gelu_erf(o.x); o.y = gelu_erf(o.y); o.z = gelu_erf(o.z); o.w = gelu_erf(o.w); }
      if (OUT_F32) ((float4*)(yf + (long)row * H))[c] = o;
      if (OUT_BF16) {
        uint2 p; p.x = pack2bf(o.x, o.y); p.y = pack2bf(o.z, o.w);
        ((uint2*)(yb + (long)row * H))[c] = p;
      }
    }
  }
}


// bf16 / f32 -> bf16 LayerNorm with 16-byte accesses: HALF a wave per row (32 lanes x NCH chunks of 8 columns, H = 256 * NCH),
// two rows per wave, eight per workgroup.  The encoder's two LayerNorms per layer read and write the bf16 residual stream
// (82 MB per call at B = 32): halving the number of memory instructions per byte is what this variant is for.
// Round 3: a half wave walks ROWS rows and keeps its gamma / beta columns in registers.  With one row per half wave every
// lane re-read 8 x NCH floats of gamma and of beta per row from L1 -- 4x the bytes of the row itself (20 KB of L1 reads per
// 2.5-KB row at H = 1280: ~8 of the kernel's 16 us at 64 B/clk/CU); the next row's chunks are requested before the current
// row's arithmetic.
// T = float is the fp32-stream mode of the encoder (round 6): two 16-byte loads and one 16-byte store per chunk and lane.  The generic
// wave-per-row kernel it replaces there re-read gamma and beta (10 KB) for every 5-KB row: 24.4 us per launch at B = 32 (123 MB:
// 5.0 TB/s).
// ACT: as layernorm_kernel's.
template <typename T, int NCH, int ROWS, int ACT = 0>
__global__ __launch_bounds__(256) void layernorm_x8_kernel(const T* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ b, bf16_t* __restrict__ y,
                                                           const float* __restrict__ rowscale, int M, float eps) {
  using L = RowLoad<T>;
  constexpr int H = NCH * 256;
  const int l = threadIdx.x & 31;
  const int row0 = (blockIdx.x * 8 + (threadIdx.x >> 5)) * ROWS;
  if (row0 >= M) return;
  float ww[NCH][8], bb[NCH][8];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = (l + i * 32) * 8;
    load_cols8(w + c, ww[i]);
    load_cols8(b + c, bb[i]);
  }
  typename L::Raw8 nx[NCH];
  {
    const T* xr = x + (long)row0 * H;
#pragma unroll
    for (int i = 0; i < NCH; ++i) L::raw8(xr, l + i * 32, nx[i]);
  }
#pragma unroll 1
  for (int rr = 0; rr < ROWS; ++rr) {
    const int row = row0 + rr;
    if (row >= M) break;                               // (uniform per half wave: the shuffles below stay inside it)
    float v[NCH][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      if constexpr (L::PAIR_SUMS) {                    // (RowLoad: the two orders keep both element types' bits; bf16 adds each pair as it unpacks it)
#pragma unroll
        for (int j = 0; j < 4; ++j) { L::unpack2(nx[i], j, v[i] + 2 * j); s += v[i][2 * j] + v[i][2 * j + 1]; }
      } else {
        L::unpack8(nx[i], v[i]);
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[i][j];
      }
    }
    if (rr + 1 < ROWS && row + 1 < M) {
      const T* xr = x + (long)(row + 1) * H;
#pragma unroll
      for (int i = 0; i < NCH; ++i) L::raw8(xr, l + i * 32, nx[i]);
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);          // lanes 0-31 / 32-63 reduce separately
    const float mean = s / (float)H;
    float q2 = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float d = v[i][j] - mean; q2 += d * d; }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) q2 += __shfl_xor(q2, o, 64);
    const float rstd = rsqrtf(q2 / (float)H + eps);
    const float rs = rowscale ? rowscale[row] : 1.0f;
    uint4* yr = (uint4*)(y + (long)row * H);
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = ((v[i][j] - mean) * rstd * ww[i][j] + bb[i][j]) * rs;
      if constexpr (ACT == 1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = gelu_erf(o[j]);
      }
      yr[l + i * 32] = pack8bf(o);
    }
  }
}


// ----------------------------------------------------------------------------- RMSNorm forward
// bf16 / f32 -> bf16 RMSNorm (the LM's residual stream; T = float: its fp32-stream mode, round 6) with 16-byte accesses, half a wave
// per row: same layout idea as layernorm_x8_kernel.  H = 256 * NCH.
template <typename T, int NCH>
__global__ __launch_bounds__(256) void rmsnorm_fwd_x8_kernel(const T* __restrict__ x, const float* __restrict__ w,
                                                             bf16_t* __restrict__ y, float* __restrict__ rstd_out, int M,
                                                             float eps) {
  using L = RowLoad<T>;
  constexpr int H = NCH * 256;
  const int row = blockIdx.x * 8 + (threadIdx.x >> 5);
  if (row >= M) return;
  const int l = threadIdx.x & 31;
  const T* xr = x + (long)row * H;
  float v[NCH][8];
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    typename L::Raw8 u;
    L::raw8(xr, l + i * 32, u);
    L::unpack8(u, v[i]);
    if constexpr (L::PAIR_SUMS) {                      // (RowLoad: the two orders keep both element types' bits)
#pragma unroll
      for (int j = 0; j < 4; ++j) q += v[i][2 * j] * v[i][2 * j] + v[i][2 * j + 1] * v[i][2 * j + 1];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) q += v[i][j] * v[i][j];
    }
  }
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
  const float rstd = rsqrtf(q / (float)H + eps);
  if (rstd_out && l == 0) rstd_out[row] = rstd;
  uint4* yr = (uint4*)(y + (long)row * H);
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    float ww[8], o[8];
    load_cols8(w + (l + i * 32) * 8, ww);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = v[i][j] * rstd * ww[j];
    yr[l + i * 32] = pack8bf(o);
  }
}

// y = w * (x * rstd)   [ACT==1: y = gelu(y)];  x f32 [M,H], or bf16 with IN_BF16
template <int MAXV, int ACT, bool IN_BF16 = false>
__global__ __launch_bounds__(256) void rmsnorm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          bf16_t* __restrict__ yb, float* __restrict__ yf,
                                                          float* __restrict__ rstd_out, int M, int H, float eps) {
  using X = elem_t<IN_BF16>;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int lane = threadIdx.x & 63;
  const int nv = H >> 2;
  const X* xr = (const X*)x + (long)row * H;
  float4 v[MAXV];
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = lane + i * 64;
    if (c < nv) {
      v[i] = RowLoad<X>::load4(xr, c);
      q += v[i].x * v[i].x + v[i].y * v[i].y + v[i].z * v[i].z + v[i].w * v[i].w;
    }
  }
  const float rstd = rsqrtf(wave_sum(q) / (float)H + eps);
  if (rstd_out && lane == 0) rstd_out[row] = rstd;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = lane + i * 64;
    if (c < nv) {
      const float4 ww = ((const float4*)w)[c];
      float4 o;
      o.x = v[i].x * rstd * ww.x; o.y = v[i].y * rstd * ww.y;
      o.z = v[i].z * rstd * ww.z; o.w = v[i].w * rstd * ww.w;
      if (ACT == 1) { o.x = gelu_erf(o.x); o.y = gelu_erf(o.y); o.z = gelu_erf(o.z); o.w = gelu_erf(o.w); }
      if (yf) ((float4*)(yf + (long)row * H))[c] = o;
      if (yb) {
        uint2 p; p.x = pack2bf(o.x, o.y); p.y = pack2bf(o.z, o.w);
        ((uint2*)(yb + (long)row * H))[c] = p;
      }
    }
  }
}

// ----------------------------------------------------------------------------- RMSNorm backward
// Backward of y = act(w * x * rstd):
//   dn = dy * act'(n)           (ACT==1, n = w*x*rstd recomputed)
//   dx = rstd * (dn*w - xh * mean(dn*w*xh)),  xh = x*rstd        (+ dres if given)
// DWM (weight gradient mode):
//   1 if dw != null: dw += sum_rows dn * xh with LDS partials + one atomicAdd per column per block (every launch without a workspace,
//     the exported ta_rmsnorm_bwd among them; the order of the float additions, hence the last bits, may change from run to run);
//   2 dw[block][:] = sum over the block's rows of dn * xh, then rmsnorm_dw_fold_kernel adds the blocks' slabs in order.  A lane keeps
//     its columns' sums in registers over the rows of its wave and the 4 waves fold through LDS in wave order: no float atomics, the
//     same bits on every run (the projector backward, which lends the slabs from its workspace).
// DRES_BF16 (round 4): the residual gradient `dres` is bf16 and may BE the output image dxb (in place: a lane reads its four
// elements before it writes them) -- the LM's d(x) stream kept in bf16, the dtype the reference's bf16 model back-propagates in
template <int MAXV, int ACT, bool X_BF16 = false, bool DY_BF16 = false, bool DRES_BF16 = false, int DWM = 1>
__global__ __launch_bounds__(256) void rmsnorm_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                          const float* __restrict__ rstd_in,
                                                          const float* __restrict__ w, const float* dres,
                                                          float* dxf, bf16_t* dxb,
                                                          float* __restrict__ dw, int M, int H) {
  using X = elem_t<X_BF16>;
  using DY = elem_t<DY_BF16>;
  using DRES = elem_t<DRES_BF16>;
  extern __shared__ float dw_lds[];   // [H] when dw != null
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nv = H >> 2;
  constexpr int NA = DWM == 2 ? MAXV : 1;
  float4 dwa[NA];
  if constexpr (DWM == 2) {
#pragma unroll
    for (int i = 0; i < NA; ++i) dwa[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (DWM == 1 && dw) {
    for (int i = threadIdx.x; i < H; i += 256) dw_lds[i] = 0.f;
    __syncthreads();
  }
  // each block handles rows_per_block consecutive groups of 4 rows (grid-stride) so dw atomics / slabs stay few
  for (int row0 = blockIdx.x * 4; row0 < M; row0 += gridDim.x * 4) {
    const int row = row0 + wv;
    if (row < M) {
      const float r = rstd_in[row];
      const X* xr = (const X*)x + (long)row * H;
      const DY* dr = (const DY*)dy + (long)row * H;
      float4 xh[MAXV], dn[MAXV];
      float dot = 0.f;
#pragma unroll
      for (int i = 0; i < MAXV; ++i) {
        const int c = lane + i * 64;
        if (c < nv) {
          const float4 xv = RowLoad<X>::load4(xr, c);
          const float4 dv = RowLoad<DY>::load4(dr, c);
          const float4 ww = ((const float4*)w)[c];
          xh[i] = make_float4(xv.x * r, xv.y * r, xv.z * r, xv.w * r);
          float4 d = dv;
          if (ACT == 1) {
            d.x *= gelu_erf_grad(xh[i].x * ww.x); d.y *= gelu_erf_grad(xh[i].y * ww.y);
            d.z *= gelu_erf_grad(xh[i].z * ww.z); d.w *= gelu_erf_grad(xh[i].w * ww.w);
          }
          if (DWM == 1 && dw) {
            atomicAdd(&dw_lds[c * 4 + 0], d.x * xh[i].x); atomicAdd(&dw_lds[c * 4 + 1], d.y * xh[i].y);
            atomicAdd(&dw_lds[c * 4 + 2], d.z * xh[i].z); atomicAdd(&dw_lds[c * 4 + 3], d.w * xh[i].w);
          }
          if constexpr (DWM == 2) {
            dwa[i].x += d.x * xh[i].x; dwa[i].y += d.y * xh[i].y; dwa[i].z += d.z * xh[i].z; dwa[i].w += d.w * xh[i].w;
          }
          dn[i] = make_float4(d.x * ww.x, d.y * ww.y, d.z * ww.z, d.w * ww.w);
          dot += dn[i].x * xh[i].x + dn[i].y * xh[i].y + dn[i].z * xh[i].z + dn[i].w * xh[i].w;
        }
      }
      const float mdot = wave_sum(dot) / (float)H;
#pragma unroll
      for (int i = 0; i < MAXV; ++i) {
        const int c = lane + i * 64;
        if (c < nv) {
          float4 o;
          o.x = r * (dn[i].x - xh[i].x * mdot); o.y = r * (dn[i].y - xh[i].y * mdot);
          o.z = r * (dn[i].z - xh[i].z * mdot); o.w = r * (dn[i].w - xh[i].w * mdot);
          if (dres) {
            const float4 e = RowLoad<DRES>::load4((const DRES*)dres + (long)row * H, c);
            o.x += e.x; o.y += e.y; o.z += e.z; o.w += e.w;
          }
          if (dxf) ((float4*)(dxf + (long)row * H))[c] = o;
          if (dxb) {
            uint2 p; p.x = pack2bf(o.x, o.y); p.y = pack2bf(o.z, o.w);
            ((uint2*)(dxb + (long)row * H))[c] = p;
          }
        }
      }
    }
  }
  if (DWM == 1 && dw) {
    __syncthreads();
    for (int i = threadIdx.x; i < H; i += 256) atomicAdd(&dw[i], dw_lds[i]);
  }
  if constexpr (DWM == 2) {
    for (int v = 0; v < 4; ++v) {       // wave 0 stores, waves 1..3 add, in this order
      if (wv == v) {
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
          const int c = lane + i * 64;
          if (c < nv) {
            float4* p = (float4*)dw_lds + c;
            if (v == 0) *p = dwa[i];
            else { float4 q = *p; q.x += dwa[i].x; q.y += dwa[i].y; q.z += dwa[i].z; q.w += dwa[i].w; *p = q; }
          }
        }
      }
      __syncthreads();
    }
    for (int i = threadIdx.x; i < H; i += 256) dw[(long)blockIdx.x * H + i] = dw_lds[i];
  }
}

// dw[c] += sum over the G slabs of rmsnorm_bwd_kernel<..., DWM = 2>, in slab order: 16 slab groups x 16 float4 columns per workgroup,
// group g adds slabs g, g + 16, ... and the 16 groups fold through LDS in group order
__global__ __launch_bounds__(256) void rmsnorm_dw_fold_kernel(const float* __restrict__ part, int G, int H, float* __restrict__ dw) {
  __shared__ float4 red[16][16];
  const int q = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int c4 = blockIdx.x * 16 + q, nv = H >> 2;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c4 < nv)
    for (int b = g; b < G; b += 16) {
      const float4 v = ((const float4*)(part + (long)b * H))[c4];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  red[g][q] = s;
  __syncthreads();
  if (g == 0 && c4 < nv) {
    float4 t = red[0][q];
    for (int k = 1; k < 16; ++k) { t.x += red[k][q].x; t.y += red[k][q].y; t.z += red[k][q].z; t.w += red[k][q].w; }
    float* o = dw + c4 * 4;
    o[0] += t.x; o[1] += t.y; o[2] += t.z; o[3] += t.w;
  }
}

// RMSNorm backward, half a wave per row with 16-byte accesses (round 6): the all-bf16 form the LM backward runs 56 times per step in the
// bf16-stream mode -- x, the incoming gradient, dres and the d(x) image bf16 (dres may BE dxb: the stream updated in place), optional
// f32 copy; no GELU, no weight gradient.  H = 256 * NCH.  11.3 -> 10.3 us per launch at M = 6144, H = 1024 (profiles/r06_g_*).  (The
// fp32-stream counterpart -- five streams, 100 MB per launch -- measured SLOWER in this layout, 19.5 against 18.6 us, and stays on the
// wave-per-row kernel: this kernel is not templated on the element type.)
template <int NCH>
__global__ __launch_bounds__(256) void rmsnorm_bwd_bf16x8_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                                 const float* __restrict__ rstd_in, const float* __restrict__ w,
                                                                 const bf16_t* dres, float* dxf, bf16_t* dxb, int M) {
  using L = RowLoad<bf16_t>;
  constexpr int H = NCH * 256;
  const int row = blockIdx.x * 8 + (threadIdx.x >> 5);
  if (row >= M) return;
  const int l = threadIdx.x & 31;
  const float r = rstd_in[row];
  float xh[NCH][8], dn[NCH][8];
  float dot = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c8 = l + i * 32;                                   // 8-column chunk index inside the row
    uint4 u, du;
    L::raw8(x + (long)row * H, c8, u);
    L::raw8(dy + (long)row * H, c8, du);
    float ww[8];
    load_cols8(w + c8 * 8, ww);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      float xv[2], d[2];
      L::unpack2(u, p, xv);
      L::unpack2(du, p, d);
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int j = 2 * p + k;
        xh[i][j] = xv[k] * r;
        dn[i][j] = d[k] * ww[j];
        dot += dn[i][j] * xh[i][j];
      }
    }
  }
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);          // lanes 0-31 / 32-63 reduce separately
  const float mdot = dot / (float)H;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c8 = l + i * 32;
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = r * (dn[i][j] - xh[i][j] * mdot);
    if (dres) {
      uint4 eu;
      float e[8];
      L::raw8(dres + (long)row * H, c8, eu);
      L::unpack8(eu, e);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] += e[j];
    }
    if (dxf) {
      float4* fr = (float4*)(dxf + (long)row * H);
      fr[c8 * 2] = make_float4(o[0], o[1], o[2], o[3]); fr[c8 * 2 + 1] = make_float4(o[4], o[5], o[6], o[7]);
    }
    if (dxb) ((uint4*)(dxb + (long)row * H))[c8] = pack8bf(o);
  }
}

// ----------------------------------------------------------------------------- C-ABI
// (with_const: common.h)
// H -> NCH = H / 256, the 8-column chunks per lane of a half-wave kernel
template <typename F> static void with_nch(int H, F&& f) { with_const<1, 2, 3, 4, 5, 6, 7, 8>(H / 256, f); }
// H -> MAXV, the float4 per lane a wave-per-row kernel holds
template <typename F> static void with_maxv(int H, F&& f) { with_const<4, 8, 20>(H <= 1024 ? 4 : (H <= 2048 ? 8 : 20), f); }

static bool norm_bad_H(int H) { return (H & 3) || H > 64 * 4 * MAXV_LIMIT; }
// the half-wave-per-row (*_x8) kernels take H a multiple of 256 up to 2048; other shapes: the wave-per-row kernels
static bool half_wave_H(int H) { return (H % 256) == 0 && H <= 2048; }

// ACT = 1 (GELU behind the norm) exists for bf16 rows with bf16 as the only output (wav2vec2's conv layers)
template <typename T, int ACT = 0>
static int layernorm_dispatch(const T* x, const float* w, const float* b, void* y_bf16, float* y_f32, const float* rowscale, int M, int H,
                              float eps, hipStream_t st) {
  if (M <= 0) return TA_OK;
  if (norm_bad_H(H) || (!y_bf16 && !y_f32)) return TA_ERR_ARG;
  if (ACT != 0 && (!y_bf16 || y_f32)) return TA_ERR_ARG;
  bf16_t* yb = (bf16_t*)y_bf16;
  const dim3 blk(256);
  if (y_bf16 && !y_f32 && half_wave_H(H)) {              // bf16 is the only output
    // rows per half wave: 4 once that still leaves >= 1 workgroup per CU (M = 16000 at B = 32: 500 workgroups; measured 41.62 /
    // 41.63 / 41.88 ms per step at 4 / 2 / 1, profiles/r03_k_ab_ln_rows.txt), 2 from 4096 rows, else 1
    const int rows = M >= 8 * 4 * 256 ? 4 : (M >= 8 * 2 * 256 ? 2 : 1);
    const dim3 g8(ta_cdiv(M, 8 * rows));
    with_nch(H, [&](auto nch) {
      with_const<4, 2, 1>(rows, [&](auto r) {
        TA_LAUNCH((layernorm_x8_kernel<T, decltype(nch)::value, decltype(r)::value, ACT>), g8, blk, 0, st, x, w, b, yb, rowscale, M, eps);
      });
    });
    TA_CHECK_LAUNCH();
    return TA_OK;
  }
  constexpr bool IN_BF16 = std::is_same_v<T, bf16_t>;
  const dim3 grid(ta_cdiv(M, 4));
  const float* xf = (const float*)x;
  with_maxv(H, [&](auto maxv) {
    constexpr int V = decltype(maxv)::value;
    if constexpr (ACT != 0) { TA_LAUNCH((layernorm_kernel<V, true, false, IN_BF16, ACT>), grid, blk, 0, st, xf, w, b, yb, y_f32, rowscale, M, H, eps); return; }
    if (y_bf16 && y_f32) TA_LAUNCH((layernorm_kernel<V, true, true, IN_BF16>), grid, blk, 0, st, xf, w, b, yb, y_f32, rowscale, M, H, eps);
    else if (y_bf16) TA_LAUNCH((layernorm_kernel<V, true, false, IN_BF16>), grid, blk, 0, st, xf, w, b, yb, y_f32, rowscale, M, H, eps);
    else TA_LAUNCH((layernorm_kernel<V, false, true, IN_BF16>), grid, blk, 0, st, xf, w, b, yb, y_f32, rowscale, M, H, eps);
  });
  TA_CHECK_LAUNCH();
  return TA_OK;
}

extern "C" int ta_layernorm_bf16(const void* x_bf16, const float* w, const float* b, void* y_bf16, float* y_f32,
                                 const float* rowscale, int M, int H, float eps, hipStream_t st) {
  return layernorm_dispatch((const bf16_t*)x_bf16, w, b, y_bf16, y_f32, rowscale, M, H, eps, st);
}

extern "C" int ta_layernorm_gelu_bf16(const void* x_bf16, const float* w, const float* b, void* y_bf16, int M, int H, float eps,
                                      hipStream_t st) {
  if (M > 0 && (!x_bf16 || !w || !b || !y_bf16 || x_bf16 == y_bf16)) return TA_ERR_ARG;
  return layernorm_dispatch<bf16_t, 1>((const bf16_t*)x_bf16, w, b, y_bf16, nullptr, nullptr, M, H, eps, st);
}

extern "C" int ta_layernorm_f32(const float* x, const float* w, const float* b, void* y_bf16, float* y_f32,
                                const float* rowscale, int M, int H, float eps, hipStream_t st) {
  return layernorm_dispatch(x, w, b, y_bf16, y_f32, rowscale, M, H, eps, st);
}

// the GELU form exists for f32 rows only (the projector's)
template <typename T>
static int rmsnorm_fwd_dispatch(const T* x, const float* w, void* y_bf16, float* y_f32, float* rstd, int M, int H, float eps, int act_gelu,
                                hipStream_t st) {
  if (M <= 0) return TA_OK;
  if (norm_bad_H(H)) return TA_ERR_ARG;
  bf16_t* yb = (bf16_t*)y_bf16;
  const dim3 blk(256);
  if (!act_gelu && y_bf16 && !y_f32 && half_wave_H(H)) {  // bf16 is the only output
    const dim3 g8(ta_cdiv(M, 8));
    with_nch(H, [&](auto nch) { TA_LAUNCH((rmsnorm_fwd_x8_kernel<T, decltype(nch)::value>), g8, blk, 0, st, x, w, yb, rstd, M, eps); });
    TA_CHECK_LAUNCH();
    return TA_OK;
  }
  constexpr bool IN_BF16 = std::is_same_v<T, bf16_t>;
  const dim3 grid(ta_cdiv(M, 4));
  const float* xf = (const float*)x;
  with_maxv(H, [&](auto maxv) {
    constexpr int V = decltype(maxv)::value;
    if constexpr (!IN_BF16)
      if (act_gelu) { TA_LAUNCH((rmsnorm_fwd_kernel<V, 1>), grid, blk, 0, st, xf, w, yb, y_f32, rstd, M, H, eps); return; }
    TA_LAUNCH((rmsnorm_fwd_kernel<V, 0, IN_BF16>), grid, blk, 0, st, xf, w, yb, y_f32, rstd, M, H, eps);
  });
  TA_CHECK_LAUNCH();
  return TA_OK;
}

extern "C" int ta_rmsnorm_fwd(const float* x, const float* w, void* y_bf16, float* y_f32, float* rstd,
                              int M, int H, float eps, int act_gelu, hipStream_t st) {
  return rmsnorm_fwd_dispatch(x, w, y_bf16, y_f32, rstd, M, H, eps, act_gelu, st);
}

// x read as bf16 (the LM's residual stream in the reference's model dtype)
extern "C" int ta_rmsnorm_fwd_bf16(const void* x_bf16, const float* w, void* y_bf16, float* y_f32, float* rstd, int M, int H,
                                   float eps, hipStream_t st) {
  return rmsnorm_fwd_dispatch((const bf16_t*)x_bf16, w, y_bf16, y_f32, rstd, M, H, eps, 0, st);
}

// The backward without GELU and without a weight gradient, for the dtypes the LM keeps x, the incoming gradient and the residual
// gradient in.  All three bf16 with H as half_wave_H wants it: the half-wave kernel.
template <bool X_BF16, bool DY_BF16, bool DRES_BF16>
static int rmsnorm_bwd_launch(const void* dy, const void* x, const float* rstd, const float* w, const void* dres, float* dx_f32, void* dx_bf16,
                              int M, int H, hipStream_t st) {
  if (M <= 0) return TA_OK;
  if (norm_bad_H(H)) return TA_ERR_ARG;
  const dim3 blk(256);
  if constexpr (X_BF16 && DY_BF16 && DRES_BF16) {
    if (half_wave_H(H)) {
      const dim3 g8(ta_cdiv(M, 8));
      with_nch(H, [&](auto nch) {
        TA_LAUNCH((rmsnorm_bwd_bf16x8_kernel<decltype(nch)::value>), g8, blk, 0, st, (const bf16_t*)dy, (const bf16_t*)x, rstd, w,
                  (const bf16_t*)dres, dx_f32, (bf16_t*)dx_bf16, M);
      });
      TA_CHECK_LAUNCH();
      return TA_OK;
    }
  }
  const dim3 grid(ta_cdiv(M, 4));
  with_maxv(H, [&](auto maxv) {
    TA_LAUNCH((rmsnorm_bwd_kernel<decltype(maxv)::value, 0, X_BF16, DY_BF16, DRES_BF16>), grid, blk, 0, st, (const float*)dy, (const float*)x,
              rstd, w, (const float*)dres, dx_f32, (bf16_t*)dx_bf16, (float*)nullptr, M, H);
  });
  TA_CHECK_LAUNCH();
  return TA_OK;
}

extern "C" int ta_rmsnorm_bwd_bf16(const void* dy, int dy_is_bf16, const void* x_bf16, const float* rstd, const float* w,
                                   const float* dres, float* dx_f32, void* dx_bf16, int M, int H, hipStream_t st) {
  return dy_is_bf16 ? rmsnorm_bwd_launch<true, true, false>(dy, x_bf16, rstd, w, dres, dx_f32, dx_bf16, M, H, st)
                    : rmsnorm_bwd_launch<true, false, false>(dy, x_bf16, rstd, w, dres, dx_f32, dx_bf16, M, H, st);
}

// the same with the residual gradient read as bf16 (dres_bf16 may alias dx_bf16: the bf16 d(x) stream updated in place)
extern "C" int ta_rmsnorm_bwd_bf16s(const void* dy, int dy_is_bf16, const void* x_bf16, const float* rstd, const float* w,
                                    const void* dres_bf16, float* dx_f32, void* dx_bf16, int M, int H, hipStream_t st) {
  return dy_is_bf16 ? rmsnorm_bwd_launch<true, true, true>(dy, x_bf16, rstd, w, dres_bf16, dx_f32, dx_bf16, M, H, st)
                    : rmsnorm_bwd_launch<true, false, true>(dy, x_bf16, rstd, w, dres_bf16, dx_f32, dx_bf16, M, H, st);
}

// fp32 residual stream, bf16 incoming gradient (ta_lm_backward in the fp32-stream mode -- under the recipe's bf16 autocast
// the gradient of a Linear's bf16 input IS a bf16 tensor, cast up afterwards, so nothing is lost by keeping its 2 bytes)
extern "C" int ta_rmsnorm_bwd_dyb(const void* dy_bf16, const float* x, const float* rstd, const float* w, const float* dres, float* dx_f32,
                         void* dx_bf16, int M, int H, hipStream_t st) {
  return rmsnorm_bwd_launch<false, true, false>(dy_bf16, x, rstd, w, dres, dx_f32, dx_bf16, M, H, st);
}

// rows of 4 per block; with a weight gradient at most 512 blocks (DWM = 2: each storing one slab of dw_ws)
static int rmsnorm_bwd_blocks(int M, bool dw) {
  const int blocks = ta_cdiv(M, 4);
  return dw && blocks > 512 ? 512 : blocks;
}
long ta_i_rmsnorm_bwd_ws_floats(int M, int H) { return M > 0 ? (long)rmsnorm_bwd_blocks(M, true) * H : 0; }

int ta_i_rmsnorm_bwd(const float* dy, const float* x, const float* rstd, const float* w, const float* dres, float* dx_f32,
                     void* dx_bf16, float* dw_accum, float* dw_ws, int M, int H, int act_gelu, hipStream_t st) {
  if (M <= 0) return TA_OK;
  if (norm_bad_H(H)) return TA_ERR_ARG;
  const int blocks = rmsnorm_bwd_blocks(M, dw_accum != nullptr);
  const size_t lds = dw_accum ? (size_t)H * 4 : 0;
  const bool slabs = dw_accum && dw_ws;                  // DWM = 2: the weight gradient goes to the workspace, folded below
  with_maxv(H, [&](auto maxv) {
    with_const<0, 1>(act_gelu ? 1 : 0, [&](auto act) {
      with_const<1, 2>(slabs ? 2 : 1, [&](auto dwm) {
        TA_LAUNCH((rmsnorm_bwd_kernel<decltype(maxv)::value, decltype(act)::value, false, false, false, decltype(dwm)::value>), dim3(blocks),
                  dim3(256), lds, st, dy, x, rstd, w, dres, dx_f32, (bf16_t*)dx_bf16, slabs ? dw_ws : dw_accum, M, H);
      });
    });
  });
  TA_CHECK_LAUNCH();
  if (slabs) {
    TA_LAUNCH(rmsnorm_dw_fold_kernel, dim3(ta_cdiv(H / 4, 16)), dim3(256), 0, st, (const float*)dw_ws, blocks, H, dw_accum);
    TA_CHECK_LAUNCH();
  }
  return TA_OK;
}

// The exported form has no workspace in its ABI: its weight gradient is accumulated with atomics (DWM = 1)
extern "C" int ta_rmsnorm_bwd(const float* dy, const float* x, const float* rstd, const float* w,
                              const float* dres, float* dx_f32, void* dx_bf16, float* dw_accum,
                              int M, int H, int act_gelu, hipStream_t st) {
  return ta_i_rmsnorm_bwd(dy, x, rstd, w, dres, dx_f32, dx_bf16, dw_accum, nullptr, M, H, act_gelu, st);
}


// ---------------------------------------------------------------------------- RMSNorm weight gradient (trainable LM)
// dw[h] += sum_m dy[m,h] * x[m,h] * rstd[m].  One workgroup = 32 rows x 256 columns: 4 row slots x 64 lanes of 4 columns,
// 8 rows per thread with the loads of a row pair in flight together; the 4 slots fold through LDS, one atomic per column.
template <bool DY_BF16, bool X_BF16>
__global__ __launch_bounds__(256) void rmsnorm_dw_kernel(const void* __restrict__ dy, const void* __restrict__ x,
                                                         const float* __restrict__ rstd, float* __restrict__ dw, int M, int H) {
  using DY = elem_t<DY_BF16>;
  using X = elem_t<X_BF16>;
  __shared__ float part[4][256];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = blockIdx.y * 256 + tx * 4, r0 = blockIdx.x * 32;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  auto ld4 = [](float4 u, float* o) { o[0] = u.x; o[1] = u.y; o[2] = u.z; o[3] = u.w; };
  if (c < H) {
#pragma unroll
    for (int i = 0; i < 8; i += 2) {
      const int ra = r0 + ty + 4 * i, rb = ra + 4;
      float g0[4], v0[4], g1[4], v1[4];
      const bool ia = ra < M, ib = rb < M;
      if (ia) { ld4(RowLoad<DY>::load4((const DY*)dy + ((long)ra * H + c), 0), g0); ld4(RowLoad<X>::load4((const X*)x + ((long)ra * H + c), 0), v0); }
      if (ib) { ld4(RowLoad<DY>::load4((const DY*)dy + ((long)rb * H + c), 0), g1); ld4(RowLoad<X>::load4((const X*)x + ((long)rb * H + c), 0), v1); }
      if (ia) { const float rs = rstd[ra]; for (int k = 0; k < 4; ++k) a[k] += g0[k] * v0[k] * rs; }
      if (ib) { const float rs = rstd[rb]; for (int k = 0; k < 4; ++k) a[k] += g1[k] * v1[k] * rs; }
    }
  }
  for (int k = 0; k < 4; ++k) part[ty][tx * 4 + k] = a[k];
  __syncthreads();
  const int cc = blockIdx.y * 256 + threadIdx.x;
  if (cc < H) unsafeAtomicAdd(dw + cc, part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x]);
}

extern "C" int ta_rmsnorm_dw(const void* dy, int dy_is_bf16, const void* x, int x_is_bf16, const float* rstd, float* dw_accum,
                             int M, int H, hipStream_t st) {
  if (M <= 0 || H <= 0) return TA_OK;
  if (H & 3) return TA_ERR_ARG;
  dim3 grid(ta_cdiv(M, 32), ta_cdiv(H, 256)), blk(256);
  if (dy_is_bf16 && x_is_bf16) TA_LAUNCH((rmsnorm_dw_kernel<true, true>), grid, blk, 0, st, dy, x, rstd, dw_accum, M, H);
  else if (dy_is_bf16) TA_LAUNCH((rmsnorm_dw_kernel<true, false>), grid, blk, 0, st, dy, x, rstd, dw_accum, M, H);
  else if (x_is_bf16) TA_LAUNCH((rmsnorm_dw_kernel<false, true>), grid, blk, 0, st, dy, x, rstd, dw_accum, M, H);
  else TA_LAUNCH((rmsnorm_dw_kernel<false, false>), grid, blk, 0, st, dy, x, rstd, dw_accum, M, H);
  TA_CHECK_LAUNCH();
  return TA_OK;
}
