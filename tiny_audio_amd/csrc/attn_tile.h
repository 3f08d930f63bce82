// The online-softmax tile the LM's forward attention kernels are built from (attention.hip, attention_extend.hip): the swizzled
// [64 rows][HD] LDS row tile and its staging, the transposing fragment read, and qk_scores / softmax_tile / pv_accumulate.
// Formulation and lane layout: the header comment of attention.hip.
#pragma once
#include "common.h"

#define KV_TILE 64
#define LOG2E 1.4426950408889634f
#define NEG_BIG (-1.0e30f)

// Row tiles are unpadded [64][HD] with the 16-B chunk index XOR-swizzled by the row: conflict-free ds_read_b128
// fragments under either lane grouping of the instruction (same scheme the GEMM uses; measured 0 conflicts there).
template <int HD> struct RowTile {
  static constexpr int STRIDE = HD * 2;
  static constexpr int BYTES = 64 * STRIDE;
  static __device__ __forceinline__ int swz(int r) { return HD == 64 ? ((r >> 1) & 7) : (r & 15); }
  // byte offset of 16-B chunk c of row r
  static __device__ __forceinline__ int off(int r, int c) { return r * STRIDE + ((c ^ swz(r)) << 4); }
  // Round 6: tiles that are ALSO read transposed (ds_read_b64_tr_b16: V in the forward; K, Q, dO in the backward) take this swizzle.
  // A transposed read's 32-lane group covers 8 consecutive rows x 32 B (chunks ca, ca ^ 1 of every row); under `r & 15` rows r and
  // r ^ 1 put (ca ^ r) and (ca ^ 1 ^ (r ^ 1)) in the SAME 16-B bank slot -- a 2-way conflict on every transposed read (PMC r05:
  // SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.27 in attn_bwd_kernel).  XOR by 2 * (r & 7) spreads the 16 (row, chunk) pairs over
  // all 16 slots, and the ds_read_b128 fragment pattern (16 rows x one chunk column per lane group) stays conflict-free under it:
  // rows {0-3, 12-15} at chunk c and rows {4-11} at chunk c + 1 land on the even and the odd slots.  (Same idea as attention_enc's vswz.)
  static __device__ __forceinline__ int swz_tr(int r) { return HD == 64 ? ((r >> 1) & 7) : ((r & 7) << 1); }
  static __device__ __forceinline__ int off_tr(int r, int c) { return r * STRIDE + ((c ^ swz_tr(r)) << 4); }
};

template <int HD>
struct RowStage {   // 64 rows x HD bf16, 256 threads
  static constexpr int N = HD / 32;   // 16-byte chunks per thread
  uint4 v[N];
  __device__ __forceinline__ void load(const bf16_t* base, long row_stride, int row0, int nrows_valid, int tid) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int ch = tid + i * 256;
      const int r = ch / (HD / 8), c = ch % (HD / 8);
      int gr = row0 + r; if (gr > nrows_valid - 1) gr = nrows_valid - 1; if (gr < 0) gr = 0;
      v[i] = *(const uint4*)(base + (long)gr * row_stride + c * 8);
    }
  }
  __device__ __forceinline__ void store(char* lds, int tid) const {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int ch = tid + i * 256;
      const int r = ch / (HD / 8), c = ch % (HD / 8);
      *(uint4*)(lds + RowTile<HD>::off(r, c)) = v[i];
    }
  }
  __device__ __forceinline__ void store_tr(char* lds, int tid) const {   // the image read_colfrag_tr reads
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int ch = tid + i * 256;
      const int r = ch / (HD / 8), c = ch % (HD / 8);
      *(uint4*)(lds + RowTile<HD>::off_tr(r, c)) = v[i];
    }
  }
};

__device__ __forceinline__ bf16x8 pack_p(const f32x4& a, const f32x4& b) {
  union { bf16x8 v; uint32_t u[4]; } r;
  r.u[0] = pack2bf(a[0], a[1]); r.u[1] = pack2bf(a[2], a[3]);
  r.u[2] = pack2bf(b[0], b[1]); r.u[3] = pack2bf(b[2], b[3]);
  return r.v;
}

// The fragment (row d = dt * 16 + l15 of the [d][64] image, columns [c0, c0+4) and [c1, c1+4)) read TRANSPOSED out of the
// ROW tile ([64 rows][HD], RowTile layout) with ds_read_b64_tr_b16 (gfx950): in each group of 16 lanes, lane L receives element
// (L & 3) of the 8-byte chunks addressed by lanes (L >> 2) + 4 j, j = 0..3.  Lane n of a group addresses (row c + (n >> 2),
// columns dt * 16 + 4 (n & 3) ..): lane L then holds rows c .. c+3 of column dt * 16 + L.  The backward kernels use it for the
// K^T / Q^T / dO^T operands, so the producers need not write (and the backward need not stage) transposed images.
typedef __attribute__((ext_vector_type(4))) short bf16x4_t;
template <int HD>
__device__ __forceinline__ bf16x8 read_colfrag_tr(const char* rowtile, int dt, int l15, int c0, int c1) {
  const int dcol = dt * 16 + 4 * (l15 & 3);                     // first of the 4 columns of this lane's 8-byte chunk
  const int chunk = dcol >> 3, half = (dcol >> 2) & 1;
  const int r0 = c0 + (l15 >> 2), r1 = c1 + (l15 >> 2);
  const bf16x4_t a = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) bf16x4_t*)(rowtile + RowTile<HD>::off_tr(r0, chunk) + half * 8));
  const bf16x4_t b = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) bf16x4_t*)(rowtile + RowTile<HD>::off_tr(r1, chunk) + half * 8));
  return (bf16x8){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// 3-input max: the compiler fuses the two maxnum calls into one v_max3_f32.  (An inline-asm v_max3_f32 here was WRONG: the
// hazard recognizer does not see inside asm, and once no other VALU work separated it from the QK^T MFMAs it read their
// accumulators before the matrix pipe had written them -- a stale, smaller row maximum, i.e. run-to-run 1-ulp noise.)
__device__ __forceinline__ float max3(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); }
__device__ __forceinline__ float group_max(float x) {
  auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  x = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
  auto q = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(q[0]), __uint_as_float(q[1]));
}

// ---- the online-softmax tile of one wave over 64 keys, in the three pieces every forward kernel is built from.  s[sub][kt] is S^T of
// key block kt (16 keys) for query sub-tile sub, o[sub][0 .. ND - 1] is O^T and o[sub][ND] the row-sum block.  What the kernels differ
// in stays with the caller: masking (between qk_scores and softmax_tile), where the V fragments come from, the epilogue -- and FENCE,
// the scheduling fences of the resident kernel, which keep the fragments of one block live at a time (VGPR budget).
// S^T = K Q^T for every query sub-tile: each K fragment read from the row tile feeds QSUB MFMAs
template <int HD, int QSUB, bool FENCE>
__device__ __forceinline__ void qk_scores(const char* Kt, const bf16x8 (&qf)[QSUB][HD / 32], f32x4 (&s)[QSUB][4], int l15, int g) {
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
    for (int sub = 0; sub < QSUB; ++sub) s[sub][kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < HD / 32; ++ks) {
      const bf16x8 a = *(const bf16x8*)(Kt + RowTile<HD>::off(kt * 16 + l15, ks * 4 + g));
#pragma unroll
      for (int sub = 0; sub < QSUB; ++sub)
        s[sub][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, qf[sub][ks], s[sub][kt], 0, 0, 0);
    }
    if (FENCE) __builtin_amdgcn_sched_barrier(0);
  }
}
// online softmax numerators of one sub-tile, masked scores already -inf (the denominator rides in the MFMA of pv_accumulate)
template <int ND>
__device__ __forceinline__ void softmax_tile(f32x4 (&s)[4], f32x4 (&o)[ND + 1], float& m_run, float sl2) {
  float mloc = max3(s[0][0], s[0][1], s[0][2]);
  mloc = max3(mloc, s[0][3], s[1][0]);
  mloc = max3(mloc, s[1][1], s[1][2]);
  mloc = max3(mloc, s[1][3], s[2][0]);
  mloc = max3(mloc, s[2][1], s[2][2]);
  mloc = max3(mloc, s[2][3], s[3][0]);
  mloc = max3(mloc, s[3][1], s[3][2]);
  mloc = fmaxf(mloc, s[3][3]);
  const float m_new = fmaxf(m_run, group_max(mloc));
  if (__any(m_new != m_run)) {                       // rescale only when some row's running max moved
    const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * sl2);
#pragma unroll
    for (int i = 0; i <= ND; ++i) { o[i][0] *= alpha; o[i][1] *= alpha; o[i][2] *= alpha; o[i][3] *= alpha; }
    m_run = m_new;
  }
  const float mb = m_new * sl2;
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int r = 0; r < 4; ++r) s[kt][r] = __builtin_amdgcn_exp2f(fmaf(s[kt][r], sl2, -mb));
}
// [O^T ; l] += [V^T ; 1] P^T.  vfrag(dt, kp) = the A fragment of row block dt (ND: the block whose first row is all ones) over the
// keys of block pair kp, i.e. columns [c, c + 4) for c = (2 kp) * 16 + g * 4 and (2 kp + 1) * 16 + g * 4
template <int ND, int QSUB, bool FENCE, typename VF>
__device__ __forceinline__ void pv_accumulate(const f32x4 (&s)[QSUB][4], f32x4 (&o)[QSUB][ND + 1], VF&& vfrag) {
#pragma unroll
  for (int kp = 0; kp < 2; ++kp) {
    bf16x8 pb[QSUB];
#pragma unroll
    for (int sub = 0; sub < QSUB; ++sub) pb[sub] = pack_p(s[sub][2 * kp], s[sub][2 * kp + 1]);
#pragma unroll
    for (int dt = 0; dt <= ND; ++dt) {
      const bf16x8 va = vfrag(dt, kp);
#pragma unroll
      for (int sub = 0; sub < QSUB; ++sub)
        o[sub][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, pb[sub], o[sub][dt], 0, 0, 0);
      if (FENCE && (dt & 1)) __builtin_amdgcn_sched_barrier(0);
    }
  }
}
