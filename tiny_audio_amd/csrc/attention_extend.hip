// ta355 attention of T > 1 given tokens per row appended to an existing KV cache (candidate scoring), gfx950.
//
//   attn_extend_kernel<GRP>   causal GQA attention, head_dim 128, of R rows x T query positions.  The keys of row r come in two
//                             segments: the prompt slots of clip clip_of[r], read IN PLACE from one layer of the cache ta_lm_prefill
//                             filled (rows of one clip share them: a row only selects a base pointer), then the row's own slots
//                             j <= t, j < len[r], from the head-major K / V ta_lm_qkv_post_fwd writes.
//
// Prefill covers "q rows = k rows, no cache", the decode step "one q row against the cache"; this is the case between them.
// The tile is the one of attention.hip (attn_tile.h): S^T = K Q^T, online softmax in base 2 with the scale folded, the row sum as one
// extra MFMA block.  K and V are both staged as ROW tiles [64 slots][128] -- the cache is row-major [slot, 128] -- and the PV
// operand is read out of the V tile with the transposing LDS read, as the short-sequence forward does: no V^T image anywhere.
//
// One workgroup = 128 stacked query rows of one (row r, kv head): the GRP = Hq / Hkv query heads of the kv head times 128 / GRP
// positions, so a K / V tile is fetched once per kv head.  4 waves x 2 sub-tiles of 16 rows; sub-tile c = wave * 2 + sub holds head
// c % GRP, positions (c / GRP) * 16 .. + 15 of the workgroup's block.  Masked slots (pmask == 0, j >= len, j > t) hold finite
// garbage by contract: their scores are replaced by -inf before the softmax, so their P is exactly 0 and they add exactly nothing.
#include "common.h"
#include "attn_tile.h"
#include "../../include/ta355.h"

template <int GRP>
__global__ __launch_bounds__(256) void attn_extend_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ Kn,
                                                          const bf16_t* __restrict__ Vn, const bf16_t* __restrict__ Kc,
                                                          const bf16_t* __restrict__ Vc, const int* __restrict__ pmask,
                                                          const int* __restrict__ clip_of, const int* __restrict__ len,
                                                          bf16_t* __restrict__ O, float* __restrict__ LSE, int B, int Hq, int Hkv,
                                                          int T, int Lp, int Lmax, float scale) {
  constexpr int HD = 128, ND = HD / 16, QSUB = 2, TQ = 128 / GRP;
  __shared__ __attribute__((aligned(16))) char Ks[RowTile<HD>::BYTES];
  __shared__ __attribute__((aligned(16))) char Vs[RowTile<HD>::BYTES];
  __shared__ __attribute__((aligned(16))) int Ms[KV_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l15 = lane & 15;
  const int nqt = (T + TQ - 1) / TQ;
  const int qt = blockIdx.x % nqt, hk = (blockIdx.x / nqt) % Hkv, r = blockIdx.x / (nqt * Hkv);
  const int n = min(max(len[r], 0), T);                            // valid positions of this row
  const int clip = min(max(clip_of[r], 0), B - 1);
  const int tq0 = qt * TQ;
  int hsub[QSUB], tsub[QSUB];                                      // head and first position of each sub-tile
#pragma unroll
  for (int sub = 0; sub < QSUB; ++sub) {
    const int c = wave * QSUB + sub;
    hsub[sub] = hk * GRP + c % GRP;
    tsub[sub] = tq0 + (c / GRP) * 16;
  }
  auto store_row = [&](int sub, int t, const f32x4 (&o)[ND + 1], float inv, float lse) {
    bf16_t* orow = O + ((long)r * T + t) * ((long)Hq * HD) + (long)hsub[sub] * HD;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) {
      uint2 w;
      w.x = pack2bf(o[dt][0] * inv, o[dt][1] * inv);
      w.y = pack2bf(o[dt][2] * inv, o[dt][3] * inv);
      *(uint2*)(orow + dt * 16 + g * 4) = w;
    }
    if (LSE && g == 0) LSE[((long)r * Hq + hsub[sub]) * T + t] = lse;
  };
  f32x4 o[QSUB][ND + 1];
#pragma unroll
  for (int sub = 0; sub < QSUB; ++sub)
#pragma unroll
    for (int i = 0; i <= ND; ++i) o[sub][i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (tq0 >= n) {                                                  // the whole block lies behind the row's end: exact zeros (workgroup-uniform)
#pragma unroll
    for (int sub = 0; sub < QSUB; ++sub) {
      const int t = tsub[sub] + l15;
      if (t < T) store_row(sub, t, o[sub], 0.f, 1.0e30f);
    }
    return;
  }
  const bf16_t* Kp = Kc + ((long)clip * Hkv + hk) * Lmax * HD;     // prompt segment: this clip's cache rows, shared by its candidates
  const bf16_t* Vp = Vc + ((long)clip * Hkv + hk) * Lmax * HD;
  const bf16_t* Kr = Kn + ((long)r * Hkv + hk) * T * HD;           // candidate segment: the row's own K / V
  const bf16_t* Vr = Vn + ((long)r * Hkv + hk) * T * HD;
  const float sl2 = scale * LOG2E;

  bf16x8 qf[QSUB][HD / 32];
#pragma unroll
  for (int sub = 0; sub < QSUB; ++sub) {
    const int t = min(tsub[sub] + l15, T - 1);
    const bf16_t* qrow = Q + (((long)r * Hq + hsub[sub]) * T + t) * HD;
#pragma unroll
    for (int ks = 0; ks < HD / 32; ++ks) qf[sub][ks] = *(const bf16x8*)(qrow + ks * 32 + g * 8);
  }
  float m_run[QSUB];
#pragma unroll
  for (int sub = 0; sub < QSUB; ++sub) m_run[sub] = NEG_BIG;

  const int np = (Lp + KV_TILE - 1) / KV_TILE;                     // prompt tiles, then the candidate tiles up to the block's last valid query
  const int ntiles = np + (min(tq0 + TQ, n) + KV_TILE - 1) / KV_TILE;
  RowStage<HD> ks_reg, vs_reg; int mk_reg = 0;
  auto fetch = [&](int i) {                                        // tile i -> staging registers (keys clamped into their segment)
    if (i < np) {
      const int s0 = i * KV_TILE;
      ks_reg.load(Kp, HD, s0, Lp, tid);
      vs_reg.load(Vp, HD, s0, Lp, tid);
      if (tid < KV_TILE) mk_reg = (s0 + tid < Lp) ? pmask[(long)clip * Lp + s0 + tid] : 0;
    } else {
      const int j0 = (i - np) * KV_TILE;
      ks_reg.load(Kr, HD, j0, T, tid);
      vs_reg.load(Vr, HD, j0, T, tid);
      if (tid < KV_TILE) mk_reg = (j0 + tid < n) ? 1 : 0;
    }
  };
  const bf16x8 ones = (bf16x8){0x3f80, 0x3f80, 0x3f80, 0x3f80, 0x3f80, 0x3f80, 0x3f80, 0x3f80};
  const bf16x8 zeros = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
  const bf16x8 one_row = l15 == 0 ? ones : zeros;                  // row 0 of the extra block is all ones: it accumulates l = sum_k P[q, k]
  fetch(0);
  for (int i = 0; i < ntiles; ++i) {                               // workgroup-uniform: the transposing reads need every lane
    ks_reg.store(Ks, tid);
    vs_reg.store_tr(Vs, tid);
    if (tid < KV_TILE) Ms[tid] = mk_reg;
    __syncthreads();
    if (i + 1 < ntiles) fetch(i + 1);
    const bool cand = i >= np;
    const int j0 = cand ? (i - np) * KV_TILE : 0;
    f32x4 s[QSUB][4];
    qk_scores<HD, QSUB, false>(Ks, qf, s, l15, g);
#pragma unroll
    for (int sub = 0; sub < QSUB; ++sub) {
      const int t = tsub[sub] + l15;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        const int4 mk = *(const int4*)(Ms + kt * 16 + g * 4);
        const int mkv[4] = {mk.x, mk.y, mk.z, mk.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          bool v = mkv[e] != 0;
          if (cand) v = v & (j0 + kt * 16 + g * 4 + e <= t);        // causal over the row's own slots only: every prompt slot precedes them
          s[sub][kt][e] = v ? s[sub][kt][e] : -INFINITY;
        }
      }
      softmax_tile<ND>(s[sub], o[sub], m_run[sub], sl2);
    }
    pv_accumulate<ND, QSUB, false>(s, o, [&](int dt, int kp) {
      return dt < ND ? read_colfrag_tr<HD>(Vs, dt, l15, (2 * kp) * 16 + g * 4, (2 * kp + 1) * 16 + g * 4) : one_row;
    });
    __syncthreads();
  }
#pragma unroll
  for (int sub = 0; sub < QSUB; ++sub) {
    const int t = tsub[sub] + l15;
    const float l_run = __shfl(o[sub][ND][0], l15, 64);            // row 0 of the sum block lives in lane group g = 0
    if (t < T) {
      const bool live = t < n && l_run > 0.f;                      // behind the row's end, or no visible key at all: exact zeros
      store_row(sub, t, o[sub], live ? 1.0f / l_run : 0.f, live ? m_run[sub] * scale + __logf(l_run) : 1.0e30f);
    }
  }
}

extern "C" int ta_attention_extend(const void* Q, const void* Kn, const void* Vn, const void* Kc, const void* Vc, const int* pmask,
                                   const int* clip_of, const int* len, void* O, float* LSE, int B, int R, int Hq, int Hkv, int T,
                                   int Lp, int Lmax, float scale, hipStream_t st) {
  if (!Q || !Kn || !Vn || !Kc || !Vc || !pmask || !clip_of || !len || !O) return TA_ERR_ARG;
  if (B < 1 || R < 1 || R > TA_EXTEND_MAX_R || T < 1 || T > TA_EXTEND_MAX_T || Lp < 1 || Lp > Lmax || Hq < 1 || Hkv < 1 || Hq % Hkv)
    return TA_ERR_ARG;
  const int grp = Hq / Hkv;
  if (grp != 1 && grp != 2 && grp != 4) return TA_ERR_ARG;
  with_const<1, 2, 4>(grp, [&](auto G) {
    constexpr int GRP = decltype(G)::value, TQ = 128 / GRP;
    TA_LAUNCH(attn_extend_kernel<GRP>, dim3((unsigned)((T + TQ - 1) / TQ) * Hkv * R), dim3(256), 0, st, (const bf16_t*)Q,
              (const bf16_t*)Kn, (const bf16_t*)Vn, (const bf16_t*)Kc, (const bf16_t*)Vc, pmask, clip_of, len, (bf16_t*)O, LSE, B, Hq,
              Hkv, T, Lp, Lmax, scale);
  });
  TA_CHECK_LAUNCH();
  return TA_OK;
}
