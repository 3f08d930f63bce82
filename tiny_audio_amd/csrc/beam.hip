// ta355 beam search: HF GenerationMixin._beam_search (TF:generation/utils.py, do_sample=False) around the unchanged decode step.
//
// Beams are ROWS: R = B * K rows, row = b * K + k, go through ta_lm_decode_step and the logits processors exactly as R greedy clips
// would.  This file holds what a beam step adds behind them (in launch order):
//   ta_beam_logprobs_f32   log_softmax of the step's f32 logits rows, in place (HF scores log-probabilities, not logits)
//   ta_beam_topk_f32       _get_top_k_continuations: per clip the M = max(2, 1 + n_eos) * K largest of row[k][v] + running_score[k]
//   ta_beam_advance        _get_running_beams_for_next_iteration, _update_finished_beams, _check_early_stop_heuristic,
//                          _beam_search_has_unfinished_sequences, and the greedy loop's bookkeeping (step, slot, pos, key mask)
//   ta_kv_beam_reorder     the cache reorder (DynamicCache.reorder_cache): generated slots of a clip's K rows permuted by `parent`
// and, once before the loop, ta_kv_beam_expand (the prompt's cache rows of clip b copied to its K rows).
// Every launch takes step-invariant arguments (the step, the slot and all flags live in device memory), so the step is captured
// into a hipGraph as the greedy step is.  The state machine is f32 adds, compares, IEEE divides and selects in HF's order: given
// the same candidates, state and output equal HF's bit for bit (tests/beam_ref.py restates it in numpy).
#include <climits>
#include "host_util.h"
#include "internal.h"

namespace {
#define BM_MAXK 8
#define BM_MAXM 32
#define BM_MAXEOS 3
#define BM_SPLIT 8                 // workgroups per row in the wide-row layouts (as TS_SPLIT of generate.hip)
#define BM_SPLIT_MAX_ROWS 64
#define BM_SPLIT_MIN_V 16384
__device__ float g_bl_ms[BM_SPLIT_MAX_ROWS * BM_SPLIT * 2];        // (m, s) per (row, slice): ta_beam_logprobs_f32's own scratch

__device__ __forceinline__ void ms_merge(float& m, float& s, float m2, float s2) {
  if (m2 == -INFINITY) return;
  if (m == -INFINITY) { m = m2; s = s2; return; }
  if (m2 > m) { const float a = m, c = s; m = m2; s = s2; m2 = a; s2 = c; }
  s += s2 * __expf(m2 - m);
}
__device__ __forceinline__ bool cand_before(float v, int i, float ov, int oi) { return v > ov || (v == ov && i < oi); }

// ---- log_softmax.  Direct: one workgroup per row reduces (m, s = sum e^(x - m)) in one pass and rewrites the row.  Split (few wide
// rows): BM_SPLIT workgroups per row leave their slice's (m, s) in g_bl_ms; beam_logprobs_apply_kernel merges the BM_SPLIT pairs in
// slice order (every workgroup of the row forms the same float) and rewrites its slice.
template <bool SPLIT>
__global__ __launch_bounds__(1024) void beam_logprobs_kernel(float* __restrict__ x, long ld, int V) {
  __shared__ float rm[16], rs[16];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int chunk = SPLIT ? ((V + BM_SPLIT - 1) / BM_SPLIT + 3) & ~3 : V;
  const int j0 = SPLIT ? min(V, (int)blockIdx.y * chunk) : 0, j1 = SPLIT ? min(V, j0 + chunk) : V;
  float* row = x + (long)r * ld;
  float m = -INFINITY, s = 0.f;
  auto take = [&](float v) {
    if (v > m) { s = m == -INFINITY ? 1.f : s * __expf(m - v) + 1.f; m = v; }
    else if (v > -INFINITY) s += __expf(v - m);
  };
  const bool vec = (((size_t)row) & 15) == 0;
  const int n4 = vec ? (j1 - j0) / 4 : 0;
  const float4* row4 = (const float4*)(row + j0);
  for (int q = tid; q < n4; q += 1024) { const float4 v = row4[q]; take(v.x); take(v.y); take(v.z); take(v.w); }
  for (int j = j0 + n4 * 4 + tid; j < j1; j += 1024) take(row[j]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ms_merge(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
  if (lane == 0) { rm[wave] = m; rs[wave] = s; }
  __syncthreads();
  m = rm[0]; s = rs[0];
  for (int w = 1; w < 16; ++w) ms_merge(m, s, rm[w], rs[w]);       // the same order in every lane
  if constexpr (SPLIT) {
    if (tid == 0) { const int p = (r * BM_SPLIT + (int)blockIdx.y) * 2; g_bl_ms[p] = m; g_bl_ms[p + 1] = s; }
  } else {
    if (m == -INFINITY) return;                                    // no finite entry: the row stays as it is
    const float ls = logf(s);
    float4* w4 = (float4*)row;
    for (int q = tid; q < n4; q += 1024) {
      float4 v = w4[q];
      v.x = (v.x - m) - ls; v.y = (v.y - m) - ls; v.z = (v.z - m) - ls; v.w = (v.w - m) - ls;
      w4[q] = v;
    }
    for (int j = n4 * 4 + tid; j < V; j += 1024) row[j] = (row[j] - m) - ls;
  }
}
__global__ __launch_bounds__(1024) void beam_logprobs_apply_kernel(float* __restrict__ x, long ld, int V) {
  const int r = blockIdx.x, tid = threadIdx.x;
  const int chunk = ((V + BM_SPLIT - 1) / BM_SPLIT + 3) & ~3;
  const int j0 = min(V, (int)blockIdx.y * chunk), j1 = min(V, j0 + chunk);
  float m = -INFINITY, s = 0.f;
  for (int p = 0; p < BM_SPLIT; ++p) ms_merge(m, s, g_bl_ms[(r * BM_SPLIT + p) * 2], g_bl_ms[(r * BM_SPLIT + p) * 2 + 1]);
  if (m == -INFINITY) return;
  const float ls = logf(s);
  float* row = x + (long)r * ld;
  const bool vec = (((size_t)row) & 15) == 0;
  const int n4 = vec ? (j1 - j0) / 4 : 0;
  float4* w4 = (float4*)(row + j0);
  for (int q = tid; q < n4; q += 1024) {
    float4 v = w4[q];
    v.x = (v.x - m) - ls; v.y = (v.y - m) - ls; v.z = (v.z - m) - ls; v.w = (v.w - m) - ls;
    w4[q] = v;
  }
  for (int j = j0 + n4 * 4 + tid; j < j1; j += 1024) row[j] = (row[j] - m) - ls;
}

// ---- top M of a clip's K * V accumulated values.  One workgroup per (slice, beam, clip): a lane keeps the CAP >= M best of the
// elements it meets as a sorted list in registers (the pattern of token_scores_kernel; a lane meets its indices in increasing order,
// so equal values keep the lower index in front), each wave pops its M best with shuffles ("wave argmax over the list heads, the
// owner pops"), the 16 wave lists meet in LDS and every entry finds its rank there.  The slice's M best go to the workspace;
// beam_topk_combine_kernel ranks the K * slices lists of a clip.  Order everywhere: larger value first, lower flat index on ties --
// -inf included, so rows with fewer than M finite entries are completed by their lowest -inf indices, as a stable sort would.
template <int CAP>
__global__ __launch_bounds__(1024) void beam_topk_kernel(const float* __restrict__ x, long ld, int V, const float* __restrict__ score,
                                                         int K, int M, int SV, float* __restrict__ part_v, int* __restrict__ part_i) {
  __shared__ float wv[16 * BM_MAXM];
  __shared__ int wi[16 * BM_MAXM];
  const int sl = blockIdx.x, k = blockIdx.y, b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int chunk = SV > 1 ? ((V + SV - 1) / SV + 3) & ~3 : V;
  const int j0 = min(V, sl * chunk), j1 = min(V, j0 + chunk);
  const float* row = x + ((long)b * K + k) * ld;
  const float sc = score[b * K + k];
  const int f0 = k * V;
  float tv[CAP]; int ti[CAP];
#pragma unroll
  for (int p = 0; p < CAP; ++p) { tv[p] = -INFINITY; ti[p] = INT_MAX; }
  auto take = [&](float v, int j) {
    const float a = v + sc;                                        // HF: log_probs + running_beam_scores[:, :, None], one f32 add
    const int f = f0 + j;
    if (cand_before(a, f, tv[CAP - 1], ti[CAP - 1])) {
      tv[CAP - 1] = a; ti[CAP - 1] = f;
#pragma unroll
      for (int p = CAP - 1; p > 0; --p)
        if (cand_before(tv[p], ti[p], tv[p - 1], ti[p - 1])) {
          const float t0 = tv[p]; tv[p] = tv[p - 1]; tv[p - 1] = t0;
          const int c0 = ti[p]; ti[p] = ti[p - 1]; ti[p - 1] = c0;
        }
    }
  };
  const bool vec = (((size_t)row) & 15) == 0;
  const int n4 = vec ? (j1 - j0) / 4 : 0;
  const float4* row4 = (const float4*)(row + j0);
  for (int q0 = tid; q0 < n4; q0 += 4 * 1024) {                    // four 16-byte loads in flight per lane
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = q0 + u * 1024;
      v[u] = q < n4 ? row4[q] : make_float4(NAN, NAN, NAN, NAN);   // (NaN never enters a list)
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + 4 * (q0 + u * 1024);
      take(v[u].x, j); take(v[u].y, j + 1); take(v[u].z, j + 2); take(v[u].w, j + 3);
    }
  }
  for (int j = j0 + n4 * 4 + tid; j < j1; j += 1024) take(row[j], j);
  for (int r = 0; r < M; ++r) {                                    // the wave's M best, in order
    float hv = tv[0]; int hi = ti[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(hv, o, 64); const int oi = __shfl_xor(hi, o, 64);
      if (cand_before(ov, oi, hv, hi)) { hv = ov; hi = oi; }
    }
    if (hi != INT_MAX && ti[0] == hi) {                            // the owner (flat indices are unique): drop the head
#pragma unroll
      for (int p = 0; p + 1 < CAP; ++p) { tv[p] = tv[p + 1]; ti[p] = ti[p + 1]; }
      tv[CAP - 1] = -INFINITY; ti[CAP - 1] = INT_MAX;
    }
    if (lane == 0) { wv[wave * M + r] = hv; wi[wave * M + r] = hi; }
  }
  __syncthreads();
  const int n = 16 * M;                                            // <= 512: one entry per lane
  if (tid < n) {
    const float v = wv[tid]; const int i = wi[tid];
    int rank = 0;
    for (int q = 0; q < n; ++q) rank += (cand_before(wv[q], wi[q], v, i) || (wv[q] == v && wi[q] == i && q < tid)) ? 1 : 0;
    if (rank < M) {                                                // (empty entries are all alike: their place in the list orders them)
      const long o = ((((long)b * K + k) * SV + sl) * M) + rank;
      part_v[o] = v; part_i[o] = i;
    }
  }
}
__global__ __launch_bounds__(1024) void beam_topk_combine_kernel(const float* __restrict__ part_v, const int* __restrict__ part_i, int n,
                                                                 int M, float* __restrict__ cand_score, int* __restrict__ cand_flat) {
  __shared__ float sv[BM_MAXK * BM_SPLIT * BM_MAXM];
  __shared__ int si[BM_MAXK * BM_SPLIT * BM_MAXM];
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int c = tid; c < n; c += 1024) { sv[c] = part_v[(long)b * n + c]; si[c] = part_i[(long)b * n + c]; }
  __syncthreads();
  for (int c = tid; c < n; c += 1024) {
    const float v = sv[c]; const int i = si[c];
    int rank = 0;
    for (int q = 0; q < n; ++q) rank += (cand_before(sv[q], si[q], v, i) || (sv[q] == v && si[q] == i && q < c)) ? 1 : 0;
    if (rank < M) { cand_score[(long)b * M + rank] = v; cand_flat[(long)b * M + rank] = i == INT_MAX ? -1 : i; }
  }
}

// ---- the beam bookkeeping of one step, one workgroup per clip.
struct BeamAdv {
  const float* cand_score; const int* cand_flat; int K, M, V;
  const long* eos; int n_eos; long pad_id; int max_new; const float* len_div; int early_stopping, heur_max_len;
  long* run_seq; float* run_score; int* parent; long* next_ids;
  long* pool_seq; float* pool_score; int* pool_len; int* pool_fin; int* heur; int* clip_done;
  const int* step_p; const int* slot_p; int* pos; int* kmask; int Lmax;
  float* tr_cand_score; int* tr_cand_flat; long* tr_run_seq; float* tr_run_score; int* tr_parent; int B;
};
__global__ __launch_bounds__(256) void beam_advance_kernel(const BeamAdv a) {
  extern __shared__ __attribute__((aligned(16))) int seq_s[];      // [K, max_new]: the running sequences as they stood before the step
  __shared__ float cs[BM_MAXM];
  __shared__ int par[BM_MAXM], tok[BM_MAXM], hit[BM_MAXM];
  __shared__ int run_src[BM_MAXK], pool_src[BM_MAXK], new_pl[BM_MAXK], new_pf[BM_MAXK];
  __shared__ float new_rs[BM_MAXK], new_ps[BM_MAXK], ms[BM_MAXK + BM_MAXM];
  __shared__ int used[BM_MAXK + BM_MAXM];
  const int b = blockIdx.x, tid = threadIdx.x, K = a.K, M = a.M, max_new = a.max_new;
  const int t = *a.step_p, slot = *a.slot_p;
  if (t < 0 || t >= max_new) return;                               // (the loop never launches past max_new)
  const int R = a.B * K;
  for (int k = 0; k < K; ++k) {
    const long* src = a.run_seq + ((long)b * K + k) * max_new;
    for (int i = tid; i < t; i += 256) {
      const long v = src[i];
      seq_s[k * max_new + i] = (int)v;
      if (a.tr_run_seq) a.tr_run_seq[(((long)t * R) + b * K + k) * max_new + i] = v;
    }
  }
  if (tid < K && a.tr_run_score) a.tr_run_score[(long)t * R + b * K + tid] = a.run_score[b * K + tid];
  if (tid < M) {
    const float v = a.cand_score[(long)b * M + tid];
    int f = a.cand_flat[(long)b * M + tid];
    if (a.tr_cand_score) { a.tr_cand_score[((long)t * a.B + b) * M + tid] = v; a.tr_cand_flat[((long)t * a.B + b) * M + tid] = f; }
    if (f < 0 || f / a.V >= K) f = 0;                              // (only a row of NaNs leaves an empty candidate)
    const int tk = f % a.V;
    bool h = t + 1 == max_new;                                     // HF MaxLengthCriteria
    for (int e = 0; e < a.n_eos; ++e) h |= (long)tk == a.eos[e];   // HF EosTokenCriteria
    cs[tid] = v; par[tid] = f / a.V; tok[tid] = tk; hit[tid] = h ? 1 : 0;
  }
  __syncthreads();
  if (tid == 0) {
#pragma clang fp contract(off)                                      // HF's separate multiply and add kernels: never one fma
    // _get_running_beams_for_next_iteration: the K best of cand + hit * -1e9
    for (int c = 0; c < M; ++c) { ms[c] = cs[c] + (hit[c] ? 1.0f : 0.0f) * -1.0e9f; used[c] = 0; }
    for (int i = 0; i < K; ++i) {
      int best = -1;
      for (int c = 0; c < M; ++c)
        if (!used[c] && (best < 0 || ms[c] > ms[best])) best = c;
      used[best] = 1; run_src[i] = best; new_rs[i] = ms[best];
    }
    // _update_finished_beams: length penalty, the three maskings in HF's order, merge with the pool, keep the K best
    const float div = a.len_div[t];
    bool full = true;
    for (int j = 0; j < K; ++j) full &= a.pool_fin[b * K + j] != 0;
    const bool heur_old = a.heur[b] != 0;
    const float m_full = (full && a.early_stopping == 1) ? 1.0f : 0.0f, m_heur = heur_old ? 0.0f : 1.0f;
    for (int j = 0; j < K; ++j) { ms[j] = a.pool_score[b * K + j]; used[j] = 0; }
    bool allhit = true;
    for (int c = 0; c < M; ++c) {
      const bool did = hit[c] && c < K;                            // only the first K candidates may finish
      float f = cs[c] / div;
      f = f + m_full * -1.0e9f;
      f = f + m_heur * -1.0e9f;
      f = f + (did ? 0.0f : 1.0f) * -1.0e9f;
      ms[K + c] = f; used[K + c] = 0;
      allhit &= hit[c] != 0;
    }
    bool allfin = true;
    float mn = INFINITY;
    for (int j = 0; j < K; ++j) {
      int best = -1;
      for (int c = 0; c < K + M; ++c)
        if (!used[c] && (best < 0 || ms[c] > ms[best])) best = c;
      used[best] = 1; pool_src[j] = best; new_ps[j] = ms[best];
      if (best < K) { new_pl[j] = a.pool_len[b * K + best]; new_pf[j] = a.pool_fin[b * K + best]; }
      else { new_pl[j] = t + 1; new_pf[j] = (hit[best - K] && best - K < K) ? 1 : 0; }
      allfin &= new_pf[j] != 0;
      mn = fminf(mn, ms[best]);
    }
    // _check_early_stop_heuristic (cur_len already advanced) and _beam_search_has_unfinished_sequences, for this clip
    const float hd = a.heur_max_len ? a.len_div[max_new - 1] : a.len_div[t];
    const float best_run = new_rs[0] / hd;
    bool any = false;
    for (int j = 0; j < K; ++j) any |= best_run > (new_pf[j] ? mn : -1.0e9f);
    const bool heur_new = heur_old && any;
    const bool cont = heur_new && !(allfin && a.early_stopping == 1) && !allhit;
    a.heur[b] = heur_new ? 1 : 0;
    a.clip_done[b] = (a.clip_done[b] != 0 || !cont) ? 1 : 0;
  }
  __syncthreads();
  // the pool, slot K-1 down to 0: a pool entry only ever moves to a higher slot (both orders are stable), so the row a slot reads
  // has not been overwritten yet; a new entry comes from the staged running sequences
  for (int j = K - 1; j >= 0; --j) {
    const int src = pool_src[j];
    long* dst = a.pool_seq + ((long)b * K + j) * max_new;
    if (src < K) {
      if (src != j) {
        const long* from = a.pool_seq + ((long)b * K + src) * max_new;
        for (int i = tid; i < max_new; i += 256) dst[i] = from[i];
      }
    } else {
      const int c = src - K, p = par[c];
      for (int i = tid; i < max_new; i += 256) dst[i] = i < t ? (long)seq_s[p * max_new + i] : (i == t ? (long)tok[c] : a.pad_id);
    }
    __syncthreads();
  }
  for (int i0 = 0; i0 < K; ++i0) {                                  // the running sequences, permuted through the LDS copy
    const int c = run_src[i0], p = par[c];
    long* dst = a.run_seq + ((long)b * K + i0) * max_new;
    if (p != i0)
      for (int i = tid; i < t; i += 256) dst[i] = (long)seq_s[p * max_new + i];
    if (tid == 0) dst[t] = (long)tok[c];
  }
  if (tid < K) {
    const int r = b * K + tid, c = run_src[tid];
    a.run_score[r] = new_rs[tid];
    a.parent[r] = par[c];
    a.next_ids[r] = (long)tok[c];
    if (a.tr_parent) a.tr_parent[(long)t * R + r] = par[c];
    a.pool_score[r] = new_ps[tid]; a.pool_len[r] = new_pl[tid]; a.pool_fin[r] = new_pf[tid];
    // as greedy_advance_kernel: the token just chosen is the next step's input, at position pos[r] in cache slot ns
    if (t > 0) a.pos[r] += 1;
    const int ns = t > 0 ? slot + 1 : slot;
    if (ns < a.Lmax) a.kmask[(long)r * a.Lmax + ns] = 1;
  }
}
// after every clip's workgroup has read them: advance the step and the slot, count the clips that are not done
__global__ __launch_bounds__(64) void beam_tick_kernel(const int* __restrict__ clip_done, int B, int max_new, int* __restrict__ step_p,
                                                       int* __restrict__ slot_p, int* __restrict__ n_unfinished) {
  const int t = *step_p, slot = *slot_p;
  if (t < 0 || t >= max_new) return;
  int alive = 0;
  for (int b = threadIdx.x; b < B; b += 64) alive += clip_done[b] ? 0 : 1;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) alive += __shfl_xor(alive, o, 64);
  if (threadIdx.x == 0) { *step_p = t + 1; *slot_p = t > 0 ? slot + 1 : slot; *n_unfinished = alive; }
}

// ---- the cache.  Both kernels move 16-byte pieces with vector loads and stores; a piece is (cache, layer, kv head, slot, 8 dims).
__global__ __launch_bounds__(256) void kv_beam_expand_kernel(const uint4* __restrict__ ksrc, const uint4* __restrict__ vsrc,
                                                             uint4* __restrict__ kdst, uint4* __restrict__ vdst, int layers, int B, int K,
                                                             int Hkv, int L, int Lsrc, int Lmax, int D8) {
  const long total = (long)layers * B * K * Hkv * L * D8;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int d = (int)(idx % D8);
  long q = idx / D8;
  const int s = (int)(q % L); q /= L;
  const int h = (int)(q % Hkv); q /= Hkv;
  const int r = (int)(q % ((long)B * K));
  const int l = (int)(q / ((long)B * K));
  const long from = ((((long)l * B + r / K) * Hkv + h) * Lsrc + s) * D8 + d;
  const long to = ((((long)l * B * K + r) * Hkv + h) * Lmax + s) * D8 + d;
  if (blockIdx.y == 0) kdst[to] = ksrc[from];
  else vdst[to] = vsrc[from];
}
// A lane owns one piece of one clip: it loads the piece from all K rows into registers, then stores to row j the piece of row
// parent[j].  No two lanes touch the same bytes, so the permutation needs no scratch copy and no ordering between workgroups.
template <int K>
__global__ __launch_bounds__(256) void kv_beam_reorder_kernel(uint4* __restrict__ kc, uint4* __restrict__ vc, int layers, int B, int Hkv,
                                                              int L, int Lmax, int D8, const int* __restrict__ parent,
                                                              const int* __restrict__ slot_p) {
  const int s = L + (int)blockIdx.y, b = blockIdx.z;
  if (s >= *slot_p || s >= Lmax) return;
  int pj[K];
  bool ident = true;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    int p = parent[b * K + j];
    if (p < 0 || p >= K) p = j;
    pj[j] = p; ident &= p == j;
  }
  if (ident) return;
  const int per = layers * Hkv * D8;                                // pieces of one (cache, clip row, slot)
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= 2 * per) return;
  uint4* base = idx < per ? kc : vc;
  int q = idx < per ? idx : idx - per;
  const int d = q % D8; q /= D8;
  const int h = q % Hkv;
  const int l = q / Hkv;
  const long row_stride = (long)Hkv * Lmax * D8;
  uint4* p0 = base + ((((long)l * B * K + (long)b * K) * Hkv + h) * Lmax + s) * D8 + d;
  uint4 v[K];
#pragma unroll
  for (int j = 0; j < K; ++j) v[j] = p0[j * row_stride];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    uint4 w = v[0];
#pragma unroll
    for (int q2 = 1; q2 < K; ++q2)
      if (pj[j] == q2) w = v[q2];                                   // compares, not a dynamically indexed array: nothing spills
    if (pj[j] != j) p0[j * row_stride] = w;
  }
}
}  // namespace

static bool beam_shape_ok(int K, int M, int n_eos) { return K >= 1 && K <= BM_MAXK && M >= 1 && M <= BM_MAXM && n_eos >= 0 && n_eos <= BM_MAXEOS; }
static int beam_slices(int R, int V) { return (R <= BM_SPLIT_MAX_ROWS && V >= BM_SPLIT_MIN_V) ? BM_SPLIT : 1; }

extern "C" int ta_beam_logprobs_f32(float* logits, long ld, int V, int R, hipStream_t st) {
  if (R <= 0) return TA_OK;
  if (!logits || V <= 0 || ld < V) return TA_ERR_ARG;
  if (beam_slices(R, V) > 1) {
    TA_LAUNCH((beam_logprobs_kernel<true>), dim3(R, BM_SPLIT), dim3(1024), 0, st, logits, ld, V);
    TA_CHECK_LAUNCH();
    TA_LAUNCH(beam_logprobs_apply_kernel, dim3(R, BM_SPLIT), dim3(1024), 0, st, logits, ld, V);
  } else {
    TA_LAUNCH((beam_logprobs_kernel<false>), dim3(R), dim3(1024), 0, st, logits, ld, V);
  }
  TA_CHECK_LAUNCH();
  return TA_OK;
}

extern "C" long ta_beam_topk_workspace_bytes(int B, int K, int V, int M) {
  if (B <= 0 || K <= 0 || M <= 0) return 0;
  return (long)B * K * beam_slices(B * K, V) * M * 8;
}
extern "C" int ta_beam_topk_f32(const float* rows, long ld, int V, const float* score, int B, int K, int M, float* cand_score,
                                int* cand_flat, void* ws, long ws_bytes, hipStream_t st) {
  if (!beam_shape_ok(K, M, 0) || M > (long)K * V) return TA_ERR_ARG;
  if (B <= 0) return TA_OK;
  if (!rows || V <= 0 || ld < V || (long)K * V >= INT_MAX || !score || !cand_score || !cand_flat || !ws ||
      ws_bytes < ta_beam_topk_workspace_bytes(B, K, V, M))
    return TA_ERR_ARG;
  const int SV = beam_slices(B * K, V);
  float* part_v = (float*)ws;
  int* part_i = (int*)(part_v + (long)B * K * SV * M);
#define BT(C_) TA_LAUNCH((beam_topk_kernel<C_>), dim3(SV, K, B), dim3(1024), 0, st, rows, ld, V, score, K, M, SV, part_v, part_i)
  if (M <= 4) BT(4);
  else if (M <= 8) BT(8);
  else if (M <= 16) BT(16);
  else BT(32);
#undef BT
  TA_CHECK_LAUNCH();
  TA_LAUNCH(beam_topk_combine_kernel, dim3(B), dim3(1024), 0, st, part_v, part_i, K * SV * M, M, cand_score, cand_flat);
  TA_CHECK_LAUNCH();
  return TA_OK;
}

extern "C" int ta_beam_advance(const float* cand_score, const int* cand_flat, int B, int K, int M, int V, const long* eos_ids, int n_eos,
                               long pad_id, int max_new, const float* len_div, int early_stopping, int heur_max_len, long* run_seq,
                               float* run_score, int* parent, long* next_ids, long* pool_seq, float* pool_score, int* pool_len,
                               int* pool_fin, int* heur, int* clip_done, int* step_dev, int* slot_dev, int* pos, int* kmask, int Lmax,
                               int* n_unfinished, float* tr_cand_score, int* tr_cand_flat, long* tr_run_seq, float* tr_run_score,
                               int* tr_parent, hipStream_t st) {
  if (!beam_shape_ok(K, M, n_eos) || M < K) return TA_ERR_ARG;
  if (B <= 0) return TA_OK;
  const size_t smem = (size_t)K * (max_new > 0 ? max_new : 0) * sizeof(int);
  const bool trace = tr_cand_score || tr_cand_flat || tr_run_seq || tr_run_score || tr_parent;
  if (!cand_score || !cand_flat || V <= 0 || (n_eos > 0 && !eos_ids) || max_new <= 0 || smem > 48 * 1024 || !len_div ||
      early_stopping < 0 || early_stopping > 2 || !run_seq || !run_score || !parent || !next_ids || !pool_seq || !pool_score ||
      !pool_len || !pool_fin || !heur || !clip_done || !step_dev || !slot_dev || !pos || !kmask || Lmax <= 0 || !n_unfinished ||
      (trace && !(tr_cand_score && tr_cand_flat && tr_run_seq && tr_run_score && tr_parent)))
    return TA_ERR_ARG;
  const BeamAdv a = {cand_score, cand_flat, K, M, V, eos_ids, n_eos, pad_id, max_new, len_div, early_stopping, heur_max_len ? 1 : 0,
                     run_seq, run_score, parent, next_ids, pool_seq, pool_score, pool_len, pool_fin, heur, clip_done,
                     step_dev, slot_dev, pos, kmask, Lmax, tr_cand_score, tr_cand_flat, tr_run_seq, tr_run_score, tr_parent, B};
  TA_LAUNCH(beam_advance_kernel, dim3(B), dim3(256), smem, st, a);
  TA_CHECK_LAUNCH();
  TA_LAUNCH(beam_tick_kernel, dim3(1), dim3(64), 0, st, clip_done, B, max_new, step_dev, slot_dev, n_unfinished);
  TA_CHECK_LAUNCH();
  return TA_OK;
}

extern "C" int ta_kv_beam_expand(const void* ksrc, const void* vsrc, void* kdst, void* vdst, int layers, int B, int K, int kv_heads,
                                 int L, int Lsrc, int Lmax, int head_dim, hipStream_t st) {
  if (K < 1 || K > BM_MAXK) return TA_ERR_ARG;
  if (B <= 0 || layers <= 0 || L <= 0) return TA_OK;
  if (!ksrc || !vsrc || !kdst || !vdst || kv_heads <= 0 || Lsrc < L || Lmax < L || head_dim <= 0 || head_dim % 8) return TA_ERR_ARG;
  const long total = (long)layers * B * K * kv_heads * L * (head_dim / 8);
  if (total > (long)INT_MAX * 128) return TA_ERR_ARG;
  TA_LAUNCH(kv_beam_expand_kernel, dim3(ta_cdiv(total, 256), 2), dim3(256), 0, st, (const uint4*)ksrc, (const uint4*)vsrc, (uint4*)kdst,
            (uint4*)vdst, layers, B, K, kv_heads, L, Lsrc, Lmax, head_dim / 8);
  TA_CHECK_LAUNCH();
  return TA_OK;
}

extern "C" int ta_kv_beam_reorder(void* kcache, void* vcache, int layers, int B, int K, int kv_heads, int L, int Lmax, int head_dim,
                                  int max_new, const int* parent, const int* slot_dev, hipStream_t st) {
  if (K < 1 || K > BM_MAXK) return TA_ERR_ARG;
  if (B <= 0 || layers <= 0 || max_new <= 0 || K == 1) return TA_OK;            // one beam: parent is the identity
  if (!kcache || !vcache || kv_heads <= 0 || L < 0 || Lmax < L + max_new || head_dim <= 0 || head_dim % 8 || !parent || !slot_dev ||
      B > 65535 || max_new > 65535)
    return TA_ERR_ARG;
  const int D8 = head_dim / 8;
  const dim3 grid(ta_cdiv(2L * layers * kv_heads * D8, 256), max_new, B);
#define KR(K_) case K_: TA_LAUNCH((kv_beam_reorder_kernel<K_>), grid, dim3(256), 0, st, (uint4*)kcache, (uint4*)vcache, layers, B, kv_heads, L, \
                                  Lmax, D8, parent, slot_dev); break
  switch (K) { KR(2); KR(3); KR(4); KR(5); KR(6); KR(7); KR(8); default: return TA_ERR_ARG; }
#undef KR
  TA_CHECK_LAUNCH();
  return TA_OK;
}
