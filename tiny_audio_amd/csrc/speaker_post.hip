// ta355 speaker turns: window labels -> frame votes -> runs -> merged turns, and words -> turns, for ragged batches of recordings
// (include/ta355.h, "speaker turns"; contract: the host functions of tiny_audio_amd/diarization.py, restated in integer frames by
// tests/speaker_post_ref.py; DESIGN.md section 3, "Speaker turns").  Every time of the reference's output is f * voting_rate for an
// integer frame f, so the kernels carry (speaker, f0, f1) and no float crosses the ABI for the turns.  The votes are integers; the VAD
// index and the merge rules are float64, evaluated as Python evaluates them (two roundings for a * r - b * r, an IEEE divide,
// truncation toward zero), so contraction is off for the whole file and no fast-math flag is on it.
//
// ---- ta_spk_vote_i32, three launches behind one memset of the counters (recording r: nf = n_frames[r], tiles of SPK_T frames):
//  1 spk_scatter_kernel, a lane per window: +1 at first and -1 at min(last, nf) of its speaker's difference array (int32 [R, S, ldf]),
//    and the same two steps on the per-tile sums (int32 [R, NT, 16]).  Integer atomics: the result does not depend on their order.
//  2 spk_owner_kernel, a workgroup per tile, four frames per lane: per speaker the count before the tile (the tile sums below it), a
//    workgroup scan of the differences, the arg-max with the lowest index among equals, then the VAD read.  Frame i0 - 1 is recomputed
//    from the counts before the tile, so the boundary flags need no neighbour workgroup.  Frame nf is a virtual silent frame that closes
//    a run reaching the end.  Per frame one byte: owner + 1 | start << 5 | end << 6; per tile the two flag counts.
//  3 spk_compact_kernel, same grid: the flag counts below the tile, a workgroup scan of the flags, run k = (k-th start, k-th end).
//    The tile that holds frame nf writes n_runs and status.  Nobody waits for another workgroup.
// ---- ta_spk_merge_i32: one workgroup per recording, runs staged through LDS SPK_MERGE_TILE at a time, lane 0 walks them.
// ---- ta_spk_words_f64: SPK_WORD_LANES lanes per word, segments staged through LDS SPK_SEG_TILE at a time, lexicographic minima.
#include "common.h"
#include "../../include/ta355.h"

#pragma clang fp contract(off)

#define SPK_THREADS 256
#define SPK_T TA_SPK_FRAME_TILE                           // frames per workgroup of the owner and compaction kernels
#define SPK_FPL (SPK_T / SPK_THREADS)                     // frames per lane
#define SPK_MERGE_TILE 1024
#define SPK_SEG_TILE TA_SPK_SEG_TILE
#define SPK_WORD_LANES 16
#define SPK_WORDS_PER_WG (SPK_THREADS / SPK_WORD_LANES)

static_assert(SPK_FPL == 4, "a lane loads its frames as one int4 / uchar4");
static_assert(TA_SPK_MAX_SPEAKERS == 16 && SPK_THREADS == 16 * 16, "the tile sums are reduced by 16 groups of 16 lanes");
static_assert(TA_SPK_MAX_SPEAKERS + 1 < 32, "owner + 1 fits the five low bits of a frame's byte");

namespace {
struct spk_ws {                                           // the workspace, carved the same way by the query and the entry point
  long ldf, NT, diff_off, tsum_off, bad_off, zero_bytes, code_off, tcnt_off, bytes;
};
__host__ inline spk_ws spk_layout(int R, int S, long max_frames) {
  spk_ws w;
  w.ldf = (max_frames + 1 + 3) / 4 * 4;                   // indices 0 .. max_frames, rows aligned for int4
  w.NT = max_frames / SPK_T + 1;                          // tiles that cover index max_frames
  w.diff_off = 0;
  w.tsum_off = w.diff_off + (long)R * S * w.ldf * 4;
  w.bad_off = w.tsum_off + (long)R * w.NT * 16 * 4;
  w.zero_bytes = w.bad_off + (long)((R + 3) / 4 * 4) * 4; // everything up to here starts from zero
  w.code_off = w.zero_bytes;
  w.tcnt_off = w.code_off + (long)R * w.ldf;
  w.bytes = w.tcnt_off + (long)R * w.NT * 2 * 4;
  return w;
}
bool spk_options_ok(const ta_spk_post_options* o) {
  if (!o) return false;
  const double v[5] = {o->voting_rate, o->vad_frame_s, o->min_segment_s, o->short_gap_s, o->same_gap_s};
  for (double x : v)
    if (!(x > 0.0 && x < INFINITY)) return false;
  return true;
}
}  // namespace

// inclusive scan over the 64 lanes of a wave
__device__ __forceinline__ int spk_wave_scan(int v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(v, d);
    if (lane >= d) v += u;
  }
  return v;
}

// exclusive scan over the workgroup; `wtot` is int[4] of LDS that nobody else touches until the next barrier after the call
__device__ __forceinline__ int spk_block_scan_excl(int v, int tid, int* wtot, int* total) {
  const int lane = tid & 63, wave = tid >> 6;
  const int inc = spk_wave_scan(v, lane);
  if (lane == 63) wtot[wave] = inc;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < SPK_THREADS / 64; ++w) {
    const int t = wtot[w];
    if (w < wave) before += t;
    all += t;
  }
  if (total) *total = all;
  return before + inc - v;
}

__global__ __launch_bounds__(SPK_THREADS) void spk_scatter_kernel(const int* __restrict__ first, const int* __restrict__ last,
                                                                  const int* __restrict__ label, const int* __restrict__ cu_win, int R, int S,
                                                                  const int* __restrict__ n_frames, long max_frames, long sum_windows,
                                                                  int* __restrict__ diff, int* __restrict__ tsum, int* __restrict__ bad,
                                                                  long ldf, long NT) {
  __shared__ int cu[TA_SPK_MAX_RECORDINGS + 1];
  const int tid = threadIdx.x;
  for (int k = tid; k <= R; k += SPK_THREADS) cu[k] = cu_win[k];
  __syncthreads();
  const long w = (long)blockIdx.x * SPK_THREADS + tid;
  if (w >= sum_windows) return;
  int r = 0;
  for (int k = 1; k <= R; ++k) r += cu[k] <= w ? 1 : 0;    // windows of recording r: cu[r] <= w < cu[r + 1]
  if (r >= R || w < cu[0]) return;                         // not inside any recording's range
  const long nf = n_frames[r];
  if (nf < 0 || nf > max_frames) return;                   // (the compaction kernel reports it)
  const int lo = first[w], lbl = label[w];
  const long la = last[w];
  if (lo < 0 || lbl < 0 || lbl >= S) {                     // refused by the Python layer; here it must not index anything
    atomicOr(bad + r, 1);
    return;
  }
  const long hi = la < nf ? la : nf;
  if ((long)lo >= hi) return;                              // empty, or first beyond the grid
  int* d = diff + ((long)r * S + lbl) * ldf;
  atomicAdd(d + lo, 1);
  atomicAdd(d + hi, -1);                                   // hi <= nf <= max_frames < ldf
  const long tl = lo / SPK_T, th = hi / SPK_T;             // th <= max_frames / SPK_T = NT - 1
  if (tl != th) {
    atomicAdd(tsum + ((long)r * NT + tl) * 16 + lbl, 1);
    atomicAdd(tsum + ((long)r * NT + th) * 16 + lbl, -1);
  }
}

// the speech decision of voting frame f: flags[clip((long)((f * voting_rate) / vad_frame_s), 0, nv - 1)], nv == 0: silence
__device__ __forceinline__ bool spk_speech(long f, const unsigned char* __restrict__ flags, long nv, double vr, double vf) {
  if (nv <= 0) return false;
  const double q = ((double)f * vr) / vf;                  // >= 0: both options are positive
  const long at = q >= (double)nv ? nv - 1 : (long)q;      // truncation toward zero, clipped above (and never out of long's range)
  return flags[at] != 0;
}

__global__ __launch_bounds__(SPK_THREADS) void spk_owner_kernel(const int* __restrict__ diff, const int* __restrict__ tsum, int S,
                                                                const int* __restrict__ n_frames, long max_frames,
                                                                const unsigned char* __restrict__ vad, long ld_vad, const int* __restrict__ n_vad,
                                                                double vr, double vf, unsigned char* __restrict__ code, int* __restrict__ tcnt,
                                                                long ldf, long NT) {
  __shared__ int part[16][17];
  __shared__ int base[16];
  __shared__ int wtot[2][SPK_THREADS / 64];
  __shared__ int lastown[SPK_THREADS];
  const int r = blockIdx.y, tid = threadIdx.x;
  const long tile = blockIdx.x, i0 = tile * SPK_T;
  const long nf = n_frames[r];
  if (nf < 0 || nf > max_frames || i0 > nf) return;        // uniform over the workgroup, before any barrier
  {                                                        // votes before the tile: the sums of the tiles below it
    const int s = tid & 15, g = tid >> 4;
    int acc = 0;
    if (s < S)
      for (long t = g; t < tile; t += 16) acc += tsum[((long)r * NT + t) * 16 + s];
    part[g][s] = acc;
    __syncthreads();
    if (tid < 16) {
      int b = 0;
      for (int k = 0; k < 16; ++k) b += part[k][tid];
      base[tid] = b;
    }
    __syncthreads();
  }
  const long f0 = i0 + SPK_FPL * tid;                      // this lane's first frame; f0 % 4 == 0 and ldf % 4 == 0
  int best[SPK_FPL], who[SPK_FPL], bestp = 0, whop = -1;
#pragma unroll
  for (int k = 0; k < SPK_FPL; ++k) { best[k] = 0; who[k] = -1; }
  for (int s = 0; s < S; ++s) {
    int4 d = make_int4(0, 0, 0, 0);
    if (f0 < ldf) d = *(const int4*)(diff + ((long)r * S + s) * ldf + f0);
    const int c[SPK_FPL] = {d.x, d.x + d.y, d.x + d.y + d.z, d.x + d.y + d.z + d.w};
    const int b = base[s] + spk_block_scan_excl(c[SPK_FPL - 1], tid, wtot[s & 1], nullptr);
    if (base[s] > bestp) { bestp = base[s]; whop = s; }    // frame i0 - 1: strictly greater, so the lowest index among the maxima
#pragma unroll
    for (int k = 0; k < SPK_FPL; ++k)
      if (b + c[k] > best[k]) { best[k] = b + c[k]; who[k] = s; }
  }
  const long nv0 = n_vad[r];
  const long nv = nv0 < 0 ? 0 : (nv0 > ld_vad ? ld_vad : nv0);
  const unsigned char* flags = vad + (long)r * ld_vad;
#pragma unroll
  for (int k = 0; k < SPK_FPL; ++k) {                      // every frame reads its decision (the index is clipped: any f is in bounds)
    const long f = f0 + k;
    const bool heard = spk_speech(f, flags, nv, vr, vf);
    who[k] = (f < nf && heard) ? who[k] : -1;
  }
  const bool heardp = spk_speech(i0 > 0 ? i0 - 1 : 0, flags, nv, vr, vf);
  whop = (i0 > 0 && heardp) ? whop : -1;                   // (i0 - 1 < nf: i0 <= nf)
  lastown[tid] = who[SPK_FPL - 1];
  __syncthreads();
  int prev = tid == 0 ? whop : lastown[tid - 1];
  unsigned char out[SPK_FPL];
  int cnt = 0;                                             // starts | ends << 16 (at most SPK_T of either in a tile)
#pragma unroll
  for (int k = 0; k < SPK_FPL; ++k) {
    const long f = f0 + k;
    int cd = 0;
    if (f <= nf) {                                         // frame nf: silent, it closes a run that reaches the end
      const int start = who[k] != -1 && who[k] != prev, end = prev != -1 && who[k] != prev;
      cd = (who[k] + 1) | (start << 5) | (end << 6);
      cnt += start + (end << 16);
      prev = who[k];
    }
    out[k] = (unsigned char)cd;
  }
  if (f0 < ldf) *(uchar4*)(code + (long)r * ldf + f0) = make_uchar4(out[0], out[1], out[2], out[3]);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d);
  __shared__ int wcnt[SPK_THREADS / 64];
  if ((tid & 63) == 0) wcnt[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) {
    int all = 0;
    for (int w = 0; w < SPK_THREADS / 64; ++w) all += wcnt[w];
    tcnt[((long)r * NT + tile) * 2] = all & 0xffff;
    tcnt[((long)r * NT + tile) * 2 + 1] = all >> 16;
  }
}

__global__ __launch_bounds__(SPK_THREADS) void spk_compact_kernel(const unsigned char* __restrict__ code, const int* __restrict__ tcnt,
                                                                  const int* __restrict__ bad, const int* __restrict__ n_frames,
                                                                  long max_frames, const int* __restrict__ cu_cap, int* __restrict__ run_spk,
                                                                  int* __restrict__ run_f0, int* __restrict__ run_f1, int* __restrict__ n_runs,
                                                                  int* __restrict__ status, long ldf, long NT) {
  __shared__ int red[2][SPK_THREADS / 64];
  __shared__ int wtot[2][SPK_THREADS / 64];
  const int r = blockIdx.y, tid = threadIdx.x;
  const long tile = blockIdx.x, i0 = tile * SPK_T;
  const long nf = n_frames[r];
  if (nf < 0 || nf > max_frames) {                         // refused: no runs
    if (tile == 0 && tid == 0) { n_runs[r] = 0; status[r] = 2; }
    return;
  }
  if (i0 > nf) return;
  int bs = 0, be = 0;                                      // starts and ends in the tiles below this one
  for (long t = tid; t < tile; t += SPK_THREADS) {
    bs += tcnt[((long)r * NT + t) * 2];
    be += tcnt[((long)r * NT + t) * 2 + 1];
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { bs += __shfl_xor(bs, d); be += __shfl_xor(be, d); }
  if ((tid & 63) == 0) { red[0][tid >> 6] = bs; red[1][tid >> 6] = be; }
  __syncthreads();
  bs = be = 0;
  for (int w = 0; w < SPK_THREADS / 64; ++w) { bs += red[0][w]; be += red[1][w]; }
  const long f0 = i0 + SPK_FPL * tid;
  uchar4 c4 = make_uchar4(0, 0, 0, 0);
  if (f0 < ldf) c4 = *(const uchar4*)(code + (long)r * ldf + f0);
  const int c[SPK_FPL] = {c4.x, c4.y, c4.z, c4.w};
  int ns = 0, ne = 0;
#pragma unroll
  for (int k = 0; k < SPK_FPL; ++k) { ns += (c[k] >> 5) & 1; ne += (c[k] >> 6) & 1; }
  int tot_s = 0;
  int ks = bs + spk_block_scan_excl(ns, tid, wtot[0], &tot_s);
  int ke = be + spk_block_scan_excl(ne, tid, wtot[1], nullptr);
  const long o = cu_cap[r];
  const long cap0 = (long)cu_cap[r + 1] - o, cap = cap0 < 0 ? 0 : cap0;
#pragma unroll
  for (int k = 0; k < SPK_FPL; ++k) {
    if ((c[k] >> 5) & 1) {
      if (ks < cap) { run_spk[o + ks] = (c[k] & 31) - 1; run_f0[o + ks] = (int)(f0 + k); }
      ++ks;
    }
    if ((c[k] >> 6) & 1) {
      if (ke < cap) run_f1[o + ke] = (int)(f0 + k);
      ++ke;
    }
  }
  if (tile == nf / SPK_T && tid == 0) {                    // the tile of the closing frame knows the total
    const long total = (long)bs + tot_s;
    n_runs[r] = (int)(total < cap ? total : cap);
    status[r] = bad[r] ? 2 : (total > cap ? 1 : 0);
  }
}

__global__ __launch_bounds__(SPK_THREADS) void spk_merge_kernel(const int* __restrict__ run_spk, const int* __restrict__ run_f0,
                                                                const int* __restrict__ run_f1, const int* __restrict__ cu_run,
                                                                const int* __restrict__ n_run, double vr, double min_seg, double short_gap, double same_gap, int* __restrict__ seg_spk,
                                                                int* __restrict__ seg_f0, int* __restrict__ seg_f1, int* __restrict__ n_seg) {
  __shared__ int ls[3][SPK_MERGE_TILE];
  const int r = blockIdx.x, tid = threadIdx.x;
  const long o = cu_run[r];
  const long room = (long)cu_run[r + 1] - o, n1 = n_run ? (long)n_run[r] : room;
  const long n = n1 < 0 || room < 0 ? 0 : (n1 < room ? n1 : room);      // never beyond the recording's own range
  bool have = false;                                       // the last kept turn (lane 0 only)
  int cs = 0, c0 = 0, c1 = 0;
  long cnt = 0;
  for (long b = 0; b < n; b += SPK_MERGE_TILE) {           // n is uniform over the workgroup: so are the barriers
    const int m = (int)(n - b < SPK_MERGE_TILE ? n - b : SPK_MERGE_TILE);
    for (int i = tid; i < m; i += SPK_THREADS) {
      ls[0][i] = run_spk[o + b + i];
      ls[1][i] = run_f0[o + b + i];
      ls[2][i] = run_f1[o + b + i];
    }
    __syncthreads();
    if (tid == 0)
      for (int i = 0; i < m; ++i) {
        const int s = ls[0][i], a = ls[1][i], e = ls[2][i];
        const double start = (double)a * vr, end = (double)e * vr;
        const bool is_short = (end - start) < min_seg;
        const double near = is_short ? short_gap : same_gap;
        if (have && cs == s && (start - (double)c1 * vr) < near) {
          c1 = e;
        } else if (!is_short) {
          if (have) { seg_spk[o + cnt - 1] = cs; seg_f0[o + cnt - 1] = c0; seg_f1[o + cnt - 1] = c1; }
          have = true; cs = s; c0 = a; c1 = e;
          ++cnt;                                           // cnt <= runs read so far: the turns fit the runs' room
        }
      }
    __syncthreads();
  }
  if (tid == 0) {
    if (have) { seg_spk[o + cnt - 1] = cs; seg_f0[o + cnt - 1] = c0; seg_f1[o + cnt - 1] = c1; }
    n_seg[r] = (int)cnt;
  }
}

__global__ __launch_bounds__(SPK_THREADS) void spk_words_kernel(const double* __restrict__ word_start, const double* __restrict__ word_end,
                                                                const int* __restrict__ cu_word, const double* __restrict__ seg_start,
                                                                const double* __restrict__ seg_end, const int* __restrict__ cu_seg,
                                                                int* __restrict__ out) {
  __shared__ double ss[SPK_SEG_TILE], se[SPK_SEG_TILE];
  const int r = blockIdx.y, tid = threadIdx.x, sub = tid & (SPK_WORD_LANES - 1);
  const long wo = cu_word[r], so = cu_seg[r];
  const long W = (long)cu_word[r + 1] - wo, G0 = (long)cu_seg[r + 1] - so, G = G0 < 0 ? 0 : G0;
  const long w = (long)blockIdx.x * SPK_WORDS_PER_WG + tid / SPK_WORD_LANES;
  if ((long)blockIdx.x * SPK_WORDS_PER_WG >= W) return;    // uniform over the workgroup
  const bool live = w < W;
  const double mid = live ? (word_start[wo + w] + word_end[wo + w]) / 2 : 0.0;
  int inside = 0x7fffffff, near_i = 0x7fffffff;            // lowest containing index; lowest index of the smallest distance
  double near_d = INFINITY;
  for (long b = 0; b < G; b += SPK_SEG_TILE) {
    const int m = (int)(G - b < SPK_SEG_TILE ? G - b : SPK_SEG_TILE);
    for (int i = tid; i < m; i += SPK_THREADS) { ss[i] = seg_start[so + b + i]; se[i] = seg_end[so + b + i]; }
    __syncthreads();
    for (int i = sub; i < m; i += SPK_WORD_LANES) {        // ascending per lane: `<` keeps the lowest index
      const double a = ss[i], e = se[i];
      const int g = (int)(b + i);
      if (a <= mid && mid <= e && g < inside) inside = g;
      const double d = fabs(mid - (a + e) / 2);
      if (d < near_d) { near_d = d; near_i = g; }
    }
    __syncthreads();
  }
#pragma unroll
  for (int d = SPK_WORD_LANES / 2; d >= 1; d >>= 1) {
    const int oi = __shfl_xor(inside, d), on = __shfl_xor(near_i, d);
    const double od = __shfl_xor(near_d, d);
    if (oi < inside) inside = oi;
    if (od < near_d || (od == near_d && on < near_i)) { near_d = od; near_i = on; }
  }
  if (live && sub == 0) out[wo + w] = G == 0 ? -1 : (inside != 0x7fffffff ? inside : near_i);
}

// ---------------------------------------------------------------------------------------------------------------- host
extern "C" long ta_spk_post_workspace_bytes(int R, int S, long max_frames, long sum_windows) {
  if (R < 1 || R > TA_SPK_MAX_RECORDINGS || S < 1 || S > TA_SPK_MAX_SPEAKERS || max_frames < 0 || max_frames > TA_SPK_MAX_FRAMES ||
      sum_windows < 0 || sum_windows > TA_SPK_MAX_ITEMS)
    return -1;
  return spk_layout(R, S, max_frames).bytes;
}

extern "C" int ta_spk_vote_i32(const int* first, const int* last, const int* label, const int* cu_win, long sum_windows, int R, int S,
                               const int* n_frames, long max_frames, const unsigned char* vad, long ld_vad, const int* n_vad,
                               const ta_spk_post_options* opt, const int* cu_cap, int* run_spk, int* run_f0, int* run_f1, int* n_runs,
                               int* status, void* ws, long ws_bytes, hipStream_t st) {
  if (R < 0 || R > TA_SPK_MAX_RECORDINGS || !spk_options_ok(opt)) return TA_ERR_ARG;
  if (R == 0) return TA_OK;
  const long need = ta_spk_post_workspace_bytes(R, S, max_frames, sum_windows);
  if (need < 0 || !ws || ws_bytes < need || ld_vad < 0) return TA_ERR_ARG;
  if (!cu_win || !n_frames || !n_vad || !cu_cap || !n_runs || !status || (ld_vad > 0 && !vad)) return TA_ERR_ARG;
  if (sum_windows > 0 && (!first || !last || !label)) return TA_ERR_ARG;
  const spk_ws L = spk_layout(R, S, max_frames);
  char* p = (char*)ws;
  int *diff = (int*)(p + L.diff_off), *tsum = (int*)(p + L.tsum_off), *bad = (int*)(p + L.bad_off), *tcnt = (int*)(p + L.tcnt_off);
  unsigned char* code = (unsigned char*)(p + L.code_off);
  (void)hipGetLastError();
  if (hipMemsetAsync(p, 0, (size_t)L.zero_bytes, st) != hipSuccess) return TA_ERR_LAUNCH;
  if (sum_windows > 0) {
    TA_LAUNCH(spk_scatter_kernel, dim3((unsigned)((sum_windows + SPK_THREADS - 1) / SPK_THREADS)), dim3(SPK_THREADS), 0, st, first, last,
              label, cu_win, R, S, n_frames, max_frames, sum_windows, diff, tsum, bad, L.ldf, L.NT);
    TA_CHECK_LAUNCH();
  }
  const dim3 grid((unsigned)L.NT, R);
  TA_LAUNCH(spk_owner_kernel, grid, dim3(SPK_THREADS), 0, st, diff, tsum, S, n_frames, max_frames, vad, ld_vad, n_vad, opt->voting_rate,
            opt->vad_frame_s, code, tcnt, L.ldf, L.NT);
  TA_CHECK_LAUNCH();
  TA_LAUNCH(spk_compact_kernel, grid, dim3(SPK_THREADS), 0, st, code, tcnt, bad, n_frames, max_frames, cu_cap, run_spk, run_f0, run_f1,
            n_runs, status, L.ldf, L.NT);
  TA_CHECK_LAUNCH();
  return TA_OK;
}

extern "C" int ta_spk_merge_i32(const int* run_spk, const int* run_f0, const int* run_f1, const int* cu_run, const int* n_run, int R,
                                const ta_spk_post_options* opt, int* seg_spk, int* seg_f0, int* seg_f1, int* n_seg, hipStream_t st) {
  if (R < 0 || R > TA_SPK_MAX_RECORDINGS || !spk_options_ok(opt)) return TA_ERR_ARG;
  if (R == 0) return TA_OK;
  if (!cu_run || !n_seg) return TA_ERR_ARG;
  TA_LAUNCH(spk_merge_kernel, dim3(R), dim3(SPK_THREADS), 0, st, run_spk, run_f0, run_f1, cu_run, n_run, opt->voting_rate, opt->min_segment_s,
            opt->short_gap_s, opt->same_gap_s, seg_spk, seg_f0, seg_f1, n_seg);
  TA_CHECK_LAUNCH();
  return TA_OK;
}

extern "C" int ta_spk_words_f64(const double* word_start, const double* word_end, const int* cu_word, const double* seg_start,
                                const double* seg_end, const int* cu_seg, int R, long max_words, int* out, hipStream_t st) {
  if (R < 0 || R > TA_SPK_MAX_RECORDINGS || max_words < 0 || max_words > TA_SPK_MAX_ITEMS) return TA_ERR_ARG;
  if (R == 0 || max_words == 0) return TA_OK;
  if (!word_start || !word_end || !cu_word || !cu_seg || !out) return TA_ERR_ARG;
  TA_LAUNCH(spk_words_kernel, dim3((unsigned)((max_words + SPK_WORDS_PER_WG - 1) / SPK_WORDS_PER_WG), R), dim3(SPK_THREADS), 0, st,
            word_start, word_end, cu_word, seg_start, seg_end, cu_seg, out);
  TA_CHECK_LAUNCH();
  return TA_OK;
}
