// ta355 text alignment: Levenshtein distance with its S/D/I split (WER / CER) and the LCS word matching of the reference's
// timestamp evaluator (scripts/eval/evaluators/alignment.py:12-79), for ragged batches of int32 symbol ids (ta_text_align_i32).
// Contract: tests/text_align_ref.py ("Text alignment"): both tables are int32, both walks have a fixed tie rule
// (edit: diagonal, then deletion, then insertion; lcs: equal symbols, then up if L[i-1][j] > L[i][j-1], else left), every output is
// an exact integer, and neither the kernel nor the tiling changes a byte.
//
// A tile is CB = 64 CPL columns (hypothesis) by RB rows (reference) and is run by ONE wave: lane l owns the tile's columns
// l CPL .. l CPL + CPL - 1 in registers (their symbols and the row above) and, at step s, fills them in row s - l -- the wave sweeps
// the tile as a skewed anti-diagonal.  What a lane needs from its left is what lane l - 1 produced one step earlier (its last
// column's value; the value of the step before that is the diagonal), so one lane shift per step carries the row dependency and a
// second one carries the reference symbol down the lanes; lane 0 is fed from 64-row chunks (the reference symbols, and the column to
// the tile's left) that are loaded one chunk ahead.  There is no LDS and no barrier in a tile.  The two decision bits of a cell
// (edit: "the diagonal achieves D", "up achieves D"; lcs: "equal", "up > left") are gathered per column over 64 rows, so a lane
// stores one aligned pair of 64-bit words bits[col][row >> 6][2] every 64 rows (RB is a multiple of 64: a word never straddles two
// tiles).
//
// Short kernel: one workgroup (one wave) per pair whose hypothesis fits one tile (max_m <= TA_TEXT_ALIGN_SHORT_MAX_M): the pair is
// a single tile of all its rows, CPL chosen from max_m, and the same wave walks the bits back.
// Long kernel, the scheme of align_long.hip: launch k runs every tile (cb, rb) with cb + rb == k of every pair; the row that enters
// a tile (rowc[pair][col], overwritten in place by the tile when rows remain below it) and the column to its left
// (colc[pair][rb (RB + 1) + ...]: slot 0 the corner D[row0 - 1][c0 - 1], slot 1 + i the value in row i, overwritten in place with
// this tile's own last column once read -- only this tile touches row block rb in launch k) go through the workspace; kernel
// boundaries order them.  A first launch checks every pair and leaves a flag and the offset of its bits in the workspace; a last
// launch walks back with one wave per pair, 64 steps per window of prefetched words.
//
// Barrier safety: no workgroup waits for another -- no flags that are spun on, no grid barrier; the per-pair flag is written by an
// EARLIER launch.  The only barriers are in the prep kernel's scan, inside loops bounded by N and the workgroup size
// (workgroup-uniform), and one in the short kernel between the fill and the walk, reached by the whole workgroup (the refused-pair
// exit is taken by the whole workgroup before it).  Every tile's early exit (no such tile, refused pair) is taken by the whole wave.
#include "common.h"
#include "../../include/ta355.h"

typedef unsigned long long u64;

#define TXA_EDIT TA_TEXT_ALIGN_EDIT
#define TXA_LCS TA_TEXT_ALIGN_LCS
#define TXA_PREP_T 256

static_assert(TA_TEXT_ALIGN_MAX_COL_BLOCK == 512 && TA_TEXT_ALIGN_SHORT_MAX_M == TA_TEXT_ALIGN_MAX_COL_BLOCK, "CPL is 1, 2, 4 or 8");
static_assert(TA_TEXT_ALIGN_COL_BLOCK % 64 == 0 && TA_TEXT_ALIGN_ROW_BLOCK % 64 == 0, "tiles are whole words of decision bits");

// the workspace: flags[N] ints, bits_off[N] longs, then (long kernel only) rowc[N][max_m] and colc[N][max_n + nRB] ints, then the
// decision bits of every pair that asked for a path, m * ceil(n / 64) * 2 words each, at bits_off[pair]
struct TextAlignWs {
  long flags_bytes, off_bytes, rowc_ints, colc_ints, fixed;
};
static TextAlignWs text_align_ws(int N, int max_n, int max_m, bool is_short, int RB) {
  TextAlignWs w;
  w.flags_bytes = ((long)N * 4 + 7) & ~7L;
  w.off_bytes = (long)N * 8;
  w.rowc_ints = is_short ? 0 : (long)N * max_m;
  w.colc_ints = is_short ? 0 : (long)N * ((long)max_n + ((long)max_n + RB - 1) / RB);
  w.fixed = (w.flags_bytes + w.off_bytes + (w.rowc_ints + w.colc_ints) * 4 + 15) & ~15L;
  return w;
}

struct TextAlignArgs {
  const int* ref; const int* cu_ref; const int* hyp; const int* cu_hyp;
  int N, max_n, max_m, RB;
  int* dist; int* counts; int* map; int* status;
  int* flags; long* bits_off; int* rowc; int* colc;
  u64* bits; long bits_cap;                               // words
};

// one workgroup: refuse what the contract refuses (and a pair whose bits would not fit the workspace the caller gave), leave the
// verdict and the offset of the pair's bits for the later launches, and settle the distance of the pairs that have no tile
template <int MODE>
__global__ __launch_bounds__(TXA_PREP_T) void text_align_prep_kernel(TextAlignArgs a, int want_path) {
  __shared__ long sc[TXA_PREP_T];
  const int tid = threadIdx.x;
  long running = 0;
  for (int base = 0; base < a.N; base += TXA_PREP_T) {    // workgroup-uniform bounds
    const int p = base + tid;
    int n = 0, m = 0, bad = 0;
    long need = 0;
    if (p < a.N) {
      n = a.cu_ref[p + 1] - a.cu_ref[p];
      m = a.cu_hyp[p + 1] - a.cu_hyp[p];
      bad = n < 0 || m < 0 || n > a.max_n || m > a.max_m;  // the caller's maxima size the launches and the carries
      if (!bad && want_path) need = (long)m * ((n + 63) >> 6) * 2;
    }
    sc[tid] = need;
    __syncthreads();
    for (int off = 1; off < TXA_PREP_T; off <<= 1) {
      const long v = tid >= off ? sc[tid - off] : 0;
      __syncthreads();
      sc[tid] += v;
      __syncthreads();
    }
    const long excl = running + sc[tid] - need;
    running += sc[TXA_PREP_T - 1];
    __syncthreads();                                       // the next round overwrites sc
    if (p < a.N) {
      if (!bad && excl + need > a.bits_cap) bad = 1;
      a.flags[p] = bad;
      a.bits_off[p] = excl;
      a.status[p] = bad ? 2 : 0;
      if (bad) a.dist[p] = -1;
      else if (n == 0 || m == 0) a.dist[p] = MODE == TXA_EDIT ? n + m : 0;
    }
  }
}

// One tile by one wave.  r: the pair's reference symbols from the tile's first row (nr of them belong to the tile), h: the pair's
// hypothesis symbols (m), the tile's columns are c0 .. c0 + nc - 1.  rowc / lv: the pair's row carry and this row block's slot of
// the column carry (unused where the tile has no neighbour on that side).  Returns D[row0 + nr][c0 + nc] in every lane.
template <int CPL, int MODE, bool PATH>
__device__ __forceinline__ int text_tile(const int* __restrict__ r, const int* __restrict__ h, int n, int m, int row0, int nr, int c0,
                                         int nc, int* rowc, int* lv, u64* bits, long nW) {
  const int lane = threadIdx.x;
  const int colb = c0 + lane * CPL, cend = c0 + nc;
  const int Lmax = (nc - 1) / CPL, clast = (nc - 1) % CPL;            // the lane and the register that hold the tile's last column
  const bool has_left = c0 > 0, has_right = cend < m, load_row = row0 > 0, store_row = row0 + nr < n;
  int hs[CPL], prev[CPL];
  unsigned acc_a[CPL], acc_b[CPL], lo_a[CPL], lo_b[CPL];
  int enter_last = 0;
#pragma unroll
  for (int c = 0; c < CPL; ++c) {
    const int col = colb + c;
    const bool on = col < cend;
    hs[c] = on ? h[col] : 0;
    prev[c] = !on ? 0 : load_row ? rowc[col] : (MODE == TXA_EDIT ? col + 1 : 0);
    acc_a[c] = acc_b[c] = lo_a[c] = lo_b[c] = 0;
    if (c == clast) enter_last = prev[c];
  }
  int last = prev[CPL - 1];
  int diag = __shfl_up(last, 1, 64);                                   // D[row0 - 1][the column left of this lane's]
  const int corner = has_left ? lv[0] : (MODE == TXA_EDIT ? row0 : 0);
  if (lane == 0) diag = corner;

  int rch = 0, lch = 0, rcur = 0, left = 0;
  int rnx = lane < nr ? r[lane] : 0;                                   // one chunk of 64 rows ahead
  int lnx = has_left && lane < nr ? lv[1 + lane] : 0;
  const int steps = nr + Lmax;
  for (int s = 0; s < steps; ++s) {                                    // wave-uniform
    const int t = s & 63;
    if (t == 0) {
      rch = rnx;
      lch = lnx;
      const int g = s + 64 + lane;
      rnx = g < nr ? r[g] : 0;
      lnx = has_left && g < nr ? lv[1 + g] : 0;                        // rows this tile has not written yet (it writes rows <= s)
    }
    const int rin = __shfl(rch, t, 64);
    const int lin = has_left ? __shfl(lch, t, 64) : (MODE == TXA_EDIT ? row0 + s + 1 : 0);
    const int rup = __shfl_up(rcur, 1, 64), lup = __shfl_up(last, 1, 64);
    rcur = lane == 0 ? rin : rup;
    left = lane == 0 ? lin : lup;
    const int il = s - lane;                                           // this lane's row of the tile in this step
    if (il >= 0 && il < nr && lane <= Lmax) {
      int d = diag, lf = left;
      const int sh = il & 31;
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        const int up = prev[c];
        const bool eq = rcur == hs[c];
        int v;
        bool b0, b1;
        if (MODE == TXA_EDIT) {
          const int sub = d + (eq ? 0 : 1), del = up + 1, ins = lf + 1;
          const int mn = del < ins ? del : ins;
          v = sub < mn ? sub : mn;
          b0 = v == sub;
          b1 = v == del;
        } else {
          v = eq ? d + 1 : (up > lf ? up : lf);
          b0 = eq;
          b1 = up > lf;
        }
        if (PATH) {
          acc_a[c] |= (unsigned)b0 << sh;
          acc_b[c] |= (unsigned)b1 << sh;
        }
        d = up;
        lf = v;
        prev[c] = v;
      }
      diag = left;
      last = prev[CPL - 1];
      if (PATH) {
        const int sh64 = il & 63;
        const bool flush = sh64 == 63 || il == nr - 1;
        if (flush) {
          const long wi = ((long)row0 + il) >> 6;
#pragma unroll
          for (int c = 0; c < CPL; ++c) {
            const u64 wa = sh64 < 32 ? (u64)acc_a[c] : ((u64)acc_a[c] << 32) | lo_a[c];
            const u64 wb = sh64 < 32 ? (u64)acc_b[c] : ((u64)acc_b[c] << 32) | lo_b[c];
            if (colb + c < cend) {
              u64* w = bits + ((long)(colb + c) * nW + wi) * 2;
              w[0] = wa;
              w[1] = wb;
            }
            acc_a[c] = acc_b[c] = lo_a[c] = lo_b[c] = 0;
          }
        } else if (sh64 == 31) {
#pragma unroll
          for (int c = 0; c < CPL; ++c) {
            lo_a[c] = acc_a[c];
            lo_b[c] = acc_b[c];
            acc_a[c] = acc_b[c] = 0;
          }
        }
      }
      if (has_right && lane == Lmax) {                                 // the column the tile to the right reads in the next launch
        int v = prev[0];
#pragma unroll
        for (int c = 1; c < CPL; ++c) v = c == clast ? prev[c] : v;
        lv[1 + il] = v;
      }
    }
  }
  int fin = prev[0];
#pragma unroll
  for (int c = 1; c < CPL; ++c) fin = c == clast ? prev[c] : fin;
  if (store_row) {
#pragma unroll
    for (int c = 0; c < CPL; ++c)
      if (colb + c < cend) rowc[colb + c] = prev[c];
  }
  if (has_right && lane == Lmax) lv[0] = enter_last;                   // after the loop: the incoming corner has long been used
  return __shfl(fin, Lmax, 64);
}

__device__ __forceinline__ u64 txa_load(const u64* p) {               // the short kernel reads what its own wave has just written
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One wave walks a pair's bits back from (n, m).  In 64 steps i and j fall by at most 64 each, so lane l loads the two words
// (per bit plane) of column j - 1 - l that cover rows i - 64 .. i - 1, and the 64 steps run on lane-broadcast registers.  The
// substitutions follow from the distance: dist = S + D + I along the path.
template <int MODE>
__device__ __forceinline__ void text_walk(int n, int m, const u64* bits, long nW, int dist, int* counts, int* map) {
  const int lane = threadIdx.x;
  int i = n, j = m, ndiag = 0, ndel = 0, nins = 0;
  while (i > 0 && j > 0) {
    const int j0 = j;
    const long w0 = (i - 1) >> 6;
    const int col = j0 - 1 - lane;
    u64 a1 = 0, b1 = 0, a0 = 0, b0 = 0;
    if (col >= 0) {
      const u64* w = bits + ((long)col * nW + w0) * 2;
      a1 = txa_load(w);
      b1 = txa_load(w + 1);
      if (w0 > 0) {
        a0 = txa_load(w - 2);
        b0 = txa_load(w - 1);
      }
    }
    for (int st = 0; st < 64 && i > 0 && j > 0; ++st) {                // wave-uniform: i and j are the same in every lane
      const int row = i - 1, sh = row & 63;
      const bool cur = (row >> 6) == w0;
      const u64 a = cur ? a1 : a0, b = cur ? b1 : b0;
      const int mine = (int)((a >> sh) & 1) | ((int)((b >> sh) & 1) << 1);
      const int v = __shfl(mine, j0 - j, 64);
      if (v & 1) {
        if (lane == 0) map[row] = j - 1;
        --i; --j; ++ndiag;
      } else if (v & 2) {
        if (lane == 0) map[row] = -1;
        --i; ++ndel;
      } else {
        --j; ++nins;
      }
    }
  }
  for (int k = lane; k < i; k += 64) map[k] = -1;                      // edit: j == 0, deletions; lcs: unmatched
  if (lane == 0) {
    if (MODE == TXA_EDIT) {
      ndel += i;
      nins += j;
      const int sub = dist - ndel - nins;
      counts[0] = ndiag - sub; counts[1] = sub; counts[2] = ndel; counts[3] = nins;
    } else {
      counts[0] = ndiag; counts[1] = 0; counts[2] = n - ndiag; counts[3] = m - ndiag;
    }
  }
}

template <int CPL, int MODE, bool PATH>
__global__ __launch_bounds__(64) void text_align_short_kernel(TextAlignArgs a) {
  const int p = blockIdx.x;
  if (a.flags[p]) return;                                              // the whole workgroup, before the barrier
  const int k0 = a.cu_ref[p], q0 = a.cu_hyp[p];
  const int n = a.cu_ref[p + 1] - k0, m = a.cu_hyp[p + 1] - q0;
  const long nW = (n + 63) >> 6;
  u64* bits = PATH ? a.bits + a.bits_off[p] : nullptr;
  int dist = MODE == TXA_EDIT ? n + m : 0;                             // n == 0 or m == 0: the prep launch has written it
  if (n > 0 && m > 0) {
    dist = text_tile<CPL, MODE, PATH>(a.ref + k0, a.hyp + q0, n, m, 0, n, 0, m, nullptr, nullptr, bits, nW);
    if (threadIdx.x == 0) a.dist[p] = dist;
  }
  if (PATH) {
    __threadfence();
    __syncthreads();
    text_walk<MODE>(n, m, bits, nW, dist, a.counts + (long)p * 4, a.map + k0);
  }
}

template <int CPL, int MODE, bool PATH>
__global__ __launch_bounds__(64) void text_align_tile_kernel(TextAlignArgs a, int k, int cb_lo) {
  const int p = blockIdx.x;
  const int cb = cb_lo + blockIdx.y, rb = k - cb;
  if (rb < 0 || a.flags[p]) return;
  const int k0 = a.cu_ref[p], q0 = a.cu_hyp[p];
  const int n = a.cu_ref[p + 1] - k0, m = a.cu_hyp[p + 1] - q0;
  const int CB = 64 * CPL, RB = a.RB;
  const long c0l = (long)cb * CB, row0l = (long)rb * RB;
  if (c0l >= m || row0l >= n) return;                                  // no such tile in this pair
  const int c0 = (int)c0l, row0 = (int)row0l;
  const int nc = m - c0 < CB ? m - c0 : CB, nr = n - row0 < RB ? n - row0 : RB;
  const long nRB = ((long)a.max_n + RB - 1) / RB;
  int* rowc = a.rowc + (long)p * a.max_m;
  int* lv = a.colc + (long)p * (a.max_n + nRB) + (long)rb * (RB + 1);
  u64* bits = PATH ? a.bits + a.bits_off[p] : nullptr;
  const int fin = text_tile<CPL, MODE, PATH>(a.ref + k0 + row0, a.hyp + q0, n, m, row0, nr, c0, nc, rowc, lv, bits, (long)((n + 63) >> 6));
  if (row0 + nr == n && c0 + nc == m && threadIdx.x == 0) a.dist[p] = fin;      // the tile that holds D[n][m]
}

template <int MODE>
__global__ __launch_bounds__(64) void text_align_walk_kernel(TextAlignArgs a) {
  const int p = blockIdx.x;
  if (a.flags[p]) return;
  const int k0 = a.cu_ref[p];
  const int n = a.cu_ref[p + 1] - k0, m = a.cu_hyp[p + 1] - a.cu_hyp[p];
  text_walk<MODE>(n, m, a.bits + a.bits_off[p], (long)((n + 63) >> 6), a.dist[p], a.counts + (long)p * 4, a.map + k0);
}

// 0 = the defaults; is_short: both 0 and the hypotheses fit the short kernel's one tile
static bool text_align_tiling(int max_m, int* col_block, int* row_block, bool* is_short) {
  const int cb = *col_block, rb = *row_block;
  if (!(cb == 0 || cb == 64 || cb == 128 || cb == 256 || cb == 512)) return false;
  if (rb < 0 || rb % 64 || rb > TA_TEXT_ALIGN_MAX_LEN) return false;
  *is_short = cb == 0 && rb == 0 && max_m <= TA_TEXT_ALIGN_SHORT_MAX_M;
  if (cb == 0) *col_block = TA_TEXT_ALIGN_COL_BLOCK;
  if (rb == 0) *row_block = TA_TEXT_ALIGN_ROW_BLOCK;
  return true;
}

extern "C" long ta_text_align_workspace_bytes(const int* cu_ref_host, const int* cu_hyp_host, int N, int max_n, int max_m,
                                              int want_path, int col_block, int row_block) {
  bool is_short = false;
  if (!text_align_tiling(max_m, &col_block, &row_block, &is_short)) return -1;
  if (N <= 0 || max_n < 0 || max_m < 0) return 0;
  long total = text_align_ws(N, max_n, max_m, is_short, row_block).fixed;
  if (want_path && cu_ref_host && cu_hyp_host)
    for (int p = 0; p < N; ++p) {
      const long n = (long)cu_ref_host[p + 1] - cu_ref_host[p], m = (long)cu_hyp_host[p + 1] - cu_hyp_host[p];
      if (n < 0 || m < 0 || n > max_n || m > max_m) continue;          // refused on the device: no bits
      total += m * ((n + 63) >> 6) * 16;
    }
  return total;
}

extern "C" int ta_text_align_i32(const int* ref, const int* cu_ref, const int* hyp, const int* cu_hyp, int N, int max_n, int max_m,
                                 int mode, int want_path, int col_block, int row_block, int* dist, int* counts, int* map, int* status,
                                 void* ws, long ws_bytes, hipStream_t st) {
  if (N < 0 || N > TA_TEXT_ALIGN_MAX_PAIRS || max_n < 0 || max_n > TA_TEXT_ALIGN_MAX_LEN || max_m < 0 || max_m > TA_TEXT_ALIGN_MAX_LEN)
    return TA_ERR_ARG;
  if ((mode != TXA_EDIT && mode != TXA_LCS) || (want_path != 0 && want_path != 1)) return TA_ERR_ARG;
  bool is_short = false;
  if (!text_align_tiling(max_m, &col_block, &row_block, &is_short)) return TA_ERR_ARG;
  if (N == 0) return TA_OK;
  if (!cu_ref || !cu_hyp || !dist || !status) return TA_ERR_ARG;
  if ((max_n > 0 && !ref) || (max_m > 0 && !hyp)) return TA_ERR_ARG;
  if (want_path && (!counts || (max_n > 0 && !map))) return TA_ERR_ARG;
  const TextAlignWs w = text_align_ws(N, max_n, max_m, is_short, row_block);
  if (!ws || ws_bytes < w.fixed) return TA_ERR_ARG;

  TextAlignArgs a;
  a.ref = ref; a.cu_ref = cu_ref; a.hyp = hyp; a.cu_hyp = cu_hyp;
  a.N = N; a.max_n = max_n; a.max_m = max_m; a.RB = row_block;
  a.dist = dist; a.counts = counts; a.map = map; a.status = status;
  a.flags = (int*)ws;
  a.bits_off = (long*)((char*)ws + w.flags_bytes);
  a.rowc = (int*)((char*)ws + w.flags_bytes + w.off_bytes);
  a.colc = a.rowc + w.rowc_ints;
  a.bits = (u64*)((char*)ws + w.fixed);
  a.bits_cap = (ws_bytes - w.fixed) / 8;

  int rc = TA_OK;
  auto launched = [&]() { if (hipGetLastError() != hipSuccess) rc = TA_ERR_LAUNCH; return rc == TA_OK; };
  with_const<TXA_EDIT, TXA_LCS>(mode, [&](auto MODE) {
    TA_LAUNCH((text_align_prep_kernel<decltype(MODE)::value>), dim3(1), dim3(TXA_PREP_T), 0, st, a, want_path);
    if (!launched()) return;
    if (max_n == 0 || max_m == 0) {                                    // no tile anywhere: the walk settles counts and map
      if (want_path) {
        TA_LAUNCH((text_align_walk_kernel<decltype(MODE)::value>), dim3(N), dim3(64), 0, st, a);
        launched();
      }
      return;
    }
    const int cpl = is_short ? (max_m <= 64 ? 1 : max_m <= 128 ? 2 : max_m <= 256 ? 4 : 8) : col_block / 64;
    with_const<1, 2, 4, 8>(cpl, [&](auto CPL) {
      with_bool(want_path != 0, [&](auto PATH) {
        if (is_short) {
          TA_LAUNCH((text_align_short_kernel<decltype(CPL)::value, decltype(MODE)::value, decltype(PATH)::value>), dim3(N), dim3(64), 0, st, a);
          launched();
          return;
        }
        const long nCB = ((long)max_m + col_block - 1) / col_block, nRB = ((long)max_n + row_block - 1) / row_block;
        for (long k = 0; k < nCB + nRB - 1 && rc == TA_OK; ++k) {
          const long lo = k - (nRB - 1) > 0 ? k - (nRB - 1) : 0, hi = k < nCB - 1 ? k : nCB - 1;    // the column blocks alive in launch k
          TA_LAUNCH((text_align_tile_kernel<decltype(CPL)::value, decltype(MODE)::value, decltype(PATH)::value>), dim3(N, (unsigned)(hi - lo + 1)), dim3(64), 0, st, a,
                    (int)k, (int)lo);
          launched();
        }
        if (rc == TA_OK && want_path) {
          TA_LAUNCH((text_align_walk_kernel<decltype(MODE)::value>), dim3(N), dim3(64), 0, st, a);
          launched();
        }
      });
    });
  });
  return rc;
}
