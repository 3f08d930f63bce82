// ta355 long-form segmentation: where to cut a whole recording into encoder windows, and the cut itself (include/ta355.h,
// "long-form segmentation"; contract tests/segment_ref.py; DESIGN.md section 3, "Long-form transcription").  R recordings lie in one
// flat f32 buffer, recording r at samples offsets[r] .. offsets[r + 1] (n of them).  Its grid has the positions p = 0 .. T with
// T = ceil(n / 160), position p standing for sample 160 p and position T for sample n.
//
// ---- ta_wave_cut_cost_f32: three launches, no atomics, nobody waits for another workgroup.
//  1 cut_power_kernel, one workgroup per tile of SEG_TP = 128 positions: the tile's samples [160 p0 - 200, 160 (p0 + 128) + 40) are
//    read once, 16 bytes per lane where the recording starts on a 16-byte boundary and 4 bytes otherwise; samples outside [0, n) are 0.
//      quad q   = ((x0 x0 + x1 x1) + x2 x2) + x3 x3                          4 consecutive samples        3 additions
//      block b  = quad[10 b] + quad[10 b + 1] + ... + quad[10 b + 9]         40 samples, left to right    9 additions
//      pw[p]    = (block[4 p - 5] + ... + block[4 p + 4]) / 400              left to right                9 additions
//    and for P the tile's own samples [160 p0, 160 (p0 + 128)), its 512 blocks 4 p0 .. 4 p0 + 511:
//      thread t = block[4 p0 + 2 t] + block[4 p0 + 2 t + 1]; the xor butterfly over a wave's 64 lanes (offsets 32, 16, .. 1); then
//      (wave 0 + wave 1) + (wave 2 + wave 3) -> partial[r][tile]                                          1 + 6 + 2 additions
//  2 cut_total_kernel, one workgroup per recording: thread t adds partial[t], partial[t + 256], ... in that order (at the cap of
//    1 048 576 positions 8193 tiles, so at most 33 terms, 32 additions), the same butterfly and wave order (8 additions), and one
//    thread forms pen[r] = cut_penalty * (float)((double)total / n).
//  3 cut_smooth_kernel, one thread per position: cost[p] = (pw[p - h] + ... + pw[p + h]) / (2 h + 1) + pen[r], left to right, positions
//    outside [0, T] skipped (they count as 0; the divisor is fixed)                                       2 h + 1 additions
// Every term is non-negative and every step is one f32 rounding (a product and the addition after it may contract into one fma: one
// rounding instead of two).  The longest chains of additions: through s[p] 3 + 9 + 9 + 2 h + 1 = 2 h + 22; through P at the cap
// 3 + 9 + 9 + 32 + 8 + 1 = 62.  K = the longest chain + 3 (the square, the two scalings) = max(2 h + 25, 65): TA_CUT_COST_K(h) of the
// header.  |cost - exact| <= gamma_K cost with gamma_K = K u / (1 - K u), u = 2^-24.  The order depends on nothing but n and h: two
// runs give the same bits, and a recording of zeros costs exactly 0.
//
// ---- ta_cut_plan_f32: one workgroup per recording runs
//      dp[0] = 0,   dp[p] = (p < T ? cost[p] : 0) + min{dp[s] : max(0, p - max_len) <= s <= p - min_len},   back[p] = the lowest such s
// (one f32 addition; dp[p] = +inf and back[p] = -1 where the range is empty, dp[p] = +inf and back[p] = its lowest s where nothing in
// it is finite).  The positions (b min_len, (b + 1) min_len] of block b read dp only at s <= b min_len, so the blocks run one after
// the other with a barrier between them and every block is parallel over the lanes.  dp lives in an LDS ring of
// ring = roundup64(max_len + min_len) <= 4544 values (18 KB): block b writes the slots of its own positions, which alias positions
// <= b min_len - max_len that no window of this or a later block reaches.
// The window minimum is two-level when a window (max_len - min_len + 1 positions) is at least 64 wide; a narrower one never holds a
// whole chunk, is scanned directly, and no pairs are formed.  Every aligned chunk of 64 positions gets its (minimum, lowest position)
// pair once, by one wave (a lane per position, then the xor butterfly over pairs, the lower position winning among equal values), in
// the block that completes it.  A chunk that a window holds entirely lies below that window's end <= b min_len, so it was completed
// before block b.  The block that completes chunk k writes positions up to 64 k + 62 + min_len before the pair is formed; their slots
// alias chunk k's only if ring <= 62 + min_len, i.e. max_len <= 62, and then the window is narrower than 64 and there are no pairs.
// A window scans its first chunk's tail, the whole chunks' pairs, and its last chunk's head, in ascending position with a strict <,
// which keeps the lowest position among equal values: at most 63 + 45 + 64 comparisons per position instead of 3000.  One lane walks
// back[] from T and writes cuts[] ascending.  Every loop runs to a bound derived from T, min_len and max_len, all uniform over the
// workgroup; no barrier sits under a condition that lanes could disagree on.
//
// ---- ta_wave_windows_f32: window w of the table copies wav[start[w] .. start[w] + len[w]) to row w of out [W, Ls] and zeros the rest
// of the row; 16-byte stores when Ls is a multiple of 4 (4-byte stores otherwise), 16-byte loads where the source quad is aligned and
// inside the buffer, 4-byte loads otherwise; nothing outside [0, total) is ever read.
#include "common.h"
#include "../../include/ta355.h"

#define SEG_T 256                              // threads of the cost and gather kernels
#define SEG_PT 1024                            // threads of the plan kernel: a lane per position of a block at the default min_len
#define SEG_TP 128                             // positions per tile of the power pass
#define SEG_QUADS (SEG_TP * 40 + 60)           // 20 720 samples = 5180 quads = 518 blocks per tile
#define SEG_BLOCKS (SEG_TP * 4 + 6)
#define SEG_CH 64                              // positions per chunk of the window minimum
#define SEG_RING_MAX ((TA_CUT_MAX_LEN + TA_CUT_MAX_LEN / 2 + SEG_CH - 1) / SEG_CH * SEG_CH)

static_assert(SEG_T == 2 * SEG_TP && SEG_T == 256, "two blocks per thread in the partial sum, four waves");
static_assert(SEG_CH == 64 && SEG_PT % 64 == 0, "a chunk of the window minimum is one wave");
static_assert(SEG_BLOCKS == 518 && SEG_QUADS == 5180, "the tile geometry the header comment states");
static_assert(TA_CUT_HOP == 160 && TA_CUT_POWER_WINDOW == 400, "blocks of 40 samples tile both the hop and the half window");

__device__ __forceinline__ long seg_positions(long n) { return (n + TA_CUT_HOP - 1) / TA_CUT_HOP; }      // T

__global__ __launch_bounds__(SEG_T) void cut_power_kernel(const float* __restrict__ wav, const long* __restrict__ offsets, long max_n,
                                                          float* __restrict__ pw, long ld, float* __restrict__ partial, long ntl) {
  __shared__ float quad[SEG_QUADS];
  __shared__ float blk[SEG_BLOCKS];
  __shared__ float wsum[SEG_T / 64];
  const int r = blockIdx.y, tid = threadIdx.x;
  const long o = offsets[r], n = offsets[r + 1] - o;
  if (n <= 0 || n > max_n) return;                        // refused: nothing of this recording is written (uniform, before any barrier)
  const long T = seg_positions(n);
  const long p0 = (long)blockIdx.x * SEG_TP;
  if (p0 > T) return;
  const float* x = wav + o;
  const bool al = (((uintptr_t)x) & 15) == 0;
  const long s0 = p0 * TA_CUT_HOP - TA_CUT_POWER_WINDOW / 2;     // a multiple of 4, possibly negative
  for (int q = tid; q < SEG_QUADS; q += SEG_T) {
    const long i = s0 + 4L * q;
    float a = 0.f, b = 0.f, c = 0.f, d = 0.f;
    if (i >= 0 && i + 4 <= n && al) {
      const float4 v = *(const float4*)(x + i);
      a = v.x; b = v.y; c = v.z; d = v.w;
    } else if (i + 4 > 0 && i < n) {
      if (i >= 0) a = x[i];
      if (i + 1 >= 0 && i + 1 < n) b = x[i + 1];
      if (i + 2 >= 0 && i + 2 < n) c = x[i + 2];
      if (i + 3 >= 0 && i + 3 < n) d = x[i + 3];
    }
    quad[q] = ((a * a + b * b) + c * c) + d * d;
  }
  __syncthreads();
  for (int j = tid; j < SEG_BLOCKS; j += SEG_T) {
    float s = quad[10 * j];
#pragma unroll
    for (int k = 1; k < 10; ++k) s += quad[10 * j + k];
    blk[j] = s;
  }
  __syncthreads();
  if (tid < SEG_TP && p0 + tid <= T) {
    float s = blk[4 * tid];
#pragma unroll
    for (int k = 1; k < 10; ++k) s += blk[4 * tid + k];
    pw[(long)r * ld + p0 + tid] = s / (float)TA_CUT_POWER_WINDOW;
  }
  float v = blk[5 + 2 * tid] + blk[5 + 2 * tid + 1];     // the tile's own samples start at block 5 of the staged range
  v = wave_sum(v);
  if ((tid & 63) == 0) wsum[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) partial[(long)r * ntl + blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

__global__ __launch_bounds__(SEG_T) void cut_total_kernel(const long* __restrict__ offsets, long max_n, const float* __restrict__ partial,
                                                          long ntl, float cut_penalty, float* __restrict__ pen) {
  __shared__ float wsum[SEG_T / 64];
  const int r = blockIdx.x, tid = threadIdx.x;
  const long n = offsets[r + 1] - offsets[r];
  if (n <= 0 || n > max_n) return;
  const long nt = seg_positions(n) / SEG_TP + 1;          // tiles 0 .. T / 128 hold positions 0 .. T
  float v = 0.f;
  for (long t = tid; t < nt; t += SEG_T) v += partial[(long)r * ntl + t];
  v = wave_sum(v);
  if ((tid & 63) == 0) wsum[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) {
    const float tot = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    pen[r] = cut_penalty * (float)((double)tot / (double)n);
  }
}

__global__ __launch_bounds__(SEG_T) void cut_smooth_kernel(const long* __restrict__ offsets, long max_n, const float* __restrict__ pw,
                                                           const float* __restrict__ pen, int h, float* __restrict__ cost, long ld) {
  const int r = blockIdx.y;
  const long n = offsets[r + 1] - offsets[r];
  if (n <= 0 || n > max_n) return;
  const long T = seg_positions(n);
  const long p = (long)blockIdx.x * SEG_T + threadIdx.x;
  if (p > T) return;
  const float* w = pw + (long)r * ld;
  const long lo = p - h > 0 ? p - h : 0, hi = p + h < T ? p + h : T;
  float s = w[lo];
  for (long q = lo + 1; q <= hi; ++q) s += w[q];
  cost[(long)r * ld + p] = s / (float)(2 * h + 1) + pen[r];
}

// ---------------------------------------------------------------------------------------------------------------- the plan
__global__ __launch_bounds__(SEG_PT) void cut_plan_kernel(const float* __restrict__ cost, long ld, const long* __restrict__ offsets,
                                                         long max_n, int min_len, int max_len, int* __restrict__ back,
                                                         int* __restrict__ cuts, long ldc, int* __restrict__ n_seg,
                                                         float* __restrict__ dp_T) {
  __shared__ float ring[SEG_RING_MAX];
  __shared__ float cmin[SEG_RING_MAX / SEG_CH];
  __shared__ int cidx[SEG_RING_MAX / SEG_CH];
  const int r = blockIdx.x, tid = threadIdx.x;
  const long n = offsets[r + 1] - offsets[r];
  if (n <= 0 || n > max_n) {                              // refused (uniform): no plan
    if (tid == 0) { n_seg[r] = -1; dp_T[r] = INFINITY; }
    return;
  }
  const int T = (int)seg_positions(n);                    // <= TA_CUT_MAX_POSITIONS: the host checked max_n
  const int RING = (max_len + min_len + SEG_CH - 1) / SEG_CH * SEG_CH, NCH = RING / SEG_CH;
  const float* c = cost + (long)r * ld;
  int* bk = back + (long)r * ld;
  if (tid == 0) { ring[0] = 0.f; bk[0] = -1; }
  int done = 0;                                           // chunks whose pair exists
  const bool pairs = max_len - min_len + 1 >= SEG_CH;     // a narrower window never holds a whole chunk
  __syncthreads();
  const int nblk = (T + min_len - 1) / min_len;
  for (int b = 0; b < nblk; ++b) {
    const int base = b * min_len;
    const int end = base + min_len < T ? base + min_len : T;
    for (int p = base + 1 + tid; p <= end; p += SEG_PT) {
      const int lo = p - max_len > 0 ? p - max_len : 0, hi = p - min_len;
      float best = INFINITY;
      int bi = -1;
      if (hi >= 0) {
        const int cl = lo >> 6, ch = hi >> 6;
        const int e1 = cl == ch ? hi : (cl << 6) + SEG_CH - 1;
        int slot = lo % RING;
        best = ring[slot];
        bi = lo;
        for (int s = lo + 1; s <= e1; ++s) {
          slot = slot + 1 == RING ? 0 : slot + 1;
          const float v = ring[slot];
          if (v < best) { best = v; bi = s; }
        }
        if (cl != ch) {
          int cs = (cl + 1) % NCH;
          for (int k = cl + 1; k < ch; ++k) {
            const float v = cmin[cs];
            if (v < best) { best = v; bi = cidx[cs]; }
            cs = cs + 1 == NCH ? 0 : cs + 1;
          }
          slot = (ch << 6) % RING;
          for (int s = ch << 6; s <= hi; ++s) {
            const float v = ring[slot];
            if (v < best) { best = v; bi = s; }
            slot = slot + 1 == RING ? 0 : slot + 1;
          }
        }
      }
      ring[p % RING] = (p < T ? c[p] : 0.f) + best;
      bk[p] = bi;
    }
    __syncthreads();
    const int full = pairs ? (end + 1) >> 6 : 0;          // chunks that lie entirely in 0 .. end
    for (int k = done + (tid >> 6); k < full; k += SEG_PT / 64) {       // a wave per chunk: k is uniform over the wave
      float best = ring[(k << 6) % RING + (tid & 63)];     // RING is a multiple of 64: a chunk never wraps
      int bi = (k << 6) + (tid & 63);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov < best || (ov == best && oi < bi)) { best = ov; bi = oi; }
      }
      if ((tid & 63) == 0) { cmin[k % NCH] = best; cidx[k % NCH] = bi; }
    }
    done = full;
    __syncthreads();
  }
  if (tid != 0) return;
  // back[] was written by this workgroup before the barriers above
  if (T < min_len) {                                      // too short to cut: the one window [0, T]
    cuts[(long)r * ldc] = 0;
    if (ldc > 1) cuts[(long)r * ldc + 1] = T;
    n_seg[r] = 1;
    dp_T[r] = 0.f;
    return;
  }
  dp_T[r] = ring[T % RING];
  const int max_seg = T / min_len;
  int ns = 0, p = T;
  bool ok = true;
  for (int k = 0; k <= max_seg && p > 0; ++k) {
    const int s = bk[p];
    if (s < 0 || s >= p) { ok = false; break; }
    p = s;
    ++ns;
  }
  if (!ok || p != 0 || ns >= ldc) { n_seg[r] = -1; return; }        // only with non-finite costs, or a table too small
  p = T;
  for (int k = ns; k > 0; --k) {
    cuts[(long)r * ldc + k] = p;
    p = bk[p];
  }
  cuts[(long)r * ldc] = 0;
  n_seg[r] = ns;
}

// ---------------------------------------------------------------------------------------------------------------- the gather
template <bool VEC>
__global__ __launch_bounds__(SEG_T) void wave_windows_kernel(const float* __restrict__ wav, long total, const long* __restrict__ start,
                                                             const int* __restrict__ len, int Ls, float* __restrict__ out,
                                                             long* __restrict__ lens) {
  const int w = blockIdx.y;
  const long st = start[w];
  int L = len[w];
  L = L < 0 ? 0 : (L > Ls ? Ls : L);
  if (blockIdx.x == 0 && threadIdx.x == 0) lens[w] = L;
  const long j = ((long)blockIdx.x * SEG_T + threadIdx.x) * 4;       // first column of this lane's quad
  if (j >= Ls) return;
  const long src = st + j;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (j + 4 <= L && src >= 0 && src + 4 <= total && ((((uintptr_t)(wav + src)) & 15) == 0)) {
    const float4 q = *(const float4*)(wav + src);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (j + k < L && src + k >= 0 && src + k < total) v[k] = wav[src + k];
  }
  float* o = out + (long)w * Ls + j;
  if (VEC) {
    *(float4*)o = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (j + k < Ls) o[k] = v[k];
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
namespace {
struct CutCostWs {
  long ld, ntl, pw_floats, partial_floats, total;
};
bool cut_max_n_ok(long max_n) { return max_n >= 1 && (max_n + TA_CUT_HOP - 1) / TA_CUT_HOP <= TA_CUT_MAX_POSITIONS; }
CutCostWs cut_cost_ws(int R, long max_n) {
  CutCostWs w;
  const long T = (max_n + TA_CUT_HOP - 1) / TA_CUT_HOP;
  w.ld = T + 1;
  w.ntl = T / SEG_TP + 1;
  w.pw_floats = (long)R * w.ld;
  w.partial_floats = (long)R * w.ntl;
  w.total = (w.pw_floats + w.partial_floats + R) * 4;
  return w;
}
}  // namespace

extern "C" long ta_wave_cut_cost_workspace_bytes(int R, long max_n) {
  if (R <= 0 || R > TA_CUT_MAX_RECORDINGS || !cut_max_n_ok(max_n)) return 0;
  return cut_cost_ws(R, max_n).total;
}

extern "C" int ta_wave_cut_cost_f32(const float* wav, const long* offsets, int R, long max_n, int h, float cut_penalty, float* cost,
                                    long ld, void* ws, long ws_bytes, hipStream_t st) {
  if (R < 0 || R > TA_CUT_MAX_RECORDINGS || h < 0 || h > TA_CUT_MAX_SMOOTH || !(cut_penalty >= 0.f) || !(cut_penalty < INFINITY))
    return TA_ERR_ARG;
  if (R == 0) return TA_OK;
  if (!cut_max_n_ok(max_n) || !wav || !offsets || !cost) return TA_ERR_ARG;
  const CutCostWs w = cut_cost_ws(R, max_n);
  if (ld < w.ld || !ws || ws_bytes < w.total) return TA_ERR_ARG;
  float* pw = (float*)ws;
  float* partial = pw + w.pw_floats;
  float* pen = partial + w.partial_floats;
  TA_LAUNCH(cut_power_kernel, dim3((unsigned)w.ntl, R), dim3(SEG_T), 0, st, wav, offsets, max_n, pw, w.ld, partial, w.ntl);
  TA_CHECK_LAUNCH();
  TA_LAUNCH(cut_total_kernel, dim3(R), dim3(SEG_T), 0, st, offsets, max_n, partial, w.ntl, cut_penalty, pen);
  TA_CHECK_LAUNCH();
  TA_LAUNCH(cut_smooth_kernel, dim3((unsigned)((w.ld + SEG_T - 1) / SEG_T), R), dim3(SEG_T), 0, st, offsets, max_n, pw, pen, h, cost, ld);
  TA_CHECK_LAUNCH();
  return TA_OK;
}

extern "C" int ta_cut_plan_f32(const float* cost, long ld, const long* offsets, int R, long max_n, int min_len, int max_len, int* back,
                               int* cuts, long ldc, int* n_seg, float* dp_T, hipStream_t st) {
  if (R < 0 || R > TA_CUT_MAX_RECORDINGS || min_len < 1 || max_len > TA_CUT_MAX_LEN || 2L * min_len > max_len) return TA_ERR_ARG;
  if (R == 0) return TA_OK;
  if (!cut_max_n_ok(max_n) || !cost || !offsets || !back || !cuts || !n_seg || !dp_T) return TA_ERR_ARG;
  const long T = (max_n + TA_CUT_HOP - 1) / TA_CUT_HOP;
  if (ld < T + 1 || ldc < T / min_len + 2 || T / min_len > TA_CUT_MAX_BLOCKS) return TA_ERR_ARG;
  TA_LAUNCH(cut_plan_kernel, dim3(R), dim3(SEG_PT), 0, st, cost, ld, offsets, max_n, min_len, max_len, back, cuts, ldc, n_seg, dp_T);
  TA_CHECK_LAUNCH();
  return TA_OK;
}

extern "C" int ta_wave_windows_f32(const float* wav, long total, const long* start, const int* len, int W, int Ls, float* out, long* lens,
                                   hipStream_t st) {
  if (W < 0 || W > TA_WAVE_WINDOWS_MAX || Ls < 1 || total < 0) return TA_ERR_ARG;
  if (W == 0) return TA_OK;
  if (!wav || !start || !len || !out || !lens) return TA_ERR_ARG;
  const dim3 grid((unsigned)(((long)Ls + 4 * SEG_T - 1) / (4 * SEG_T)), W);
  if (Ls % 4 == 0 && (((uintptr_t)out) & 15) == 0)
    TA_LAUNCH(wave_windows_kernel<true>, grid, dim3(SEG_T), 0, st, wav, total, start, len, Ls, out, lens);
  else
    TA_LAUNCH(wave_windows_kernel<false>, grid, dim3(SEG_T), 0, st, wav, total, start, len, Ls, out, lens);
  TA_CHECK_LAUNCH();
  return TA_OK;
}
