// ta355 forced alignment, long form: the trellis of align.hip for transcripts and recordings beyond one workgroup's reach
// (ta_ctc_align_long_f32: up to 262 144 tokens against 1 048 576 frames), as a tiled wavefront over launches.  Same contract as
// ta_ctc_align_f32, defined by tests/align_ref.py: the same f32 recurrence (one f32 add per candidate, nothing else rounds), ties
// go to `move`, the same status 0 / 1 / 2, the same frames and score -- the reference's bytes, and inside the old envelope the
// short kernel's bytes.
//
// With cols = J + 1 trellis columns, a clip's trellis is cut into tiles of CB = col_block columns by FB = frame_block frames.  Tile
// (cb, fb) updates the cells (t + 1, j) for t in [fb FB, fb FB + FB) and j in [cb CB, cb CB + CB), and needs
//   * the row that enters it, trellis[fb FB, its columns]: the leaving row of tile (cb, fb - 1), or the initial row for fb = 0;
//   * for each of its frames t the value trellis[t, cb CB - 1] of the column to its left: what tile (cb - 1, fb) saw in its last
//     column at the rows BEFORE each update (the entering row's last element included).
// Both carries go through the workspace: rowc[n][cb][CB] is read at the start of a tile and overwritten at its end by the same
// workgroup; colc[n][cb][t] is indexed by the frame, so that tile (cb - 1, fb + 1), which writes it, and tile (cb, fb), which reads
// it in the same launch, touch disjoint ranges.  Launch k runs every tile with cb + fb == k of every clip, one workgroup of
// TA_ALIGN_THREADS threads per tile: nCB + nFB - 1 launches on the one stream carry all dependencies (kernel boundaries order the
// carries; no tile is skipped, so every carry a tile reads was written by the launch before).
//
// Inside a tile the body is align.hip's: thread i owns the tile's columns i, i + 256, ...; the previous and the next row live in LDS
// (ping-pong), one barrier per frame; the emissions are staged in LDS for SF = min(64, 8192 / (tile columns + 1)) frames at a time
// (e[t, blank], the gather e[t, tokens[j - 1]] of this tile's columns only, and the left column's values of those frames); a wave's
// 64 decision bits are one ballot = one aligned 64-bit word bits[n][t][j >> 6] (CB is a multiple of 64, so a word never straddles
// two tiles).  A first launch checks every clip (lengths against the declared maxima, token ids against [0, C)) and leaves a flag
// per clip in the workspace; a last launch walks the bits back with one wave per clip, 64 frames per iteration, as align.hip's wave 0.
//
// Barrier safety: no kernel waits for another workgroup -- no flags that are spun on, no grid barrier; the per-clip flag is written
// by an EARLIER launch.  Every loop that holds a barrier is bounded by the tile's frame and column counts, which are
// workgroup-uniform; columns past the tile are predicated off, never skipped; every early exit (tile outside the clip, refused
// clip) is taken by the whole workgroup before the first barrier.
//
// LDS of the tile kernel: 2 rows + the column-index row (3 x 2048 x 4 B) + the stage (32 KB) + 64 left values = 56.3 KB.
#include "common.h"
#include "../../include/ta355.h"

#define ALL_T TA_ALIGN_THREADS
#define ALL_CB TA_ALIGN_LONG_MAX_COL_BLOCK
#define ALL_STAGE TA_ALIGN_STAGE_FLOATS
#define ALL_SF TA_ALIGN_FRAME_BLOCK            // frames staged at a time, at most

static_assert(ALL_T % 64 == 0, "a wave's ballot must be one aligned word of decision bits");
static_assert(ALL_CB % 64 == 0 && TA_ALIGN_LONG_COL_BLOCK % 64 == 0 && TA_ALIGN_LONG_COL_BLOCK <= ALL_CB, "tiles are whole words");
static_assert(ALL_STAGE / (ALL_CB + 1) >= 1, "the stage holds at least one frame of the widest tile");
static_assert(ALL_SF <= ALL_T, "one thread per staged left value");

// the workspace: bits[N][max_T][W] words, then rowc[N][nCB][CB], colc[N][nCB][max_T] floats, then flags[N] ints
struct AlignLongWs {
  long W, nCB, bits_bytes, rowc_floats, colc_floats, total;
};
static AlignLongWs align_long_ws(int N, int max_T, int max_J, int CB) {
  AlignLongWs w;
  w.W = (max_J >> 6) + 1;
  w.nCB = ((long)max_J + CB) / CB;                        // ceil((max_J + 1) / CB)
  w.bits_bytes = (long)N * max_T * w.W * 8;
  w.rowc_floats = (long)N * w.nCB * CB;
  w.colc_floats = (long)N * w.nCB * max_T;
  w.total = w.bits_bytes + (w.rowc_floats + w.colc_floats) * 4 + (((long)N * 4 + 7) & ~7L);
  return w;
}

// one workgroup per clip: refuse what ta_ctc_align_f32 refuses, leave the verdict in flags[n] for the later launches, write the
// trellis's row 0, and settle the clips that have no tile (T = 0)
__global__ __launch_bounds__(ALL_T) void ctc_align_long_prep_kernel(int C, const int* __restrict__ cu_frames, const int* __restrict__ tokens,
                                                                    const int* __restrict__ cu_tokens, int max_T, int max_J,
                                                                    float* __restrict__ score, int* __restrict__ status,
                                                                    int* __restrict__ flags, float* __restrict__ trellis,
                                                                    const long* __restrict__ trellis_off) {
  const int n = blockIdx.x, tid = threadIdx.x;
  const int f0 = cu_frames[n], k0 = cu_tokens[n];
  const int T = cu_frames[n + 1] - f0, J = cu_tokens[n + 1] - k0;
  int bad = T < 0 || J < 0 || T > max_T || J > max_J;     // the caller's maxima size the workspace: never run past them
  if (!bad)
    for (int c = tid; c < J; c += ALL_T) {
      const int id = tokens[k0 + c];
      bad |= (id < 0 || id >= C);
    }
  bad = __syncthreads_or(bad);
  if (tid == 0) {
    flags[n] = bad;
    if (bad) { status[n] = 2; score[n] = -INFINITY; }
    else if (T == 0) { status[n] = J == 0 ? 0 : 1; score[n] = J == 0 ? 0.f : -INFINITY; }
  }
  if (bad || !trellis) return;
  float* tr = trellis + trellis_off[n];
  for (int c = tid; c <= J; c += ALL_T) tr[c] = c == 0 ? 0.f : -INFINITY;
}

__global__ __launch_bounds__(ALL_T) void ctc_align_long_tile_kernel(const float* __restrict__ em, long ld, const int* __restrict__ cu_frames,
                                                                    const int* __restrict__ tokens, const int* __restrict__ cu_tokens,
                                                                    int blank, int max_T, int max_J, int CB, int FB, int k, int cb_lo,
                                                                    float* __restrict__ score, int* __restrict__ status,
                                                                    unsigned long long* __restrict__ bits, float* __restrict__ rowc,
                                                                    float* __restrict__ colc, const int* __restrict__ flags,
                                                                    float* __restrict__ trellis, const long* __restrict__ trellis_off) {
  __shared__ float row[2][ALL_CB];
  __shared__ int colidx[ALL_CB];
  __shared__ float stage[ALL_STAGE];
  __shared__ float left[ALL_SF];
  const int n = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int cb = cb_lo + blockIdx.x, fb = k - cb;
  if (fb < 0 || flags[n]) return;
  const int f0 = cu_frames[n], k0 = cu_tokens[n];
  const int T = cu_frames[n + 1] - f0, J = cu_tokens[n + 1] - k0;
  const int cols = J + 1;
  const int c0 = cb * CB;                                 // cb <= max_J / CB: no overflow
  const long t0 = (long)fb * FB;
  if (c0 >= cols || t0 >= T) return;                      // no such tile in this clip
  const int nc = cols - c0 < CB ? cols - c0 : CB;         // columns and frames of this tile
  const int nft = T - t0 < FB ? (int)(T - t0) : FB;
  const int K = (nc + ALL_T - 1) / ALL_T;
  const long W = (max_J >> 6) + 1, nCB = ((long)max_J + CB) / CB;      // the workspace's geometry: the same for every clip
  const float NEG = -INFINITY;

  float* rc_g = rowc + ((long)n * nCB + cb) * CB;
  const float* lc_g = cb > 0 ? colc + ((long)n * nCB + cb - 1) * max_T : nullptr;     // the left neighbour's last column
  float* wc_g = c0 + CB < cols ? colc + ((long)n * nCB + cb) * max_T : nullptr;        // ours, when a tile to the right reads it
  for (int c = tid; c < nc; c += ALL_T) {
    const int g = c0 + c;
    colidx[c] = g == 0 ? blank : tokens[k0 + g - 1];
    row[0][c] = fb == 0 ? (g == 0 ? 0.f : NEG) : rc_g[c];
  }
  float* tr = trellis ? trellis + trellis_off[n] : nullptr;
  unsigned long long* wbits = bits + (long)n * max_T * W;
  const float* e0 = em + (long)f0 * ld;

  const int SW = nc + 1;                                  // a staged frame: e[t, blank], then the gather of the tile's columns
  int SF = ALL_STAGE / SW;
  SF = SF > ALL_SF ? ALL_SF : SF;
  int cur = 0;
  for (int ts = 0; ts < nft; ts += SF) {
    const int nf = nft - ts < SF ? nft - ts : SF;
    // the previous block's last barrier has retired every read of the stage and of the left values
    for (int f = 0; f < nf; ++f) {
      const float* er = e0 + (t0 + ts + f) * ld;
      for (int c = tid; c < nc; c += ALL_T) stage[f * SW + 1 + c] = er[colidx[c]];
      if (tid == 0) stage[f * SW] = er[blank];
    }
    if (lc_g && tid < nf) left[tid] = lc_g[t0 + ts + tid];
    __syncthreads();
    for (int f = 0; f < nf; ++f) {
      const float* g = stage + f * SW;
      const float* rc = row[cur];
      float* rn = row[cur ^ 1];
      const float eb = g[0];
      const long t = t0 + ts + f;
      if (wc_g && tid == 0) wc_g[t] = rc[nc - 1];         // trellis[t, our last column], before this frame's update
      for (int kk = 0; kk < K; ++kk) {
        const int c = tid + kk * ALL_T, gc = c0 + c;
        const bool valid = c < nc;
        float stay = NEG, move = NEG;
        if (valid) {
          stay = rc[c] + eb;
          if (gc > 0) move = (c > 0 ? rc[c - 1] : left[f]) + g[1 + c];
        }
        const bool take = valid && gc > 0 && move >= stay;
        const unsigned long long m = __ballot(take);
        if (valid) {
          const float v = move > stay ? move : stay;       // Python's max(stay, move)
          rn[c] = v;
          if (tr) tr[(t + 1) * cols + gc] = v;
          if (lane == 0) wbits[t * W + (gc >> 6)] = m;
        }
      }
      __syncthreads();
      cur ^= 1;
    }
  }
  // after the last barrier: row[cur] is trellis[t0 + nft, this tile's columns]
  if (t0 + nft < T) {
    for (int c = tid; c < nc; c += ALL_T) rc_g[c] = row[cur][c];
  } else if (c0 + nc == cols && tid == 0) {               // the tile that holds trellis[T, J]
    const float sc = row[cur][nc - 1];
    score[n] = sc;
    status[n] = sc == NEG ? 1 : 0;
  }
}

// one wave per clip: align.hip's walk.  In 64 frames j falls by at most 64, so the walk needs at most two words per frame: lane l
// loads both for frame t - 1 - l (64 independent loads), then the 64 steps run on lane-broadcast registers.
__global__ __launch_bounds__(64) void ctc_align_long_backtrack_kernel(const int* __restrict__ cu_frames, const int* __restrict__ cu_tokens,
                                                                      int max_T, int max_J, int* __restrict__ frames,
                                                                      const int* __restrict__ status,
                                                                      const unsigned long long* __restrict__ bits,
                                                                      const int* __restrict__ flags) {
  const int n = blockIdx.x, lane = threadIdx.x;
  if (flags[n] || status[n] != 0) return;
  const int k0 = cu_tokens[n];
  const int T = cu_frames[n + 1] - cu_frames[n], J = cu_tokens[n + 1] - k0;
  const long W = (max_J >> 6) + 1;
  const unsigned long long* wbits = bits + (long)n * max_T * W;
  int t = T, j = J;
  while (t > 0 && j > 0) {
    const int wi = j >> 6;
    const long tf = (long)t - 1 - lane;
    unsigned long long hi = 0, lo = 0;
    if (tf >= 0) {
      hi = wbits[tf * W + wi];
      if (wi > 0) lo = wbits[tf * W + wi - 1];
    }
    const int steps = t < 64 ? t : 64;
    for (int l = 0; l < steps && j > 0; ++l) {
      const unsigned long long h = __shfl(hi, l, 64), o = __shfl(lo, l, 64);
      const unsigned long long w = (j >> 6) == wi ? h : o;
      if ((w >> (j & 63)) & 1ull) {
        if (lane == 0) frames[k0 + j - 1] = t - 1 - l;
        --j;
      }
    }
    t -= steps;
  }
}

static bool align_long_tiling(int* col_block, int* frame_block) {
  if (*col_block == 0) *col_block = TA_ALIGN_LONG_COL_BLOCK;
  if (*frame_block == 0) *frame_block = TA_ALIGN_LONG_FRAME_BLOCK;
  return *col_block > 0 && *col_block % 64 == 0 && *col_block <= ALL_CB && *frame_block >= 1;
}

extern "C" long ta_ctc_align_long_workspace_bytes(int N, int max_T, int max_J, int col_block, int frame_block) {
  if (!align_long_tiling(&col_block, &frame_block)) return -1;
  if (N <= 0 || max_T < 0 || max_J < 0) return 0;
  return align_long_ws(N, max_T, max_J, col_block).total;
}

extern "C" int ta_ctc_align_long_f32(const float* emission, long ld, int C, const int* cu_frames, const int* tokens, const int* cu_tokens,
                                     int N, int max_T, int max_J, int blank_id, int col_block, int frame_block, int* frames,
                                     float* score, int* status, void* ws, long ws_bytes, float* trellis_out, const long* trellis_off,
                                     hipStream_t st) {
  if (N < 0 || N > TA_ALIGN_LONG_MAX_CLIPS || max_T < 0 || max_T > TA_ALIGN_LONG_MAX_FRAMES || max_J < 0 ||
      max_J > TA_ALIGN_LONG_MAX_TOKENS)
    return TA_ERR_ARG;
  if (C < 1 || C > TA_ALIGN_LONG_MAX_CLASSES || ld < C || blank_id < 0 || blank_id >= C) return TA_ERR_ARG;
  if (!align_long_tiling(&col_block, &frame_block)) return TA_ERR_ARG;
  if (N == 0) return TA_OK;
  if (!cu_frames || !cu_tokens || !score || !status) return TA_ERR_ARG;
  if (max_T > 0 && !emission) return TA_ERR_ARG;
  if (max_J > 0 && (!tokens || !frames)) return TA_ERR_ARG;
  if (trellis_out && !trellis_off) return TA_ERR_ARG;
  const AlignLongWs w = align_long_ws(N, max_T, max_J, col_block);
  if (ws_bytes < w.total || !ws) return TA_ERR_ARG;
  unsigned long long* bits = (unsigned long long*)ws;
  float* rowc = (float*)((char*)ws + w.bits_bytes);
  float* colc = rowc + w.rowc_floats;
  int* flags = (int*)(colc + w.colc_floats);

  TA_LAUNCH(ctc_align_long_prep_kernel, dim3(N), dim3(ALL_T), 0, st, C, cu_frames, tokens, cu_tokens, max_T, max_J, score, status, flags,
            trellis_out, trellis_off);
  TA_CHECK_LAUNCH();
  const long nCB = w.nCB, nFB = ((long)max_T + frame_block - 1) / frame_block;
  for (long k = 0; nFB > 0 && k < nCB + nFB - 1; ++k) {
    const long lo = k - (nFB - 1) > 0 ? k - (nFB - 1) : 0, hi = k < nCB - 1 ? k : nCB - 1;      // the column blocks alive in launch k
    TA_LAUNCH(ctc_align_long_tile_kernel, dim3((unsigned)(hi - lo + 1), N), dim3(ALL_T), 0, st, emission, ld, cu_frames, tokens,
              cu_tokens, blank_id, max_T, max_J, col_block, frame_block, (int)k, (int)lo, score, status, bits, rowc, colc, flags,
              trellis_out, trellis_off);
    TA_CHECK_LAUNCH();
  }
  if (max_J > 0 && max_T > 0) {
    TA_LAUNCH(ctc_align_long_backtrack_kernel, dim3(N), dim3(64), 0, st, cu_frames, cu_tokens, max_T, max_J, frames, status, bits, flags);
    TA_CHECK_LAUNCH();
  }
  return TA_OK;
}
