// ta355 forced alignment: the Viterbi trellis of CTC emissions against a token sequence and its backtrack, for word timestamps
// (replaces ForcedAligner._get_trellis / _backtrack, tiny_audio/alignment.py:47-152, a Python double loop over frames x tokens).
// The semantics are defined by tests/align_ref.py (a literal float32 loop).
//
// One workgroup of TA_ALIGN_THREADS = 256 threads (4 waves) per clip.  With cols = J + 1 trellis columns:
//   * thread i owns columns i, i + 256, ... (K = ceil(cols / 256) of them; K is the same for every thread of the workgroup);
//   * the previous and the next trellis row live in LDS (ping-pong), so a frame costs ONE barrier;
//   * the emissions a frame needs -- emission[t, blank] and the gathered emission[t, tokens[j - 1]] -- are staged into LDS for a
//     block of FB = min(TA_ALIGN_FRAME_BLOCK, AL_STAGE / cols) frames at a time: FB * cols independent loads, all in flight
//     together, instead of one dependent global load per frame.  Any C works the same way (the gather never reads a whole row);
//   * trellis[t + 1, j] = max(trellis[t, j] + e[t, blank], trellis[t, j - 1] + e[t, tokens[j - 1]]): one f32 add per candidate,
//     nothing else rounds, so the result is the reference's bit for bit;
//   * the decision bit of cell (t + 1, j), "move >= stay" (ties go to move), is what the backtrack would recompute from exactly
//     these two sums.  A wave's 64 bits are one ballot = one aligned 64-bit word of the workspace, bits[n][t][j >> 6] bit j & 63
//     (clip n owns max_T frames of ceil((max_J + 1) / 64) words);
//   * wave 0 then walks the bits back from (T, J).  In 64 frames j falls by at most 64, so the walk needs at most two words per
//     frame: lane l loads both for frame t - 1 - l (64 independent loads), then the 64 steps run on lane-broadcast registers.
//
// Barrier safety: every loop that holds a barrier is bounded by T, J or FB of the clip, which are workgroup-uniform; columns past
// J are predicated off, never skipped; the three early exits (clip outside the declared maxima, token id outside [0, C), failed
// alignment) are taken by the whole workgroup or, for the last one, after the final barrier.
//
// LDS: 2 rows + the column-index row (3 x 2052 x 4 B) + the stage (32 KB) = 56.6 KB per workgroup.
#include "common.h"
#include "../../include/ta355.h"

#define AL_T TA_ALIGN_THREADS
#define AL_COLS (TA_ALIGN_MAX_TOKENS + 4)     // J + 1 <= 2049, padded
#define AL_STAGE TA_ALIGN_STAGE_FLOATS        // 8192 floats of staged emissions: FB = min(64, 8192 / cols) >= 3 frames

static_assert(AL_T % 64 == 0, "a wave's ballot must be one aligned word of decision bits");
static_assert(AL_STAGE / (TA_ALIGN_MAX_TOKENS + 1) >= 1, "the stage holds at least one frame of the widest clip");

__global__ __launch_bounds__(AL_T) void ctc_align_kernel(const float* __restrict__ em, long ld, int C, const int* __restrict__ cu_frames,
                                                         const int* __restrict__ tokens, const int* __restrict__ cu_tokens, int blank,
                                                         int max_T, int max_J, int* __restrict__ frames, float* __restrict__ score,
                                                         int* __restrict__ status, unsigned long long* __restrict__ bits,
                                                         float* __restrict__ trellis, const long* __restrict__ trellis_off) {
  __shared__ float row[2][AL_COLS];
  __shared__ int colidx[AL_COLS];
  __shared__ float stage[AL_STAGE];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int f0 = cu_frames[n], k0 = cu_tokens[n];
  const int T = cu_frames[n + 1] - f0, J = cu_tokens[n + 1] - k0;
  if (T < 0 || J < 0 || T > max_T || J > max_J) {        // the caller's maxima size the workspace: never run past them
    if (tid == 0) { status[n] = 2; score[n] = -INFINITY; }
    return;
  }
  const int cols = J + 1, K = (cols + AL_T - 1) / AL_T;
  const int W = (max_J >> 6) + 1;                         // words per frame of the workspace, the same for every clip
  const float NEG = -INFINITY;

  int bad = 0;
  for (int c = tid; c < cols; c += AL_T) {
    const int id = c == 0 ? blank : tokens[k0 + c - 1];
    bad |= (id < 0 || id >= C);
    colidx[c] = id;
    row[0][c] = c == 0 ? 0.f : NEG;
  }
  if (__syncthreads_or(bad)) {
    if (tid == 0) { status[n] = 2; score[n] = -INFINITY; }
    return;
  }
  float* tr = trellis ? trellis + trellis_off[n] : nullptr;
  if (tr)
    for (int c = tid; c < cols; c += AL_T) tr[c] = c == 0 ? 0.f : NEG;
  unsigned long long* wbits = bits + (long)n * max_T * W;      // T <= max_T: inside the workspace whatever the other clips hold
  const float* e0 = em + (long)f0 * ld;

  int FB = AL_STAGE / cols;
  FB = FB > TA_ALIGN_FRAME_BLOCK ? TA_ALIGN_FRAME_BLOCK : FB;
  int cur = 0;
  for (int t0 = 0; t0 < T; t0 += FB) {
    const int nf = T - t0 < FB ? T - t0 : FB;
    // the previous block's last barrier has retired every read of the stage
    for (int f = 0; f < nf; ++f) {
      const float* er = e0 + (long)(t0 + f) * ld;
      for (int c = tid; c < cols; c += AL_T) stage[f * cols + c] = er[colidx[c]];
    }
    __syncthreads();
    for (int f = 0; f < nf; ++f) {
      const float* g = stage + f * cols;
      const float* rc = row[cur];
      float* rn = row[cur ^ 1];
      const float eb = g[0];
      const int t = t0 + f;
      for (int k = 0; k < K; ++k) {
        const int c = tid + k * AL_T;
        const bool valid = c < cols;
        float stay = NEG, move = NEG;
        if (valid) {
          stay = rc[c] + eb;
          if (c > 0) move = rc[c - 1] + g[c];
        }
        const bool take = valid && c > 0 && move >= stay;
        const unsigned long long m = __ballot(take);
        if (valid) {
          const float v = move > stay ? move : stay;       // Python's max(stay, move)
          rn[c] = v;
          if (tr) tr[(long)(t + 1) * cols + c] = v;
          if (lane == 0) wbits[(long)t * W + (c >> 6)] = m;
        }
      }
      __syncthreads();
      cur ^= 1;
    }
  }
  // after the last barrier: row[cur] is trellis[T, :], and every decision word of this clip is visible to the workgroup
  const float sc = row[cur][J];
  const bool ok = !(sc == NEG);
  if (tid == 0) { score[n] = sc; status[n] = ok ? 0 : 1; }
  if (!ok || J == 0 || tid >= 64) return;

  int t = T, j = J;
  while (t > 0 && j > 0) {
    const int wi = j >> 6, tf = t - 1 - lane;
    unsigned long long hi = 0, lo = 0;
    if (tf >= 0) {
      hi = wbits[(long)tf * W + wi];
      if (wi > 0) lo = wbits[(long)tf * W + wi - 1];
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

extern "C" long ta_ctc_align_workspace_bytes(int N, int max_T, int max_J) {
  if (N <= 0 || max_T <= 0 || max_J < 0) return 0;
  return (long)N * max_T * ((max_J >> 6) + 1) * 8;
}

extern "C" int ta_ctc_align_f32(const float* emission, long ld, int C, const int* cu_frames, const int* tokens, const int* cu_tokens,
                                int N, int max_T, int max_J, int blank_id, int* frames, float* score, int* status, void* ws,
                                long ws_bytes, float* trellis_out, const long* trellis_off, hipStream_t st) {
  if (N < 0 || N > TA_ALIGN_MAX_CLIPS || max_T < 0 || max_T > TA_ALIGN_MAX_FRAMES || max_J < 0 || max_J > TA_ALIGN_MAX_TOKENS)
    return TA_ERR_ARG;
  if (C < 1 || C > TA_ALIGN_MAX_CLASSES || ld < C || blank_id < 0 || blank_id >= C) return TA_ERR_ARG;
  if (N == 0) return TA_OK;
  if (!cu_frames || !cu_tokens || !score || !status) return TA_ERR_ARG;
  if (max_T > 0 && !emission) return TA_ERR_ARG;
  if (max_J > 0 && (!tokens || !frames)) return TA_ERR_ARG;
  if (trellis_out && !trellis_off) return TA_ERR_ARG;
  const long need = ta_ctc_align_workspace_bytes(N, max_T, max_J);
  if (ws_bytes < need || (need > 0 && !ws)) return TA_ERR_ARG;
  TA_LAUNCH(ctc_align_kernel, dim3(N), dim3(AL_T), 0, st, emission, ld, C, cu_frames, tokens, cu_tokens, blank_id, max_T, max_J, frames,
            score, status, (unsigned long long*)ws, trellis_out, trellis_off);
  TA_CHECK_LAUNCH();
  return TA_OK;
}
