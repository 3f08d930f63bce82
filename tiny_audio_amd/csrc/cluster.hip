// ta355 -- spectral clustering of speaker embeddings on the device (include/ta355.h, "speaker clustering"): the O(N^2) / O(N^3) part
// of the reference's SpectralCluster (tiny_audio/diarization.py:49-106).  Everything is f32.
//
//   ta_spk_affinity_f32          E [N, D] -> pruned, symmetrised cosine affinity W [N, N] and its row sums deg [N]
//                                  1  rows normalised into the workspace (zero padded to a multiple of 16 columns);
//                                     S = E^ E^T: 64 x 64 tiles of the UPPER triangle, every tile also stored transposed, so
//                                     S[i, j] and S[j, i] are the same bits (inside a diagonal tile both are the same k-ordered
//                                     fmaf chain of commuting products)
//                                  2  per row: the keep-th largest value by bisection on the ordered-integer image of the row held
//                                     in LDS (the method of logits_warp_kernel, generate.hip), ties at the threshold kept lowest
//                                     column first, everything else zeroed in place
//                                  4  W = (P + P^T) / 2 in place over tile pairs, diagonal zeroed; deg = row sums in a fixed order
//   ta_spk_laplacian_matmul_f32  Y = diag(deg) X - W X, X [N, p <= 32]: one streaming pass over W on the f32 MFMA (16 rows x 16
//                                columns of Y per wave, 16 B of W per lane and step), the columns of W split over workgroups so that
//                                a 16-column block fills the GPU; the splits' partial sums are added in split order by a second kernel
//   ta_spk_panel_gram_f32        C = A^T B     rows split over workgroups, partial sums added in split order
//   ta_spk_panel_update_f32      B -= A C      one fixed k order
//   ta_spk_panel_combine_f32     Y = V Z
// No floating-point atomics anywhere: the same inputs give the same bits.  Every loop has a fixed trip count; no kernel waits on
// another workgroup.
#include "common.h"
#include "../../include/ta355.h"

namespace {
constexpr int SPK_DP_MAX = TA_SPK_MAX_D;           // padded embedding width: D rounded up to 16
constexpr int LM_TARGET_BLOCKS = 2048;             // workgroups a product or a Gram launch aims for and the product stays under: 256
                                                   // CUs x 8 resident workgroups of 256 threads, so that no second round trails

inline int spk_dpad(int D) { return (D + 15) / 16 * 16; }

__device__ __forceinline__ int spk_ord(float f) { const int i = __float_as_int(f); return i >= 0 ? i : i ^ 0x7fffffff; }
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// sum over the 256 threads of a workgroup; red: 4 ints of LDS.  Every thread gets the total.
__device__ __forceinline__ int block_sum_i256(int v, int* red) {
  v = wave_sum_i(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// ---- 1. rows normalised: Eh [N, Dp] = E / |E| (a zero row stays zero, as sklearn's normalize has it), columns D .. Dp zero
__global__ __launch_bounds__(256) void spk_normalize_kernel(const float* __restrict__ E, float* __restrict__ Eh, int N, int D, int Dp) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= N) return;
  const float* e = E + (size_t)row * D;
  float v[SPK_DP_MAX / 64];
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < SPK_DP_MAX / 64; ++q) {
    const int c = lane + 64 * q;
    v[q] = c < D ? e[c] : 0.f;
    s = fmaf(v[q], v[q], s);
  }
  s = wave_sum(s);
  const float nrm = sqrtf(s);
#pragma unroll
  for (int q = 0; q < SPK_DP_MAX / 64; ++q) {
    const int c = lane + 64 * q;
    if (c < Dp) Eh[(size_t)row * Dp + c] = nrm > 0.f ? v[q] / nrm : v[q];
  }
}

// S = Eh Eh^T.  Grid (tiles, tiles), tiles below the diagonal return at once; 256 threads, a 4 x 4 micro-tile each.
__global__ __launch_bounds__(256) void spk_cosine_kernel(const float* __restrict__ Eh, int N, int Dp, float* __restrict__ S, size_t ld) {
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj < bi) return;
  __shared__ __align__(16) float As[16][64 + 4], Bs[16][64 + 4];
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int i0 = bi * 64, j0 = bj * 64;
  const int lr = tid >> 2, lk = (tid & 3) * 4;          // the staging load of this thread: row lr, k lk .. lk + 3
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (int k0 = 0; k0 < Dp; k0 += 16) {
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (i0 + lr < N) a = *(const float4*)(Eh + (size_t)(i0 + lr) * Dp + k0 + lk);
    if (j0 + lr < N) b = *(const float4*)(Eh + (size_t)(j0 + lr) * Dp + k0 + lk);
    __syncthreads();
    As[lk + 0][lr] = a.x; As[lk + 1][lr] = a.y; As[lk + 2][lr] = a.z; As[lk + 3][lr] = a.w;
    Bs[lk + 0][lr] = b.x; Bs[lk + 1][lr] = b.y; Bs[lk + 2][lr] = b.z; Bs[lk + 3][lr] = b.w;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const float4 av = *(const float4*)&As[k][ty * 4], bv = *(const float4*)&Bs[k][tx * 4];
      const float ar[4] = {av.x, av.y, av.z, av.w}, br[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(ar[i], br[j], acc[i][j]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = i0 + ty * 4 + i, c = j0 + tx * 4 + j;
      if (r < N && c < N) {
        S[(size_t)r * ld + c] = acc[i][j];
        if (bi != bj) S[(size_t)c * ld + r] = acc[i][j];
      }
    }
}

// ---- 2. one workgroup per row: keep the `keep` largest entries, ties at the threshold lowest column first; zero the rest
__global__ __launch_bounds__(256) void spk_prune_kernel(float* __restrict__ S, size_t ld, int N, int keep, int* __restrict__ kept_count) {
  extern __shared__ __align__(16) float spk_lds[];
  const int Np = (N + 3) & ~3;
  float* rowv = spk_lds;                             // [Np]
  int* tcnt = (int*)(spk_lds + Np);                  // [256] ties per thread chunk
  int* red = tcnt + 256;                             // [4]
  const int tid = threadIdx.x;
  float* row = S + (size_t)blockIdx.x * ld;
  for (int j = tid; j < N; j += 256) rowv[j] = row[j];
  __syncthreads();
  // the keep-th largest value = the largest ordered integer o with count(x >= o) >= keep: 32 halvings of the 2^32 images
  long lo = -2147483648L, hi = 2147483647L;
  for (int it = 0; it < 32; ++it) {
    const long mid = lo + (hi - lo + 1) / 2;
    int c = 0;
    for (int j = tid; j < N; j += 256) c += (long)spk_ord(rowv[j]) >= mid ? 1 : 0;
    c = block_sum_i256(c, red);
    if (lo < hi) { if (c >= keep) lo = mid; else hi = mid - 1; }
  }
  const int thr = (int)lo;
  int gt = 0;
  for (int j = tid; j < N; j += 256) gt += spk_ord(rowv[j]) > thr ? 1 : 0;
  gt = block_sum_i256(gt, red);
  const int need = keep - gt;                        // ties to keep (>= 1 by the definition of thr)
  // ties are ranked in column order: thread t owns the columns [t per, (t + 1) per)
  const int per = (N + 255) / 256, c0 = tid * per, c1 = min(N, c0 + per);
  int ties = 0;
  for (int j = c0; j < c1; ++j) ties += spk_ord(rowv[j]) == thr ? 1 : 0;
  tcnt[tid] = ties;
  __syncthreads();
  int rank = 0;
  for (int t = 0; t < tid; ++t) rank += tcnt[t];
  int kept = 0;
  for (int j = c0; j < c1; ++j) {
    const int o = spk_ord(rowv[j]);
    bool k = o > thr;
    if (o == thr) { k = rank < need; ++rank; }
    if (!k) rowv[j] = 0.f;
    kept += k ? 1 : 0;
  }
  kept = block_sum_i256(kept, red);                  // (its barriers also publish rowv)
  for (int j = tid; j < N; j += 256) row[j] = rowv[j];
  if (kept_count && tid == 0) kept_count[blockIdx.x] = kept;
}

// ---- 4. W = (P + P^T) / 2 in place, diagonal zero.  One workgroup per pair of 32 x 32 tiles (bi <= bj): both tiles are read into LDS
// before anything is written, and nobody else touches them.
__global__ __launch_bounds__(256) void spk_symmetrize_kernel(float* __restrict__ S, size_t ld, int N) {
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj < bi) return;
  __shared__ float As[32][33], Bs[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int i0 = bi * 32, j0 = bj * 32;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = ty + 8 * q;
    As[r][tx] = (i0 + r < N && j0 + tx < N) ? S[(size_t)(i0 + r) * ld + j0 + tx] : 0.f;
    Bs[r][tx] = (j0 + r < N && i0 + tx < N) ? S[(size_t)(j0 + r) * ld + i0 + tx] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = ty + 8 * q;
    const int i = i0 + r, j = j0 + tx;
    if (i < N && j < N) S[(size_t)i * ld + j] = i == j ? 0.f : 0.5f * (As[r][tx] + Bs[tx][r]);
    const int i2 = j0 + r, j2 = i0 + tx;                                      // the mirrored tile: the same sum, operands swapped
    if (bi != bj && i2 < N && j2 < N) S[(size_t)i2 * ld + j2] = 0.5f * (Bs[r][tx] + As[tx][r]);
  }
}

__global__ __launch_bounds__(256) void spk_rowsum_kernel(const float* __restrict__ W, size_t ld, int N, float* __restrict__ deg) {
  __shared__ float red[4];
  const float* row = W + (size_t)blockIdx.x * ld;
  float s = 0.f;
  for (int j = threadIdx.x; j < N; j += 256) s += row[j];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) deg[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- the Laplacian product.  Grid (row groups of 64, column splits); wave w of a workgroup owns the rows 64 g + 16 w .. + 15.  Per step
// of 16 columns lane l reads W[row l % 16][c0 + 4 (l / 16) .. + 3] (16 B) and issues four 16x16x4 MFMAs: MFMA q contracts the columns
// c0 + 4 kq + q (kq = 0 .. 3), so its B operand is X[c0 + 4 (l / 16) + q][l % 16].  CT column tiles of 16 share the A operand.
template <int CT>
__global__ __launch_bounds__(256) void spk_lapmul_kernel(const float* __restrict__ W, size_t ldw, const float* __restrict__ X, size_t ldx,
                                                        int N, int p, int chunk, float* __restrict__ part, int vec) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = (blockIdx.x * 4 + wave) * 16;
  if (r0 >= N) return;
  const int r = r0 + (lane & 15), kq = lane >> 4, jl = lane & 15;
  const bool rok = r < N;
  const float* wrow = W + (size_t)(rok ? r : 0) * ldw;
  const int cb = blockIdx.y * chunk, ce = min(N, cb + chunk);
  f32x4 acc[CT][2];
#pragma unroll
  for (int t = 0; t < CT; ++t) { acc[t][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[t][1] = acc[t][0]; }
  for (int c0 = cb; c0 < ce; c0 += 16) {
    const int c = c0 + 4 * kq;
    float a[4];
    if (vec && c + 3 < N) {
      const float4 v = *(const float4*)(wrow + c);
      a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) a[q] = c + q < N ? wrow[c + q] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float av = rok ? a[q] : 0.f;
#pragma unroll
      for (int t = 0; t < CT; ++t) {
        const int j = t * 16 + jl;
        const float bv = (c + q < N && j < p) ? X[(size_t)(c + q) * ldx + j] : 0.f;
        acc[t][q & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[t][q & 1], 0, 0, 0);
      }
    }
  }
  // D: lane l holds rows 4 (l / 16) + i, column l % 16
  float* out = part + (size_t)blockIdx.y * N * (CT * 16);
#pragma unroll
  for (int t = 0; t < CT; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rr = r0 + 4 * kq + i;
      if (rr < N) out[(size_t)rr * (CT * 16) + t * 16 + jl] = acc[t][0][i] + acc[t][1][i];
    }
}

__global__ __launch_bounds__(256) void spk_lapmul_reduce_kernel(const float* __restrict__ part, int nsplit, int pw, const float* __restrict__ deg,
                                                               const float* __restrict__ X, size_t ldx, float* __restrict__ Y, size_t ldy,
                                                               int N, int p) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)N * p) return;
  const int i = (int)(idx / p), j = (int)(idx % p);
  float t = 0.f;
  for (int s = 0; s < nsplit; ++s) t += part[((size_t)s * N + i) * pw + j];
  Y[(size_t)i * ldy + j] = deg[i] * X[(size_t)i * ldx + j] - t;
}

struct LapSplit { int groups, nsplit, chunk, pw; };
inline LapSplit lap_split(int N, int p) {
  LapSplit s;
  s.groups = (N + 63) / 64;
  int want = LM_TARGET_BLOCKS / s.groups;
  const int most = (N + 255) / 256;                  // a split streams at least 256 columns
  if (want > most) want = most;
  if (want < 1) want = 1;
  s.chunk = (((N + want - 1) / want) + 63) / 64 * 64;
  s.nsplit = (N + s.chunk - 1) / s.chunk;
  s.pw = p <= 16 ? 16 : 32;
  return s;
}

// ---- panel algebra.  C = A^T B: grid (a tiles of 32, b tiles of 32, row splits); a 2 x 2 micro-tile per thread.
__global__ __launch_bounds__(256) void spk_gram_kernel(const float* __restrict__ A, size_t lda, int a, const float* __restrict__ B, size_t ldb,
                                                      int b, int N, int rows, float* __restrict__ part) {
  __shared__ float As[32][33], Bs[32][33];
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int a0 = blockIdx.x * 32, b0 = blockIdx.y * 32;
  const int n0 = blockIdx.z * rows, n1 = min(N, n0 + rows);
  float acc[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
  for (int nb = n0; nb < n1; nb += 32) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int idx = tid + 256 * q, rn = idx >> 5, cc = idx & 31;
      const bool ok = nb + rn < n1;
      As[rn][cc] = (ok && a0 + cc < a) ? A[(size_t)(nb + rn) * lda + a0 + cc] : 0.f;
      Bs[rn][cc] = (ok && b0 + cc < b) ? B[(size_t)(nb + rn) * ldb + b0 + cc] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int n = 0; n < 32; ++n) {
      const float x0 = As[n][ty * 2], x1 = As[n][ty * 2 + 1], y0 = Bs[n][tx * 2], y1 = Bs[n][tx * 2 + 1];
      acc[0][0] = fmaf(x0, y0, acc[0][0]); acc[0][1] = fmaf(x0, y1, acc[0][1]);
      acc[1][0] = fmaf(x1, y0, acc[1][0]); acc[1][1] = fmaf(x1, y1, acc[1][1]);
    }
  }
  float* out = part + (size_t)blockIdx.z * a * b;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ia = a0 + ty * 2 + i, ib = b0 + tx * 2 + j;
      if (ia < a && ib < b) out[(size_t)ia * b + ib] = acc[i][j];
    }
}

__global__ __launch_bounds__(256) void spk_gram_reduce_kernel(const float* __restrict__ part, int nsplit, int a, int b, float* __restrict__ C,
                                                             size_t ldc) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)a * b) return;
  float t = 0.f;
  for (int s = 0; s < nsplit; ++s) t += part[(size_t)s * a * b + idx];
  C[(idx / b) * ldc + idx % b] = t;
}

struct GramSplit { int nsplit, rows; };
inline GramSplit gram_split(int N, int a, int b) {
  const long tiles = (long)((a + 31) / 32) * ((b + 31) / 32);
  long want = (LM_TARGET_BLOCKS + tiles - 1) / tiles;
  const long most = (N + 255) / 256;                 // a split sums at least 256 rows
  if (want > most) want = most;
  if (want < 1) want = 1;
  GramSplit s;
  s.rows = (int)(((N + want - 1) / want + 31) / 32 * 32);
  s.nsplit = (N + s.rows - 1) / s.rows;
  return s;
}

// Y[n, j] = (SUB ? Bin[n, j] - acc : acc), acc = sum_k A[n, k] C[k, j] in increasing k.  8 rows x 32 columns per workgroup.
template <bool SUB>
__global__ __launch_bounds__(256) void spk_panel_mul_kernel(const float* __restrict__ A, size_t lda, int a, const float* __restrict__ Cm, size_t ldc,
                                                           int b, const float* Bin, size_t ldb, float* Y, size_t ldy, int N) {
  __shared__ float As[8][65], Cs[64][32];
  const int tid = threadIdx.x, r = tid >> 5, j = tid & 31;
  const int n0 = blockIdx.x * 8;
  float acc = 0.f;
  for (int k0 = 0; k0 < a; k0 += 64) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int idx = tid + 256 * q, rr = idx >> 6, kk = idx & 63;
      As[rr][kk] = (n0 + rr < N && k0 + kk < a) ? A[(size_t)(n0 + rr) * lda + k0 + kk] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int idx = tid + 256 * q, kk = idx >> 5, jj = idx & 31;
      Cs[kk][jj] = (k0 + kk < a && jj < b) ? Cm[(size_t)(k0 + kk) * ldc + jj] : 0.f;
    }
    __syncthreads();
#pragma unroll 16
    for (int kk = 0; kk < 64; ++kk) acc = fmaf(As[r][kk], Cs[kk][j], acc);
  }
  const int n = n0 + r;
  if (n < N && j < b) Y[(size_t)n * ldy + j] = SUB ? Bin[(size_t)n * ldb + j] - acc : acc;
}

inline bool spk_n_ok(int N) { return N >= 1 && N <= TA_SPK_MAX_N; }
}  // namespace

extern "C" long ta_spk_affinity_ws_floats(int N, int D) {
  if (N < TA_SPK_MIN_N || N > TA_SPK_MAX_N || D < 1 || D > TA_SPK_MAX_D) return 0;
  return (long)N * spk_dpad(D);
}

extern "C" int ta_spk_affinity_f32(const float* E, int N, int D, int keep, float* W, long ldw, float* deg, int* kept_count, float* ws,
                                   int phases, hipStream_t st) {
  if (N < TA_SPK_MIN_N || N > TA_SPK_MAX_N || D < 1 || D > TA_SPK_MAX_D || keep < 1 || keep > N || ldw < N) return TA_ERR_ARG;
  if (!W || (phases & ~7) || !(phases & 7)) return TA_ERR_ARG;
  if ((phases & 1) && (!E || !ws || (((size_t)ws) & 15))) return TA_ERR_ARG;
  if ((phases & 4) && !deg) return TA_ERR_ARG;
  const int Dp = spk_dpad(D);
  if (phases & 1) {
    TA_LAUNCH(spk_normalize_kernel, dim3(ta_cdiv(N, 4)), dim3(256), 0, st, E, ws, N, D, Dp);
    TA_CHECK_LAUNCH();
    const int nt = ta_cdiv(N, 64);
    TA_LAUNCH(spk_cosine_kernel, dim3(nt, nt), dim3(256), 0, st, (const float*)ws, N, Dp, W, (size_t)ldw);
    TA_CHECK_LAUNCH();
  }
  if (phases & 2) {
    static bool attr = false;
    if (!attr) {
      const size_t most = ((size_t)TA_SPK_MAX_N + 256 + 4) * sizeof(float);
      if (hipFuncSetAttribute((const void*)spk_prune_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)most) != hipSuccess)
        return TA_ERR_LAUNCH;
      attr = true;
    }
    const size_t lds = ((size_t)((N + 3) & ~3) + 256 + 4) * sizeof(float);
    TA_LAUNCH(spk_prune_kernel, dim3(N), dim3(256), lds, st, W, (size_t)ldw, N, keep, kept_count);
    TA_CHECK_LAUNCH();
  }
  if (phases & 4) {
    const int nt = ta_cdiv(N, 32);
    TA_LAUNCH(spk_symmetrize_kernel, dim3(nt, nt), dim3(256), 0, st, W, (size_t)ldw, N);
    TA_CHECK_LAUNCH();
    TA_LAUNCH(spk_rowsum_kernel, dim3(N), dim3(256), 0, st, (const float*)W, (size_t)ldw, N, deg);
    TA_CHECK_LAUNCH();
  }
  return TA_OK;
}

extern "C" long ta_spk_lapmul_ws_floats(int N, int p) {
  if (!spk_n_ok(N) || p < 1 || p > TA_SPK_MAX_P) return 0;
  const LapSplit s = lap_split(N, p);
  return (long)s.nsplit * N * s.pw;
}

extern "C" int ta_spk_laplacian_matmul_f32(const float* W, long ldw, const float* deg, const float* X, long ldx, float* Y, long ldy, int N,
                                           int p, float* ws, hipStream_t st) {
  if (!spk_n_ok(N) || p < 1 || p > TA_SPK_MAX_P || ldw < N || ldx < p || ldy < p) return TA_ERR_ARG;
  if (!W || !deg || !X || !Y || !ws || X == Y) return TA_ERR_ARG;
  const LapSplit s = lap_split(N, p);
  const int vec = (ldw % 4 == 0 && (((size_t)W) & 15) == 0) ? 1 : 0;
  const dim3 grid(s.groups, s.nsplit);
  if (s.pw == 16)
    TA_LAUNCH((spk_lapmul_kernel<1>), grid, dim3(256), 0, st, W, (size_t)ldw, X, (size_t)ldx, N, p, s.chunk, ws, vec);
  else
    TA_LAUNCH((spk_lapmul_kernel<2>), grid, dim3(256), 0, st, W, (size_t)ldw, X, (size_t)ldx, N, p, s.chunk, ws, vec);
  TA_CHECK_LAUNCH();
  TA_LAUNCH(spk_lapmul_reduce_kernel, dim3(ta_cdiv((long)N * p, 256)), dim3(256), 0, st, (const float*)ws, s.nsplit, s.pw, deg, X, (size_t)ldx, Y,
            (size_t)ldy, N, p);
  TA_CHECK_LAUNCH();
  return TA_OK;
}

extern "C" long ta_spk_gram_ws_floats(int N, int a, int b) {
  if (!spk_n_ok(N) || a < 1 || a > TA_SPK_MAX_COLS || b < 1 || b > TA_SPK_MAX_COLS) return 0;
  return (long)gram_split(N, a, b).nsplit * a * b;
}

extern "C" int ta_spk_panel_gram_f32(const float* A, long lda, int a, const float* B, long ldb, int b, int N, float* C, long ldc, float* ws,
                                     hipStream_t st) {
  if (!spk_n_ok(N) || a < 1 || a > TA_SPK_MAX_COLS || b < 1 || b > TA_SPK_MAX_COLS || lda < a || ldb < b || ldc < b) return TA_ERR_ARG;
  if (!A || !B || !C || !ws) return TA_ERR_ARG;
  const GramSplit s = gram_split(N, a, b);
  TA_LAUNCH(spk_gram_kernel, dim3(ta_cdiv(a, 32), ta_cdiv(b, 32), s.nsplit), dim3(256), 0, st, A, (size_t)lda, a, B, (size_t)ldb, b, N, s.rows, ws);
  TA_CHECK_LAUNCH();
  TA_LAUNCH(spk_gram_reduce_kernel, dim3(ta_cdiv((long)a * b, 256)), dim3(256), 0, st, (const float*)ws, s.nsplit, a, b, C, (size_t)ldc);
  TA_CHECK_LAUNCH();
  return TA_OK;
}

extern "C" int ta_spk_panel_update_f32(float* B, long ldb, int b, const float* A, long lda, int a, const float* C, long ldc, int N,
                                       hipStream_t st) {
  if (!spk_n_ok(N) || a < 1 || a > TA_SPK_MAX_COLS || b < 1 || b > TA_SPK_MAX_P || lda < a || ldb < b || ldc < b) return TA_ERR_ARG;
  if (!A || !B || !C || (const float*)B == A) return TA_ERR_ARG;
  TA_LAUNCH((spk_panel_mul_kernel<true>), dim3(ta_cdiv(N, 8)), dim3(256), 0, st, A, (size_t)lda, a, C, (size_t)ldc, b, (const float*)B, (size_t)ldb, B,
            (size_t)ldb, N);
  TA_CHECK_LAUNCH();
  return TA_OK;
}

extern "C" int ta_spk_panel_combine_f32(const float* V, long ldv, int c, const float* Z, long ldz, int m, float* Y, long ldy, int N,
                                        hipStream_t st) {
  if (!spk_n_ok(N) || c < 1 || c > TA_SPK_MAX_COLS || m < 1 || m > TA_SPK_MAX_P || ldv < c || ldz < m || ldy < m) return TA_ERR_ARG;
  if (!V || !Z || !Y || (const float*)Y == V) return TA_ERR_ARG;
  TA_LAUNCH((spk_panel_mul_kernel<false>), dim3(ta_cdiv(N, 8)), dim3(256), 0, st, V, (size_t)ldv, c, Z, (size_t)ldz, m, (const float*)nullptr, (size_t)0, Y,
            (size_t)ldy, N);
  TA_CHECK_LAUNCH();
  return TA_OK;
}
