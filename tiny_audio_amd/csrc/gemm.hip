// ta355 GEMM:  C[M,N] = epilogue( A[M,K] (bf16) x W[N,K]^T (bf16) ), fp32 accumulate on MFMA.
//
// Every linear layer of the hot path is y = x W^T with W stored [out, in] (nn.Linear), so one
// "NT" kernel serves the whole step: frozen weights additionally keep a transposed bf16 copy so
// that the dX = dY W backward is NT as well (288 GB of HBM makes the second copy free).
//
// Structure (gfx950): 128x128x64 tile, 256 threads = 4 waves in 2x2, each wave 64x64 as 4x4
// v_mfma_f32_16x16x32_bf16 accumulators.  Tiles are staged HBM -> LDS with
// global_load_lds_dwordx4 (no VGPR round trip), double buffered (2 x 32 KiB), one barrier per
// K-step.  The LDS image is lane-linear (required by the DMA), so the bank-conflict-free XOR
// swizzle is applied to the per-lane *source* chunk and undone on the ds_read_b128 side.
// Operands are swapped in the MFMA (D^T = W_frag x A_frag) so that each lane owns 4 consecutive
// output columns of one row: 8-byte (bf16) / 16-byte (f32) stores, bias as one float4.
//
// A and C rows go through an affine "row map"  row -> (row / rpb) * batch_stride + (row % rpb) * ld
// which expresses, with no im2col copy:
//   * Conv1d(k=3) over a zero-padded [B, T+2, C] time-major buffer: ld = stride*C, K = 3*C
//     (GlmAsrEncoder conv1/conv2, TF:models/glmasr/modeling_glmasr.py:299-300,314-315);
//   * the projector's frame stacking [B,S,E] -> [B,S/k,k*E] incl. tail truncation
//     (tiny_audio/projectors.py:79-87).
#include "gemm_common.h"

// BMT = 128, or 96 rows per tile (waves 2x2 of 48x64): M = 6144 x N = 1024 is then 512 tiles = every resident slot of the
// chip (two workgroups per CU) instead of 384.
// KEXT: the K extension of ta_gemm_opts.a2/w2 (LoRA) is compiled in (its pointer switch sits in the main loop: 0.3 ms per
// step for every GEMM when it was a run-time test)
template <int ACT, bool OUT_BF16, bool HAS_RES, int BMT = 128, bool KEXT = false>
__global__ __launch_bounds__(256, 2) void gemm_nt_kernel(GemmArgs p) {
  constexpr int MI = BMT / 32, WR = BMT / 2;       // 16-row fragments per wave, rows per wave
  __shared__ __attribute__((aligned(16))) char smem[4 * TILE_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int g = lane >> 4, l15 = lane & 15;

  // This kernel keeps its own copy of the tile walk (tile_ctx, gemm_common.h, is what the other three call; the group height here
  // defaults to 8).  With tile_ctx it had 1-2 VGPRs fewer and the same bits, and every launch of the step on it measured
  // 0.5 - 1.4 % slower (17.63 against 17.36 us for M = 4000, N = K = 1024 on 96-row tiles; profiles/gemm_refactor.md).
  // ---- XCD-aware, grouped tile order (block b runs on XCD b % 8: give each XCD a contiguous chunk)
  const int nwg = gridDim.x;
  int bid = blockIdx.x;
  {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, within = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + within;
  }
  const int tiles = p.tiles_m * p.tiles_n;
  const int z = bid / tiles;
  int t = bid - z * tiles;
  const int GROUP_M = p.group_m > 0 ? p.group_m : 8;
  const int width = GROUP_M * p.tiles_n;
  const int group = t / width;
  const int first_m = group * GROUP_M;
  const int gsize = min(p.tiles_m - first_m, GROUP_M);
  int pm = first_m + (t % width) % gsize;
  const int pn = (t % width) / gsize;
  const int* segp; const bf16_t* Wp; const float* biasp; const int* krp;
  if (!resolve_group<BMT>(p, pm, z, segp, Wp, biasp, krp)) return;            // block-uniform: before any barrier
  const int m0 = pm * BMT, n0 = pn * BN;

  const int nkt = p.K / BK;
  int kt_begin = 0, kt_end = nkt;                  // 32-bit, and only when split: two 64-bit quotients cost ~2 k cycles per workgroup
  if (p.splits > 1) { kt_begin = (nkt * z) / p.splits; kt_end = (nkt * (z + 1)) / p.splits; }
  if (krp) { kt_begin = krp[0]; kt_end = krp[1]; }
  if (KEXT) kt_end = nkt + p.K2 / BK;              // K extension (host guarantees splits == 1, no krange)
  int Mact = p.M, rbase = 0;
  if (segp) { rbase = segp[0]; Mact = segp[1]; if (m0 >= Mact) return; }

  // ---- per-thread DMA source pointers: 4 x 16 B chunks of A and of W per K-step
  const int lr = tid >> 3;
  const int clog = (tid & 7) ^ ((lr >> 1) & 7);
  const char* a_src[MI];
  const char* w_src[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = i * 32 + lr;
    if (i < MI) a_src[i] = a_chunk_src(p, rbase + min(m0 + r, Mact - 1), kt_begin, clog);
    w_src[i] = w_chunk_src(p, Wp, min(n0 + r, p.N - 1), nkt, kt_begin, clog);
  }
  const int w_step = p.w_blocked ? 8192 : BK * 2;      // bytes to the next K tile of the same rows
  char* lds_w = smem + wave * 1024;   // + buf*2*TILE + (A:0 | W:TILE) + i*4096, lane*16 added by the DMA

  // ---- per-lane fragment read offsets (bytes) inside a tile
  const int a_rd = (wm * WR + l15) * 128;
  const int b_rd = (wn * 64 + l15) * 128;
  const FragOff ko2 = frag_koff(l15, g);

  f32x4 acc[MI][4];
  const bool res_init = residual_is_start<ACT, OUT_BF16, HAS_RES>(p);
  if (res_init) residual_start<MI, 4>(acc, p, m0 + wm * WR + l15, Mact, rbase, n0 + wn * 64, g);
  else zero_acc<MI, 4>(acc);

  int next_tile = kt_begin;
  auto stage = [&](int buf) {
    if (KEXT && next_tile == nkt) {                // switch both operands to the extension
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = i * 32 + lr;
        if (i < MI) a_src[i] = (const char*)(p.A2 + (long)(rbase + min(m0 + r, Mact - 1)) * p.lda2 + clog * 8);
        w_src[i] = (const char*)(p.W2 + (long)min(n0 + r, p.N - 1) * p.K2 + clog * 8);
      }
    }
    ++next_tile;
    char* base = lds_w + buf * (2 * TILE_BYTES);
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      glds16(a_src[i], base + i * 4096);
      a_src[i] += BK * 2;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      glds16(w_src[i], base + TILE_BYTES + i * 4096);
      w_src[i] += w_step;
    }
  };

  if (kt_begin < kt_end) stage(0);
  __syncthreads();
  for (int kt = kt_begin; kt < kt_end; ++kt) {
    const int cur = (kt - kt_begin) & 1;
    if (kt + 1 < kt_end) stage(cur ^ 1);
    const char* As = smem + cur * (2 * TILE_BYTES);
    const char* Bs = As + TILE_BYTES;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int ko = kk ? ko2.k1 : ko2.k0;
      bf16x8 af[MI], bfr[4];
#pragma unroll
      for (int i = 0; i < MI; ++i) af[i] = *(const bf16x8*)(As + a_rd + i * 2048 + ko);
#pragma unroll
      for (int j = 0; j < 4; ++j) bfr[j] = *(const bf16x8*)(Bs + b_rd + j * 2048 + ko);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }

  // ---- epilogue: lane owns row m = .. + l15, columns n .. n+3 (n = .. + g*4)
  char* Cb = (char*)p.C;
  if (p.splits > 1) Cb += (long)z * p.slab_stride * 4;
  const bool wide = p.wide != 0;
  const float2* lut = stage_gelu_lut<ACT, 256>(smem, p, tid, false);       // the K loop ended with a barrier
  if (res_init) epilogue_tile<MI, 4, ACT, OUT_BF16, false>(acc, p, Cb, m0 + wm * WR + l15, Mact, rbase, n0 + wn * 64, g, wide, biasp, lut);
  else epilogue_tile<MI, 4, ACT, OUT_BF16, HAS_RES>(acc, p, Cb, m0 + wm * WR + l15, Mact, rbase, n0 + wn * 64, g, wide, biasp, lut);
}

// ============================================================================ v2: 256-row tiles, 8 waves, 1 WG / CU
// The 128x128 kernel above is bound by the per-CU L2 -> LDS DMA rate: it must stage 32 KB per 2.1 MFLOP tile-step
// (profiles/r01_a_pmc_summary.md: L2 request volume ~48x the algorithmic bytes).  A 256 x BN2 tile halves
// (BN2 = 256) the bytes staged per flop.  8 waves as 2 (M) x 4 (N): each wave owns
// 128 x BN2/4 outputs = 8 x NT accumulator fragments.  Same DMA + source-side swizzle + double buffer as v1.
// (Rounds 1-5 also had a plain double-buffered main loop on this tile -- variants 1, 256x256, and 2, 256x128, with the next
// K tile's DMA interleaved in four places between MFMA groups: 0.9 and 0.5 of the 128x128 kernel's rate per unit area against
// 1.40 for the schedule below, so the launch-time model could choose neither; DESIGN.md "dead ends".)
//
// Ping-pong: the two wave groups (wm = 0 / 1; wave w and w+4 share a SIMD) run ONE barrier interval apart,
// alternating a load interval L(t,s) = {ds_read the 12 fragments of k-step s (+ issue the next tile's DMA when
// s = 0); wait for them} with a compute interval C(t,s) = {32 MFMAs}.  In every interval one group feeds the
// matrix pipe while its SIMD partner loads, so the pipe never waits on LDS latency, DMA issue or the barrier:
//   global barrier #   ..4t | 4t+1 | 4t+2 | 4t+3 | 4t+4 ..
//   group 0            L(t,0)+DMA(t+1) | C(t,0) | L(t,1) | C(t,1) | L(t+1,0)
//   group 1            C(t-1,1) | L(t,0)+DMA(t+1) | C(t,0) | L(t,1) | C(t,1)
// Hazards: every wave drains its own DMA (vmcnt 0) at the end of L(t,1), i.e. before barrier 4t+3 (group 0) /
// 4t+4 (group 1), and the first read of tile t+1 is after barrier 4t+4; the last reads of tile t-1 (group 1's
// L(t-1,1)) retire (lgkmcnt 0) before barrier 4t, and the first DMA into that buffer is issued after it.
// The K step itself is pingpong_ktile (gemm_common.h), shared with the persistent form below.
template <int BN2, int ACT, bool OUT_BF16, bool HAS_RES, bool KEXT = false>
__global__ __launch_bounds__(512, 2) void gemm_nt_kernel_v2(GemmArgs p) {
  constexpr int BM2 = 256;
  constexpr int NT = BN2 / 64;                 // n-fragments per wave
  constexpr int NA = BM2 / 64, NB = BN2 / 64;  // 16-B DMA chunks per thread per K-tile (A, W)
  constexpr int A_BYTES = BM2 * 128, STAGE = (BM2 + BN2) * 128;
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3;
  const int g = lane >> 4, l15 = lane & 15;

  const TileCtx c = block_tile<BM2, BN2>(p);
  if (!c.ok) return;
  const int m0 = c.m0, n0 = c.n0, z = c.z, Mact = c.Mact, rbase = c.rbase;
  const bf16_t* Wp = c.Wp; const float* biasp = c.biasp;
  const int nkt = p.K / BK;
  const int kt_begin = c.kb;
  const int kt_end = KEXT ? nkt + p.K2 / BK : c.ke;

  const int lr = tid >> 3;                                    // 0..63
  const int clog = (tid & 7) ^ ((lr >> 1) & 7);
  const char* a_src[NA];
  const char* w_src[NB];
#pragma unroll
  for (int i = 0; i < NA; ++i) a_src[i] = a_chunk_src(p, rbase + min(m0 + i * 64 + lr, Mact - 1), kt_begin, clog);
#pragma unroll
  for (int i = 0; i < NB; ++i) w_src[i] = w_chunk_src(p, Wp, min(n0 + i * 64 + lr, p.N - 1), nkt, kt_begin, clog);
  const int w_step = p.w_blocked ? 8192 : BK * 2;
  char* lds_w = smem + wave * 1024;

  const int a_rd = (wm * 128 + l15) * 128;
  const int b_rd = A_BYTES + (wn * (BN2 / 4) + l15) * 128;
  const FragOff ko2 = frag_koff(l15, g);

  f32x4 acc[8][NT];
  const bool res_init = residual_is_start<ACT, OUT_BF16, HAS_RES>(p);
  if (res_init) residual_start<8, NT>(acc, p, m0 + wm * 128 + l15, Mact, rbase, n0 + wn * (BN2 / 4), g);
  else zero_acc<8, NT>(acc);

  auto dma_tile = [&](char* base, int tile) {       // K tile `tile` of both operands into the stage at `base`
    if (KEXT && tile == nkt) {                      // switch both operands to the extension
#pragma unroll
      for (int i = 0; i < NA; ++i)
        a_src[i] = (const char*)(p.A2 + (long)(rbase + min(m0 + i * 64 + lr, Mact - 1)) * p.lda2 + clog * 8);
#pragma unroll
      for (int i = 0; i < NB; ++i)
        w_src[i] = (const char*)(p.W2 + (long)min(n0 + i * 64 + lr, p.N - 1) * p.K2 + clog * 8);
    }
#pragma unroll
    for (int i = 0; i < NA; ++i) { glds16(a_src[i], base + i * 8192); a_src[i] += BK * 2; }
#pragma unroll
    for (int i = 0; i < NB; ++i) { glds16(w_src[i], base + A_BYTES + i * 8192); w_src[i] += w_step; }
  };

  if (kt_begin < kt_end) dma_tile(lds_w, kt_begin);
  __syncthreads();
  const int lag = __builtin_amdgcn_readfirstlane(wm);     // SGPR: scalar branches around the extra barriers
  if (lag) __builtin_amdgcn_s_barrier();
  for (int kt = kt_begin; kt < kt_end; ++kt) {
    const int cur = (kt - kt_begin) & 1;
    const bool more = kt + 1 < kt_end;
    char* nxt = lds_w + (cur ^ 1) * STAGE;
    pingpong_ktile<8, NT>(smem + cur * STAGE, a_rd, b_rd, ko2, acc, [&] { if (more) dma_tile(nxt, kt + 1); });
  }
  if (!lag) __builtin_amdgcn_s_barrier();

  char* Cb = (char*)p.C;
  if (p.splits > 1) Cb += (long)z * p.slab_stride * 4;
  const bool wide = p.wide != 0;
  const float2* lut = stage_gelu_lut<ACT, 512>(smem, p, tid, false);       // both wave groups are past their last LDS read
  if (res_init) epilogue_tile<8, NT, ACT, OUT_BF16, false>(acc, p, Cb, m0 + wm * 128 + l15, Mact, rbase, n0 + wn * (BN2 / 4), g, wide, biasp, lut);
  else epilogue_tile<8, NT, ACT, OUT_BF16, HAS_RES>(acc, p, Cb, m0 + wm * 128 + l15, Mact, rbase, n0 + wn * (BN2 / 4), g, wide, biasp, lut);
}


// ============================================================================ v4: the ping-pong tile as a PERSISTENT workgroup
// Measured on v2 (scripts/gemm_wg_life.py, profiles/r02_gemm_wg_life.txt): of the ~90 k cycles a CU spends per 256x320 tile of a
// K = 1280 GEMM, 70 k are the main loop; 9.4 k go to issuing the epilogue's stores (16 rows x 64 B per instruction: the
// store path takes row segments, not bytes), 4.7 k to the prologue (address set-up + the first K tile's DMA latency) and
// 5.0 k pass between one workgroup's last store and the next workgroup's first instruction on that CU.  v4 keeps v2's
// main loop (same accumulation order: bit-identical results) and changes what surrounds it:
//   * grid = min(tiles, CUs); workgroup b walks tiles b, b + grid, ... (the same tile -> XCD map as the plain launch order),
//     so a CU never waits for a workgroup hand-over between rounds;
//   * after the main loop BOTH stage buffers are free: the next tile's first K tile is DMA'd into stage 0 BEFORE the
//     epilogue, whose latency it hides behind the stores;
//   * the DMA sources are a uniform base pointer (SGPR pair, stepped along K by scalar adds) + one 32-bit byte offset per
//     16-B chunk: 9 registers instead of 18 and no vector adds in the main loop (which is what makes room for the loop-carried
//     state of a persistent workgroup next to 160 accumulator registers);
//   * the epilogue is v2's (direct stores in the accumulator layout).  Staging the bf16 tile through LDS to store whole
//     640-B rows was built and measured: a CU issues contiguous 1-KB stores at 46 B/clk against 22 B/clk for the 16 rows x
//     64 B of the direct form (scripts/probe/store_rate.hip), but pack + ds_write + barrier + ds_read per 64-row pass cost
//     more than the stores saved (10.3 k cycles per tile against 8.5 k), so it was removed.
// Per tile of a K = 1280 GEMM: 0.7 k wait + 60.5 k main loop + 2.2 k next-tile set-up + ~8.5 k epilogue, against 90 k for v2.

// BM2 = 192 (round 3): the same kernel on a 192-row tile (each wave group owns 96 rows = 6 fragment rows).  M = 6144 (the LM at
// B = 32) is 32 x 192: N = 2048 gives 256 tiles = ONE per CU and N = 4096 gives 512 = two full rounds, where 256-row tiles leave
// a quarter of the chip idle (192 of 256 CUs; 1.5 rounds).
template <int BN2, int ACT, bool OUT_BF16, bool HAS_RES, int BM2 = 256>
__global__ __launch_bounds__(512, 2) void gemm_nt_kernel_v4(GemmArgs p) {
  constexpr int MI = BM2 / 32;                      // 16-row fragment rows per wave (two wave groups split the tile's rows)
  constexpr int NT = BN2 / 64;
  constexpr int NA = BM2 / 64, NB = BN2 / 64;
  constexpr int A_BYTES = BM2 * 128, STAGE = (BM2 + BN2) * 128;
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3;
  const int g = lane >> 4, l15 = lane & 15;
  const int total = p.tiles_m * p.tiles_n * p.splits;
  const int nkt = p.K / BK;

  // DMA sources: a uniform base pointer that walks along K (scalar adds) + one 32-bit byte offset per 16-B chunk
  // (operands < 4 GB, checked by the host): half the registers of per-chunk pointers and no vector adds in the main loop
  const char* a_base; const char* w_base;
  unsigned a_off[NA], w_off[NB];
  const int w_step = p.w_blocked ? 8192 : BK * 2;
  // A given as [M/64][K/64][64][64] blocks, like w_blocked (round 3 probe).  No entry point sets a_blocked; the branch stays because the
  // register allocation of every instantiation hangs on it: without it the kernels of the step take 5-6 more VGPRs and the 256-VGPR
  // o_proj / fc2 kernel <320, 0, true, true> gets 16 bytes of scratch (profiles/gemm_prune_isa.md)
  const bool a_blk = p.a_blocked != 0;
  const int a_step = a_blk ? 8192 : BK * 2;
  // wave-uniform LDS byte address of this wave's 1-KB DMA window in stage 0
  const unsigned lds_w = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long)(__attribute__((address_space(3))) char*)smem + wave * 1024);
  const int a_rd = (wm * (BM2 / 2) + l15) * 128;
  const int b_rd = A_BYTES + (wn * (BN2 / 4) + l15) * 128;
  const FragOff ko2 = frag_koff(l15, g);
  const int lag = __builtin_amdgcn_readfirstlane(wm);
  // The thread index, re-derived where the code around the main loop needs it (wave number from an SGPR + v_mbcnt): index
  // arithmetic that started from threadIdx.x was hoisted out of the tile loop and carried, spilled, across the main loop.
  const int wave_s = __builtin_amdgcn_readfirstlane(wave);
  auto fresh_tid = [&]() -> int {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return wave_s * 64 + l;
  };

  auto dma_tile = [&](unsigned base) {                          // one K tile of both operands; the bases step to the next one
    const char* ab = uniform_ptr(a_base);
    const char* wb = uniform_ptr(w_base);
#pragma unroll
    for (int i = 0; i < NA; ++i) glds16_s(ab, a_off[i], base + i * 8192);
#pragma unroll
    for (int i = 0; i < NB; ++i) glds16_s(wb, w_off[i], base + A_BYTES + i * 8192);
    a_base += a_step; w_base += w_step;
  };
  // Offsets are relative to the tile's first row of each operand (the base carries the rest), so they stay far below 4 GB
  // whatever the operand's size; only A under a non-identity row map is addressed from the start of A (host: < 4 GB, no gather).
  auto first_dma = [&](const TileCtx& c, int st) {              // sources of tile c + its first K tile into stage st
    const int te = fresh_tid(), lr = te >> 3, clog = (te & 7) ^ ((lr >> 1) & 7);
    if (a_blk) {
#pragma unroll
      for (int i = 0; i < NA; ++i) a_off[i] = (unsigned)((((long)(i * nkt) << 12) + (lr << 6) + clog * 8) * 2);
      a_base = (const char*)(p.A + ((((long)((c.rbase + c.m0) >> 6)) * nkt + c.kb) << 12));
    } else if (p.a_plain) {
#pragma unroll
      for (int i = 0; i < NA; ++i)
        a_off[i] = rel_off(min(c.m0 + i * 64 + lr, c.Mact - 1), c.m0, p.lda, clog);
      a_base = (const char*)(p.A + (long)(c.rbase + c.m0) * p.lda) + (long)c.kb * (BK * 2);
    } else {
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        a_off[i] = (unsigned)((a_row_off(p, c.rbase + min(c.m0 + i * 64 + lr, c.Mact - 1)) + clog * 8) * 2);
      }
      a_base = (const char*)p.A + (long)c.kb * (BK * 2);
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int gn = min(c.n0 + i * 64 + lr, p.N - 1);
      w_off[i] = p.w_blocked ? (unsigned)(((((long)((gn >> 6) - (c.n0 >> 6)) * nkt) << 12) + ((gn & 63) << 6) + clog * 8) * 2)
                             : rel_off(gn, c.n0, p.K, clog);
    }
    w_base = (const char*)c.Wp + (p.w_blocked ? (((long)(c.n0 >> 6) * nkt) << 13) + (long)c.kb * 8192 : ((long)c.n0 * p.K + (long)c.kb * BK) * 2);
    if (c.kb < c.ke) dma_tile(lds_w + st * STAGE);
  };
  // The epilogue's constants of tile c into the stage whose wave window starts at `base` (see EPI_LDS_*): issued where the main
  // loop's LAST K tile would request its successor, waited for by that K tile's own vmcnt(0) + barriers.
  constexpr bool GELU = ACT == 1;
  constexpr bool ROPE = ACT == 2;
  auto dma_epi = [&](const TileCtx& c, unsigned base) {
    const int te = fresh_tid();                                 // (keeps this address arithmetic out of the K loop's live ranges)
    if (c.biasp && te < BN2 / 4) {
      const int n = c.n0 + te * 4;
      glds16_s(uniform_ptr((const char*)c.biasp), (unsigned)((n < p.N ? n : p.N - 4) * 4), base + EPI_LDS_BIAS);
    }
    if (GELU && !p.gelu_erf) {
      static_assert(GELU_LUT_N * 8 == 512 * 16, "one 16-B piece per thread");
      glds16_s(uniform_ptr((const char*)kGeluLut), (unsigned)(te * 16), base + EPI_LDS_TAB);
    }
    if (ROPE) {
      const char* rb = uniform_ptr((const char*)p.rope_tab);
#pragma unroll
      for (int i = 0; i < BM2 * 128 / 8192; ++i) {
        const int q = i * 512 + te, r = q >> 3, cch = q & 7;
        const int m = c.rbase + min(c.m0 + r, c.Mact - 1);
        glds16_s(rb, (unsigned)(((m % p.rope_rows) * 32 + ((cch ^ (r & 7)) << 2)) * 4), base + EPI_LDS_TAB + i * 8192);
      }
    }
  };

  const bool res_init = residual_is_start<ACT, OUT_BF16, HAS_RES>(p);
  int h = blockIdx.x;
  TileCtx cur = tile_ctx<BM2, BN2>(p, h, total);
  while (!cur.ok) {                                              // surplus tiles of a grouped launch
    h += gridDim.x;
    if (h >= total) return;
    cur = tile_ctx<BM2, BN2>(p, h, total);
  }
  int ph = 0;                                                    // the stage that receives the tile's first K tile
  first_dma(cur, ph);

  for (;;) {
    f32x4 acc[MI][NT];
    // the residual's loads (residual_start) go out here, behind the first K tile's DMA and in front of the wait that tile needs anyway
    if (res_init) {
      const int te = fresh_tid();
      residual_start<MI, NT>(acc, p, cur.m0 + (te >> 8) * (BM2 / 2) + (te & 15), cur.Mact, cur.rbase, cur.n0 + ((te >> 6) & 3) * (BN2 / 4), (te >> 4) & 3);
    } else {
      zero_acc<MI, NT>(acc);
    }

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // this wave's share of the first K tile (and its last stores)
    __syncthreads();                                             // every wave is past the previous epilogue's LDS reads
    // which tile comes next is scalar work (two divisions, the grouped launches' table look-ups): done HERE, where it shares the
    // issue slots with the main loop's first MFMAs, instead of between the main loop and the epilogue (~1 k cycles per tile)
    int hn = h + gridDim.x;
    TileCtx nx; nx.ok = 0;
    while (hn < total) {
      nx = tile_ctx<BM2, BN2>(p, hn, total);
      if (nx.ok) break;
      hn += gridDim.x;
    }
    if (lag) __builtin_amdgcn_s_barrier();
    // (Round 3, measured and removed: giving every DMA three barrier intervals to land instead of two -- the leading group waiting for
    // K tile kt + 1 only in front of the iteration's last barrier, the lagging group requesting K tile kt + 2 right behind the barrier
    // that ends its last reads of stage cs.  Bit-identical, race hunt clean; the late wait changed nothing (40.79 vs 40.70 ms per
    // step) and the early request cost 2.1 ms (42.8): both groups' DMA bursts then leave in the same interval instead of one apart.
    // DMA latency is not what these GEMMs wait for.  profiles/r03_w_ab_dma_schedule.txt)
    for (int kt = cur.kb; kt < cur.ke; ++kt) {
      const int cs = ((kt - cur.kb) & 1) ^ ph;
      const bool more = kt + 1 < cur.ke;
      const unsigned nxt = lds_w + (cs ^ 1) * STAGE;
      // the issue step: the next K tile, or -- behind the last one -- the epilogue's constants
      pingpong_ktile<MI, NT>(smem + cs * STAGE, a_rd, b_rd, ko2, acc, [&] { if (more) dma_tile(nxt); else dma_epi(cur, nxt); });
    }
    if (!lag) __builtin_amdgcn_s_barrier();                      // both groups are past their last LDS read: both stages are free

    // ---- the next tile of this workgroup (found before the main loop): its first K tile travels while the epilogue runs
    // the last K tile sat in stage `last`: free now, it takes the next tile's first K tile; the other one holds the epilogue's
    // constants until the next tile's SECOND K tile is requested (behind the next loop-top barrier, i.e. after this epilogue)
    const int nK = cur.ke - cur.kb;
    const int last = __builtin_amdgcn_readfirstlane(nK > 0 ? (((nK - 1) & 1) ^ ph) : ph);
    const char* els = smem + (last ^ 1) * STAGE;
    if (nK <= 0) {                                               // (an empty K range: nothing was staged on the way)
      dma_epi(cur, lds_w + (last ^ 1) * STAGE);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    if (nx.ok) first_dma(nx, last);
    const float2* lut = (GELU && !p.gelu_erf) ? (const float2*)(els + EPI_LDS_TAB) : nullptr;

    // ---- epilogue of `cur`.  Its index arithmetic starts from an opaque copy of the thread index: otherwise the compiler
    // hoists those loop-invariant values out of the tile loop and carries them, spilled, across the main loop.
    const int te = fresh_tid();
    const int e_l15 = te & 15, e_g = (te >> 4) & 3, e_wn = (te >> 6) & 3, e_wm = te >> 8;
    char* Cb = (char*)p.C;
    if (p.splits > 1) Cb += (long)cur.z * p.slab_stride * 4;
    const bool wide = p.wide != 0;
    const int erow0 = e_wm * (BM2 / 2) + e_l15;
    // full tiles: row-merged stores
    const bool full = OUT_BF16 && wide && p.c_plain && (!HAS_RES || res_init) && cur.m0 + BM2 <= cur.Mact && cur.n0 + BN2 <= p.N;
    if constexpr (OUT_BF16) {
      if (full) epilogue_tile_full<MI, NT, ACT, true>(acc, p, Cb, cur.m0 + erow0, cur.rbase, cur.n0 + e_wn * (BN2 / 4), e_g, cur.biasp, lut, els, cur.n0, erow0);
    }
    if (full) { }
    else if (res_init)
      epilogue_tile<MI, NT, ACT, OUT_BF16, false, 0, true>(acc, p, Cb, cur.m0 + erow0, cur.Mact, cur.rbase, cur.n0 + e_wn * (BN2 / 4), e_g,
                                                           wide, cur.biasp, lut, els, cur.n0, erow0);
    else
      epilogue_tile<MI, NT, ACT, OUT_BF16, HAS_RES, ((BM2 == 192 || (HAS_RES && !OUT_BF16 && ACT == 0)) ? 1 : 0), true>(acc, p, Cb, cur.m0 + erow0, cur.Mact, cur.rbase,
                                                                                cur.n0 + e_wn * (BN2 / 4), e_g, wide, cur.biasp, lut, els, cur.n0, erow0);
    if (!nx.ok) return;
    cur = nx; h = hn; ph = last;
  }
}


// (v3, the 4-slot ring of 32-deep half K-tiles -- variants 6 / 7, experiment builds of rounds 2-5 -- and v6, v5 on
// v_mfma_f32_32x32x16_bf16 -- variant 11 -- measured slower in the step and live in scripts/attic/gemm_r05_with_experiments.hip.txt;
// DESIGN.md "dead ends".)

// out[i] = (add ? add[i] : 0) + sum_z slab[z][i]  (f32 and/or bf16 out; add may alias out); n4 = count / 4
__global__ void splitk_reduce_kernel(const float* __restrict__ slabs, int splits, long slab_stride, const float* add,
                                     float* out, bf16_t* __restrict__ out_bf, long n4) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    float4 s = add ? ((const float4*)add)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int z = 0; z < splits; ++z) {
      const float4 v = ((const float4*)(slabs + (long)z * slab_stride))[i];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    if (out) ((float4*)out)[i] = s;
    if (out_bf) {
      uint2 o; o.x = pack2bf(s.x, s.y); o.y = pack2bf(s.z, s.w);
      ((uint2*)out_bf)[i] = o;
    }
  }
}

// ============================================================================ v5: 192 x 128 tile, ONE 4-wave workgroup per CU, 3-slot ring
// For outputs that are ONE round of small tiles (the LM's M = 6144 x N = 1024 products: 512 tiles of 96x128, two per CU, or
// 256 tiles of 192x128).  One 192 x 128 tile per CU stages (192 + 128) rows per K step instead of 2 x (96 + 128), and as 4 waves
// of 96 x 64 (6 A + 4 W fragments per 24 MFMAs) it reads 10 KB of LDS per 24 MFMAs instead of 7 KB per 12.  With a single wave
// per SIMD nothing else hides latency or issue slots, so:
//   * a ring of 3 K-tile slots (120 KB): group t+2 is DMA'd while tile t is computed; the wait for group t+1 is counted
//     (s_waitcnt vmcnt(10): one group of 10 instructions may stay in flight), i.e. every DMA has two K tiles to land;
//   * fragments are double-buffered in registers: the ds_reads of half-step h+1 and the DMA issues of group t+2 sit BETWEEN the
//     24 MFMAs of half-step h, one per MFMA (all of them in front of the MFMA group: 660 cycles per half-step for 384 of MFMA);
//   * DMA sources are a uniform base + 32-bit tile-relative offsets (as in v4); rows are 128 B (whole lines: a first version
//     with 64-B half K-tile slots needed one address-path cycle per 64-B row segment, 320 per half-step -- measured 700 cycles
//     per half-step against 400 with the DMA removed);
//   * one barrier per K TILE: it publishes slot t+1 (every wave waited for its own share) and retires slot t-1.
// Slot image: v2's ([rows][128 B], 16-B chunk index XOR (row >> 1 & 7), applied on the source side of the DMA).
template <int N> __device__ __forceinline__ void wait_vm_lgkm0_n() { asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory"); }
// KEXT: the K extension of ta_gemm_opts.a2 / w2 (LoRA): after the K tiles of A / W the groups continue over A2 / W2.
template <int ACT, bool OUT_BF16, bool HAS_RES, bool KEXT = false>
__global__ __launch_bounds__(256) void gemm_nt_kernel_v5(GemmArgs p) {
  constexpr int BM5 = 192, BN5 = 128, NS = 3;
  constexpr int A_BYTES = BM5 * 128, SLOT = (BM5 + BN5) * 128;
  __shared__ __attribute__((aligned(16))) char smem[NS * SLOT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int g = lane >> 4, l15 = lane & 15;

  const TileCtx c = block_tile<BM5, BN5>(p);
  if (!c.ok) return;
  const int m0 = c.m0, n0 = c.n0, z = c.z, Mact = c.Mact, rbase = c.rbase;
  const bf16_t* Wp = c.Wp; const float* biasp = c.biasp;
  const int nkt = p.K / BK;
  const int kt_begin = c.kb;
  const int kt_end = KEXT ? nkt + p.K2 / BK : c.ke;   // host guarantees splits == 1, no krange

  // ---- DMA sources: pass q stages rows [32 q, 32 q + 32) of A (q < 6) / of W (q - 6 < 4); a thread owns one 16-B chunk per pass
  const int lr = tid >> 3;
  const int clog = (tid & 7) ^ ((lr >> 1) & 7);
  unsigned a_off[6], w_off[4];
  const char* a_base; const char* w_base;
  if (p.a_plain) {
#pragma unroll
    for (int q = 0; q < 6; ++q)
      a_off[q] = rel_off(min(m0 + q * 32 + lr, Mact - 1), m0, p.lda, clog);
    a_base = (const char*)(p.A + (long)(rbase + m0) * p.lda) + (long)kt_begin * (BK * 2);
  } else {
#pragma unroll
    for (int q = 0; q < 6; ++q) a_off[q] = (unsigned)((a_row_off(p, rbase + min(m0 + q * 32 + lr, Mact - 1)) + clog * 8) * 2);
    a_base = (const char*)p.A + (long)kt_begin * (BK * 2);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q)
    w_off[q] = rel_off(min(n0 + q * 32 + lr, p.N - 1), n0, p.K, clog);
  w_base = (const char*)(Wp + (long)n0 * p.K) + (long)kt_begin * (BK * 2);
  const unsigned lds_w = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long)(__attribute__((address_space(3))) char*)smem + wave * 1024);

  const int a_rd = (wm * 96 + l15) * 128;
  const int b_rd = A_BYTES + (wn * 64 + l15) * 128;
  const FragOff ko2 = frag_koff(l15, g);

  f32x4 acc[6][4];
  const bool res_init = residual_is_start<ACT, OUT_BF16, HAS_RES>(p);
  if (res_init) residual_start<6, 4>(acc, p, m0 + wm * 96 + l15, Mact, rbase, n0 + wn * 64, g);
  else zero_acc<6, 4>(acc);

  const int nt = kt_end - kt_begin;
  if (nt > 0) {
    // DMA group k (k = 0, 1, ...) loads K tile min(k, nt - 1) into slot k % 3: the groups past the end re-load the last tile into
    // a retired slot, so that every K tile issues exactly one group and every wait is the same count.
    int islot = 0, kgrp = 0;
    auto advance = [&]() {
      ++kgrp;
      if (kgrp < nt) {
        if (KEXT && kt_begin + kgrp == nkt) {                   // the next group is the first K tile of the extension
          a_base = (const char*)(p.A2 + (long)(rbase + m0) * p.lda2);
          w_base = (const char*)(p.W2 + (long)n0 * p.K2);
#pragma unroll
          for (int q = 0; q < 6; ++q) a_off[q] = rel_off(min(m0 + q * 32 + lr, Mact - 1), m0, p.lda2, clog);
#pragma unroll
          for (int q = 0; q < 4; ++q) w_off[q] = rel_off(min(n0 + q * 32 + lr, p.N - 1), n0, p.K2, clog);
        } else {
          a_base += BK * 2; w_base += BK * 2;
        }
      }
      islot = islot == NS - 1 ? 0 : islot + 1;
    };
    for (int hh = 0; hh < 2; ++hh) {
      const char* ab = uniform_ptr(a_base);
      const char* wb = uniform_ptr(w_base);
      const unsigned base = lds_w + islot * SLOT;
#pragma unroll
      for (int q = 0; q < 6; ++q) glds16_s(ab, a_off[q], base + q * 4096);
#pragma unroll
      for (int q = 0; q < 4; ++q) glds16_s(wb, w_off[q], base + A_BYTES + q * 4096);
      advance();
    }
    bf16x8 af0[6], bf0[4], af1[6], bf1[4];
    wait_vm_lgkm0_n<10>();                                     // group 0 landed
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int j = 0; j < 4; ++j) bf0[j] = *(const bf16x8*)(smem + b_rd + j * 2048 + ko2.k0);
#pragma unroll
    for (int i = 0; i < 6; ++i) af0[i] = *(const bf16x8*)(smem + a_rd + i * 2048 + ko2.k0);
    int rslot = 0;                                             // slot of the K tile being computed
    // One half-step.  FIRST (k columns 0..31 of tile t): MFMAs on (ca, cb), reads of the second half of the same slot into
    // (na, nb), DMA of group t + 2 into the slot tile t - 1 left.  SECOND: waits for group t + 1 (group t + 2 may stay in flight),
    // barrier, MFMAs, reads of the first half of slot t + 1.  In the last half-step the reads fetch a slot nobody uses.
    auto step = [&](auto first_tag, bf16x8* ca, bf16x8* cb, bf16x8* na, bf16x8* nb) {
      constexpr bool FIRST = decltype(first_tag)::value;
      const int nslot = rslot == NS - 1 ? 0 : rslot + 1;
      if (FIRST) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      else wait_vm_lgkm0_n<10>();
      // pass the fragments through an empty asm: the compiler's own wait for them lands HERE, not behind the reads issued below.
      // The A fragment read LAST goes first, so that this is one lgkmcnt(0) whatever the compiler knows about its counters: in
      // issue order it can become a ladder lgkmcnt(5) ... lgkmcnt(0) behind the wait above -- ten more s_waitcnt per K tile with
      // nothing to hide them at one wave per SIMD, 55.1 against 54.2 us for K = 5120 (profiles/gemm_refactor.md)
#pragma unroll
      for (int i = 5; i >= 0; --i) asm volatile("" : "+v"(ca[i]));
#pragma unroll
      for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(cb[j]));
      __builtin_amdgcn_sched_barrier(0);
      if (!FIRST) {
        __builtin_amdgcn_s_barrier();                          // slot t + 1 is complete; slot t may be overwritten (by group t + 3, next tile)
        __builtin_amdgcn_sched_barrier(0);
      }
      const char* S = smem + (FIRST ? rslot : nslot) * SLOT + (FIRST ? ko2.k1 : ko2.k0);
      const char* ab = uniform_ptr(a_base);
      const char* wb = uniform_ptr(w_base);
      const unsigned base = lds_w + islot * SLOT;
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int q = 0; q < 24; ++q) {
        const int i = q >> 2, j = q & 3;
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cb[j], ca[i], acc[i][j], 0, 0, 0);
        if (q < 4) nb[q] = *(const bf16x8*)(S + b_rd + q * 2048);
        else if (q < 10) na[q - 4] = *(const bf16x8*)(S + a_rd + (q - 4) * 2048);
        else if (FIRST) {
          if (q < 16) glds16_s(ab, a_off[q - 10], base + (q - 10) * 4096);
          else if (q < 20) glds16_s(wb, w_off[q - 16], base + A_BYTES + (q - 16) * 4096);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      __builtin_amdgcn_s_setprio(0);
      if (FIRST) advance(); else rslot = nslot;
    };
    for (int kt = 0; kt < nt; ++kt) {
      step(std::true_type{}, af0, bf0, af1, bf1);
      step(std::false_type{}, af1, bf1, af0, bf0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // the surplus groups: no DMA may be in flight into LDS at the end
  }

  char* Cb = (char*)p.C;
  if (p.splits > 1) Cb += (long)z * p.slab_stride * 4;
  const bool wide = p.wide != 0;
  const float2* lut = stage_gelu_lut<ACT, 256>(smem, p, tid, true);
  if (res_init) epilogue_tile<6, 4, ACT, OUT_BF16, false>(acc, p, Cb, m0 + wm * 96 + l15, Mact, rbase, n0 + wn * 64, g, wide, biasp, lut);
  else epilogue_tile<6, 4, ACT, OUT_BF16, HAS_RES, ((HAS_RES && !OUT_BF16) ? 3 : 2)>(acc, p, Cb, m0 + wm * 96 + l15, Mact, rbase, n0 + wn * 64, g, wide, biasp, lut);   // one wave per SIMD: registers to spare
}

// ---- optional in-situ timing of every GEMM launch (bench.py's roofline leg): HIP events recorded on the
//      launch stream around the kernel, summed after the fact.  Off by default (zero overhead).
#include <vector>
namespace {
struct ProfRec { hipEvent_t a, b; double flops; };
bool g_prof_on = false;
std::vector<ProfRec> g_prof;
// ta_profile_gemm(2): a log of every launch's shape, epilogue and chosen tile (no events): the step-shape parity test replays it
#define TA_GEMM_LOG_FIELDS 24
bool g_log_on = false;
std::vector<long> g_log;
}  // namespace

#include <cstdlib>
// The two environment knobs of the GEMM launcher, read ONCE (round 4: they were 17 getenv calls PER LAUNCH).
// ta_gemm_reload_knobs() re-reads the environment: tests and the A/B scripts that switch a knob between launches call it
// (tiny_audio_amd/ops.py does so when it sees one of them change).
struct GemmKnobs {
  int variant;    // TA355_GEMM_VARIANT: force one tile variant; -1 = the model's choice
  int gelu_erf;   // TA355_GELU_LUT=0: arithmetic erf-GELU instead of the chord table (the tests compare both)
  void load() {
    auto i = [](const char* n, int d) { const char* v = getenv(n); return (v && *v) ? atoi(v) : d; };
    variant = i("TA355_GEMM_VARIANT", -1);
    gelu_erf = i("TA355_GELU_LUT", 1) == 0;
  }
};
static GemmKnobs& knobs() {
  static GemmKnobs k = [] { GemmKnobs x; x.load(); return x; }();
  return k;
}
void ta_i_reload_decode_knobs();   // generate.hip: TA355_DECODE_FUSED
extern "C" int ta_gemm_reload_knobs(void) { knobs().load(); ta_i_reload_decode_knobs(); return TA_OK; }

// ---- the tile variants.  The library carries the variants the launch-time model can choose; everything a variant number means is
// its row here.  Rounds 1-5 also had the plain double-buffered 256x256 / 256x128 tiles (1 / 2: rates 0.9 / 0.5, never the model's
// choice -- variant 3 has 1's tile and slots at a higher rate, and 128x128 has no more rounds than 2 at half the cost per round) and, in
// experiment builds, the ring form (6 / 7), stamped timing builds (8 / 9), the 32x32x16 form of v5 (11) and v5's timing experiments: all
// removed (git, scripts/attic/gemm_r05_with_experiments.hip.txt and profiles/ keep sources and measurements; DESIGN.md "dead ends").
// Model: time ~ rounds(tiles / resident slots) * tile area / relative rate * tiles per CU; pick the cheapest (the first of equals, in
// table order).  The relative rates come from scripts/gemm_bench.py on MI355X (see profiles/).  TA355_GEMM_VARIANT forces one
// (tests, microbenchmarks); a number the library does not carry means the model's choice.
enum : unsigned { V_GATHER = 1, V_FAR_A = 2, V_KEXT = 4, V_WBLOCKED = 8 };   // what a launch may need: gathered A rows, row-mapped A beyond 32-bit offsets, the K extension, blocked W
// What the persistent kernel (v4) does not take.  Gathered A rows (their offsets are not bounded by the tile) and far row-mapped A.
// And the K extension (LoRA): its first persistent form hoisted the extension's nine DMA offsets out of
// the tile loop and spilled the regular ones (91.8 against 61.6 us per launch, profiles/r03_p_ab_lora.txt); with the offsets derived
// from a fresh thread index at the switch there was no scratch and the LoRA step was the same on both kernels (45.45 ms each,
// profiles/r03_r_ab_lora_persist_kext.txt), so v4 carries no extension.
constexpr unsigned V_NOT_PERSISTENT = V_GATHER | V_FAR_A | V_KEXT;
struct Variant {
  int id, bm, bn;      // TA355_GEMM_VARIANT / launch-log number; tile rows, columns
  int slots, per_cu;   // resident tiles on the chip; tiles a CU runs concurrently (a round costs per_cu tile areas per CU)
  double rate;         // per-CU throughput per unit tile area relative to the 128x128 kernel (gemm_common.h); <= 0: never chosen
  int min_k;           // the model chooses it only for K / splits >= min_k
  bool v2;             // persistent workgroups (v4), and one workgroup per tile (v2) for a launch with one of V_NOT_PERSISTENT
  unsigned cannot;     // what no form of the variant takes: such a launch goes to `fallback`
  int fallback;
};
constexpr Variant kVariants[] = {
    {0, 128, 128, 512, 2, 1.0, 0, false, 0, 0},                                          // 4 waves, 2 WG / CU (gemm_nt_kernel)
    {3, 256, 256, 256, 1, TA355_RATE_256x256_PP, 0, true, 0, 3},
    // N = 1280 / 3840 / 5120 divide exactly: M = 16000 x N = 1280 is 252 tiles = ONE round of 256 CUs
    {4, 256, 320, 256, 1, TA355_RATE_256x320_PP, 0, true, 0, 4},
    {5, 96, 128, 512, 2, TA355_RATE_96x128, 0, false, 0, 5},                             // the same kernel as 0
    // one 4-wave workgroup per CU (v5): no gather, plain W only.  Only long contractions: with one workgroup per CU nothing overlaps
    // its prologue and epilogue (K = 1280: 33 vs 28 us for 96x128)
    {10, 192, 128, 256, 1, TA355_RATE_192x128, 2048, false, V_GATHER | V_FAR_A | V_WBLOCKED, 5},
    // the 192-row ping-pong tile exists in the persistent form only: what that form does not take goes to the 256x256 tile.
    // (a minimum contraction length -- two K tiles -- so that tiny-K launches stay on the small tiles)
    {12, 192, 256, 256, 1, TA355_RATE_192x256_PP, 128, false, V_NOT_PERSISTENT, 3},
};
constexpr const Variant* find_variant(int id) {
  for (const Variant& v : kVariants)
    if (v.id == id) return &v;
  return nullptr;
}
constexpr bool fallbacks_take_everything() {
  for (const Variant& v : kVariants) {
    const Variant* f = find_variant(v.fallback);
    if (!f || (v.cannot && f->cannot)) return false;
  }
  return true;
}
static_assert(fallbacks_take_everything(), "a launch a variant cannot take must end at a row that takes it");

static const Variant& pick_variant(int M, int N, int K, int splits) {
  if (const Variant* forced = find_variant(knobs().variant)) return *forced;
  const Variant* best = &kVariants[0]; double best_t = 1e300;
  for (const Variant& v : kVariants) {
    if (v.rate <= 0.0 || K / splits < v.min_k) continue;
    const long tiles = (long)ta_cdiv(M, v.bm) * ta_cdiv(N, v.bn) * splits;
    const double rounds = (double)((tiles + v.slots - 1) / v.slots);
    const double t = rounds * (double)v.bm * v.bn / v.rate * (double)v.per_cu;
    if (t < best_t) { best_t = t; best = &v; }
  }
  // (Rounds 4-5 built two more kernel families on these tiles and removed them from the library after measuring them slower in the step:
  // gemm_v7 -- one 4-wave workgroup per CU, one wave per SIMD, 256 AGPR accumulators, 4-stage BK = 32 ring -- and its round-5
  // two-workgroups-per-CU form on 128x256 / 256x128 tiles; a 32x32x16 form (gemm_v8).  Sources: scripts/attic/; measurements:
  // profiles/r04_a/e_*, profiles/r05_b_gemm_2wg_*)
  return *best;
}

// The variant -> kernel map.  persist: the ping-pong variants 3 / 4 as persistent workgroups (v4, grid = one workgroup per CU at most)
// instead of one workgroup per tile (v2); variant 12 exists in the persistent form only.  Only rows of kVariants arrive here.
template <int ACT, bool OUT_BF16, bool HAS_RES, bool KEXT>
static void launch_variant(const Variant& v, bool persist, int grid, int pgrid, const GemmArgs& a, hipStream_t st) {
  switch (v.id) {
    case 0: TA_LAUNCH((gemm_nt_kernel<ACT, OUT_BF16, HAS_RES, 128, KEXT>), dim3(grid), dim3(256), 0, st, a); break;
    case 5: TA_LAUNCH((gemm_nt_kernel<ACT, OUT_BF16, HAS_RES, 96, KEXT>), dim3(grid), dim3(256), 0, st, a); break;
    case 3:
      if (persist) TA_LAUNCH((gemm_nt_kernel_v4<256, ACT, OUT_BF16, HAS_RES>), dim3(pgrid), dim3(512), 0, st, a);
      else TA_LAUNCH((gemm_nt_kernel_v2<256, ACT, OUT_BF16, HAS_RES, KEXT>), dim3(grid), dim3(512), 0, st, a);
      break;
    case 4:
      if (persist) TA_LAUNCH((gemm_nt_kernel_v4<320, ACT, OUT_BF16, HAS_RES>), dim3(pgrid), dim3(512), 0, st, a);
      else TA_LAUNCH((gemm_nt_kernel_v2<320, ACT, OUT_BF16, HAS_RES, KEXT>), dim3(grid), dim3(512), 0, st, a);
      break;
    case 10: TA_LAUNCH((gemm_nt_kernel_v5<ACT, OUT_BF16, HAS_RES, KEXT>), dim3(grid), dim3(256), 0, st, a); break;
    case 12: TA_LAUNCH((gemm_nt_kernel_v4<256, ACT, OUT_BF16, HAS_RES, 192>), dim3(pgrid), dim3(512), 0, st, a); break;
  }
}

template <int ACT, bool OUT_BF16, bool HAS_RES>
static int launch_gemm(GemmArgs a, hipStream_t st) {
  if (a.A2 && ACT != 0) return TA_ERR_ARG;          // the K extension exists for plain linears only (LoRA)
  const bool a_far = !a.a_plain && ((long)(a.M / a.a_rpb + 1) * a.a_bs + a.lda * a.a_rpb) * 2 >= (1L << 32);   // row-mapped A is addressed from its start with 32-bit offsets
  const unsigned needs = (a.a_idx ? V_GATHER : 0u) | (a_far ? V_FAR_A : 0u) | (a.A2 ? V_KEXT : 0u) | (a.w_blocked ? V_WBLOCKED : 0u);
  const Variant* vp = &pick_variant(a.M, a.N, a.K, a.splits);
  while (vp->cannot & needs) vp = find_variant(vp->fallback);      // (10 -> 5, 12 -> 3: rows that take everything)
  const Variant& v = *vp;
  // rows-grouped launch: every group may end in a partial M tile, so the tile grid is an upper bound (surplus tiles exit)
  a.tiles_m = ta_cdiv(a.M, v.bm) + ((a.grp_n > 0 && a.seg) ? a.grp_n : 0); a.tiles_n = ta_cdiv(a.N, v.bn);
  const int grid = a.tiles_m * a.tiles_n * a.splits;
  // few M-tiles (LM head): one group, W panels read once per XCD; otherwise the kernel's own group height.
  // (Round 3, measured and not kept: groups of 16 row tiles instead of 4 for the 12 column tiles of 320 of the encoder's q | k | v GEMM
  // -- an XCD's round is then 16 row tiles x 2 column tiles.  Cold operands (profiles/r03_c_gemm_enc_groupm_cold.txt): 146.3 us against
  // 153.9 (g = 8: 148.1); N = 5120 / 1280 shapes are flat in g; in the STEP 42.85 vs 42.79 ms (profiles/r03_d_ab_groupm.txt).)
  a.group_m = (v.id != 0 && a.tiles_m <= 8) ? a.tiles_m : 0;
  a.wide = (((long)a.N | a.ldc | a.c_off | a.c_bs) & 7) == 0;
  a.gelu_erf = knobs().gelu_erf;
  // (variant 12 is always persistent; `persist`, which the launch log records, says which form variants 3 / 4 take)
  const bool persist = v.v2 && !(needs & V_NOT_PERSISTENT);
  static const int ncu = [] { int dev = 0, n = 0; (void)hipGetDevice(&dev); (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev); return n > 0 ? n : 256; }();
  const int pgrid = grid < ncu ? grid : ncu;
  ProfRec r;
  if (g_prof_on) {
    if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) return TA_ERR_LAUNCH;
    r.flops = 2.0 * (double)a.M * (double)a.N * (double)a.K;
    (void)hipEventRecord(r.a, st);
  }
  if constexpr (ACT == 0) {
    if (a.A2) launch_variant<ACT, OUT_BF16, HAS_RES, true>(v, persist, grid, pgrid, a, st);
  }
  if (!a.A2) launch_variant<ACT, OUT_BF16, HAS_RES, false>(v, persist, grid, pgrid, a, st);
  if (g_prof_on) { (void)hipEventRecord(r.b, st); g_prof.push_back(r); }
  if (g_log_on) {
    const long flags = (a.a_idx ? 1 : 0) | (a.seg ? 2 : 0) | (a.krange ? 4 : 0) | (a.A2 ? 8 : 0) | (a.w_blocked ? 16 : 0) | (a.grp_n > 0 ? 32 : 0) |
                       (a.a_plain ? 256 : 0) | (a.c_plain ? 512 : 0);
    const long rec[TA_GEMM_LOG_FIELDS] = {a.M, a.N, a.K, a.lda, a.a_rpb, a.a_bs, a.ldc, a.c_rpb, a.c_bs, a.c_off, ACT, OUT_BF16 ? 1 : 0,
                                          HAS_RES ? 1 : 0, a.res_bf16, a.bias ? 1 : 0, a.splits, a.rope_cols, a.rope_rows, flags, a.K2, v.id,
                                          a.grp_n, 0, persist ? 1 : 0};
    g_log.insert(g_log.end(), rec, rec + TA_GEMM_LOG_FIELDS);
  }
  TA_CHECK_LAUNCH();
  return TA_OK;
}

// (act, out_bf16, residual) -> the instantiation.  ACT 2 (rope) exists only as <2, true, false> (the entry point has refused the rest),
// an unknown act is an argument error
static int dispatch_gemm(int act, bool out_bf16, bool has_res, const GemmArgs& a, hipStream_t st) {
  int rc = TA_ERR_ARG;
  with_const<0, 1, 2>(act, [&](auto act_c) {
    with_bool(out_bf16, [&](auto ob) {
      with_bool(has_res, [&](auto hr) {
        constexpr int ACT = decltype(act_c)::value;
        if constexpr (ACT != 2 || (decltype(ob)::value && !decltype(hr)::value)) rc = launch_gemm<ACT, decltype(ob)::value, decltype(hr)::value>(a, st);
      });
    });
  });
  return rc;
}

extern "C" int ta_profile_gemm(int enable) {
  g_prof_on = enable == 1;
  g_log_on = enable == 2;
  if (enable == 2) g_log.clear();
  return TA_OK;
}
// the launches logged since ta_profile_gemm(2): rows of 24 longs {M, N, K, lda, a_rpb, a_bs, ldc, c_rpb, c_bs, c_off, act (the epilogue
// instantiation: 0 none, 1 GELU, 2 rope), out_bf16, has_residual, residual_bf16,
// has_bias, splits, rope_cols, rope_rows, flags (1 gather, 2 segments, 4 K range, 8 K extension, 16 blocked W, 32 grouped,
// 256 / 512 identity A / C row map), K2, tile variant as launched, groups, 0 (reserved),
// persistent}.  Returns the number of rows (at most max_rows are written; out may be NULL to count).
extern "C" long ta_profile_gemm_log(long* out, long max_rows) {
  const long n = (long)(g_log.size() / TA_GEMM_LOG_FIELDS);
  if (out)
    for (long i = 0; i < n && i < max_rows; ++i)
      for (int f = 0; f < TA_GEMM_LOG_FIELDS; ++f) out[i * TA_GEMM_LOG_FIELDS + f] = g_log[i * TA_GEMM_LOG_FIELDS + f];
  return n;
}
// sums (and clears) the recorded launches: total kernel milliseconds, total algorithmic flops (2*M*N*K), launch count
extern "C" int ta_profile_gemm_collect(double* total_ms, double* total_flops, long* launches) {
  double ms = 0.0, fl = 0.0;
  for (auto& r : g_prof) {
    float t = 0.f;
    if (hipEventSynchronize(r.b) != hipSuccess || hipEventElapsedTime(&t, r.a, r.b) != hipSuccess) return TA_ERR_LAUNCH;
    ms += t; fl += r.flops;
    (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b);
  }
  if (total_ms) *total_ms = ms;
  if (total_flops) *total_flops = fl;
  if (launches) *launches = (long)g_prof.size();
  g_prof.clear();
  return TA_OK;
}

// ----------------------------------------------------------------------------- C-ABI (see include/ta355.h)
extern "C" int ta_gemm_bf16_nt(const void* A, const void* W, void* C, int M, int N, int K,
                               long lda, int a_rpb, long a_bs,
                               long ldc, int c_rpb, long c_bs, long c_off,
                               const float* bias, const float* residual,
                               int act, int out_bf16, int splits, float* splitk_ws, hipStream_t st) {
  return ta_gemm_bf16_nt_opt(A, W, C, M, N, K, lda, a_rpb, a_bs, ldc, c_rpb, c_bs, c_off, bias, residual, act, out_bf16,
                             splits, splitk_ws, nullptr, nullptr, nullptr, nullptr, st);
}
extern "C" int ta_gemm_bf16_nt_ex(const void* A, const void* W, void* C, int M, int N, int K, long lda, int a_rpb, long a_bs,
                                  long ldc, int c_rpb, long c_bs, long c_off, const float* bias, const float* residual,
                                  int act, int out_bf16, int splits, float* splitk_ws, const int* a_idx, const int* seg,
                                  const int* krange, hipStream_t st) {
  return ta_gemm_bf16_nt_opt(A, W, C, M, N, K, lda, a_rpb, a_bs, ldc, c_rpb, c_bs, c_off, bias, residual, act, out_bf16,
                             splits, splitk_ws, a_idx, seg, krange, nullptr, st);
}

// M is the UPPER BOUND on rows when `seg` is given (grid sizing); the kernel reads the actual base/count on device.
extern "C" int ta_gemm_bf16_nt_opt(const void* A, const void* W, void* C, int M, int N, int K,
                                   long lda, int a_rpb, long a_bs,
                                   long ldc, int c_rpb, long c_bs, long c_off,
                                   const float* bias, const float* residual,
                                   int act, int out_bf16, int splits, float* splitk_ws,
                                   const int* a_idx, const int* seg, const int* krange, const ta_gemm_opts* opts,
                                   hipStream_t st) {
  static const ta_gemm_opts none = {nullptr, nullptr, 0, 0, nullptr, nullptr, 0, 0, 0};
  const ta_gemm_opts& o = opts ? *opts : none;
  const void* resb = o.residual_bf16;
  if (resb) { if (residual) return TA_ERR_ARG; residual = (const float*)resb; }
  const void *xA2 = o.a2, *xW2 = o.w2;
  const int xK2 = o.a2 ? o.k2 : 0;
  if (o.a2 && (o.k2 <= 0 || o.k2 % BK || o.lda2 % 8 || !o.w2)) return TA_ERR_ARG;
  if (M <= 0 || N <= 0 || K <= 0) return TA_OK;
  if ((a_idx || seg || krange) && splits > 1) return TA_ERR_ARG;
  if ((K % BK) != 0 || (N % 4) != 0 || (lda % 8) != 0 || (a_bs % 8) != 0 || (ldc % 4) != 0 ||
      (c_off % 4) != 0 || (c_bs % 4) != 0)
    return TA_ERR_ARG;
  GemmArgs a;                                        // (what is not set here keeps its default: gemm_common.h)
  a.A = (const bf16_t*)A; a.W = (const bf16_t*)W; a.C = C; a.bias = bias; a.res = residual;
  a.M = M; a.N = N; a.K = K;
  a.lda = lda; a.a_rpb = a_rpb > 0 ? a_rpb : M; a.a_bs = a_bs;
  a.ldc = ldc; a.c_rpb = c_rpb > 0 ? c_rpb : (seg ? 0x7fffffff : M); a.c_bs = c_bs; a.c_off = c_off;
  if (seg && a_rpb <= 0) a.a_rpb = 0x7fffffff;
  a.a_plain = (a.a_rpb >= M && (!seg || a.a_rpb == 0x7fffffff)) ? 1 : 0;       // rows < a_rpb: quotient 0, remainder = row
  a.c_plain = (a.c_rpb >= M && (!seg || a.c_rpb == 0x7fffffff)) ? 1 : 0;
  a.a_idx = a_idx; a.seg = seg; a.krange = krange;
  a.A2 = (const bf16_t*)xA2; a.W2 = (const bf16_t*)xW2; a.K2 = xK2; a.lda2 = o.lda2;
  a.res_bf16 = resb != nullptr;
  a.rope_tab = o.rope_tab; a.rope_rows = o.rope_rows; a.rope_cols = o.rope_cols > 0 ? o.rope_cols : N;
  a.w_blocked = o.w_blocked ? 1 : 0;
  if (a.w_blocked && ((N & 63) || xA2 || krange || a_idx)) return TA_ERR_ARG;
  if (act == 2 && (!o.rope_tab || o.rope_rows <= 0 || !out_bf16 || residual || splits > 1 || (N % 64) || o.rope_cols < 0 || (o.rope_cols % 64))) return TA_ERR_ARG;
  if (resb && splits > 1) return TA_ERR_ARG;
  if (a.A2 && (splits > 1 || krange)) return TA_ERR_ARG;
  a.splits = splits > 1 ? splits : 1;
  if (a.splits > K / BK) a.splits = K / BK;
  a.slab_stride = (long)M * N;
  if (a.splits > 1) {
    // partial slabs are plain [M, N] f32; the epilogue (none) is applied by the reduce.
    if (!splitk_ws || act != 0 || bias || a.c_rpb != M || ldc != N || c_off != 0) return TA_ERR_ARG;
    GemmArgs s = a;
    s.C = splitk_ws; s.res = nullptr; s.bias = nullptr;
    int rc = launch_gemm<0, false, false>(s, st);
    if (rc) return rc;
    const long n4 = (long)M * N / 4;
    int blocks = (int)((n4 + 255) / 256); if (blocks > 2048) blocks = 2048;
    TA_LAUNCH(splitk_reduce_kernel, dim3(blocks), dim3(256), 0, st, (const float*)splitk_ws,
                       a.splits, a.slab_stride, residual, out_bf16 ? nullptr : (float*)C,
                       out_bf16 ? (bf16_t*)C : nullptr, n4);
    TA_CHECK_LAUNCH();
    return TA_OK;
  }
  return dispatch_gemm(act, out_bf16 != 0, residual != nullptr, a, st);
}


// ---- grouped launches (MoE experts): see GemmArgs.grp_n and include/ta355.h
extern "C" int ta_gemm_bf16_nt_grouped(const void* A, const void* W, void* C, int M, int N, int K, const float* bias, int act,
                                       int out_bf16, const int* a_idx, const int* seg, const int* krange, int n_groups,
                                       long w_stride, long c_stride, hipStream_t st) {
  if (M <= 0 || N <= 0 || K <= 0 || n_groups <= 0) return TA_OK;
  if (n_groups > 8 || (seg != nullptr) == (krange != nullptr) || (K % BK) || (N % 4) || (w_stride % 8) || (c_stride % 4)) return TA_ERR_ARG;
  if (krange && (out_bf16 || bias || act || a_idx || w_stride)) return TA_ERR_ARG;      // K-slice form: plain f32 products
  if (act != 0 && act != 1) return TA_ERR_ARG;
  GemmArgs a;                                        // plain operands, identity row maps: the defaults
  a.A = (const bf16_t*)A; a.W = (const bf16_t*)W; a.C = C; a.bias = bias;
  a.M = M; a.N = N; a.K = K;
  a.lda = K; a.ldc = N;
  a.a_idx = a_idx; a.seg = seg; a.krange = krange;
  a.grp_n = n_groups; a.grp_w_stride = w_stride;
  a.splits = krange ? n_groups : 1;           // K-slice form: z = group, slabs c_stride apart
  a.slab_stride = krange ? c_stride : (long)M * N;
  return dispatch_gemm(act, out_bf16 != 0, false, a, st);
}

extern "C" long ta_gemm_splitk_ws_bytes(int M, int N, int splits) {
  return splits > 1 ? (long)M * N * 4 * splits : 0;
}
