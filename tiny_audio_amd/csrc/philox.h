// Philox4x32-10 (Salmon et al. 2011, "Parallel random numbers: as easy as 1, 2, 3"): a counter-based generator, so every
// draw is a pure function of (counter, key) and any thread can regenerate any draw without state.  Shared by the sampler
// (generate.hip), the LoRA dropout masks (lora.hip) and the Gaussian floor of the waveform augmentation (augment.hip).
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ uint4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return make_uint4(c0, c1, c2, c3);
}

// ---- LoRA dropout keep masks (peft LoraLayer: each adapted linear j applies its own nn.Dropout(p) to its input).
// The keep decision of element (m, c) of linear j (peft order q, k, v, o, gate, up, down = 0..6) in decoder layer l is
//   w   = philox4x32_10(counter = ((8 l + j) << 20 | c >> 3,  m,  lo32(offset),  hi32(offset)),  key = (lo32(seed), hi32(seed)))
//   u16 = 16-bit half (c & 1) (low half first) of word (c & 7) >> 1 of w
//   keep  <=>  u16 >= thr,   thr = round(p * 65536)
// i.e. one Philox call decides 8 consecutive columns, and the drop probability is p rounded to a multiple of 2^-16 (the
// kept values are scaled by 1 / (1 - p) with p as given, as peft does).  Nothing depends on the launch geometry: the
// backward regenerates the forward's masks instead of storing them.  Valid for in < 2^23 columns and l < 2^9 layers.
struct LoraDropDev {
  unsigned k0, k1, o0, o1;     // key = seed, counter words 2, 3 = offset
  unsigned thr;                // drop iff u16 < thr
  float inv_keep;              // 1 / (1 - p)
};
// 8-bit keep mask of columns [c8 * 8, c8 * 8 + 8) of row m, linear lj = 8 l + j (bit e = column c8 * 8 + e)
__device__ __forceinline__ unsigned lora_keep8(const LoraDropDev& d, unsigned lj, unsigned c8, unsigned m) {
  const uint4 w = philox4x32_10((lj << 20) | c8, m, d.o0, d.o1, d.k0, d.k1);
  const unsigned ws[4] = {w.x, w.y, w.z, w.w};
  unsigned bits = 0;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const unsigned u = (ws[e >> 1] >> ((e & 1) * 16)) & 0xffffu;
    bits |= (u >= d.thr ? 1u : 0u) << e;
  }
  return bits;
}

// ---- Gaussian floor of the waveform augmentation (augment.hip; audiomentations AddGaussianSNR).  The standard normal z[b, t] added
// to sample t of clip b is a pure function of (seed, offset, b, t):
//   w  = philox4x32_10(counter = (t >> 2,  b,  lo32(offset),  hi32(offset)),  key = (lo32(seed), hi32(seed)))
//   samples 4 q, 4 q + 1 come from (wa, wb) = (w.x, w.y), samples 4 q + 2, 4 q + 3 from (w.z, w.w), by Box-Muller:
//   u1 = ((wa >> 8) + 1) 2^-24  in (0, 1],   u2 = (wb >> 8) 2^-24  in [0, 1),   r = sqrt(-2 ln u1),
//   z  = r cos(2 pi u2),  r sin(2 pi u2)
// i.e. one Philox call gives 4 consecutive samples, |z| <= sqrt(48 ln 2) = 5.77.  logf / sincosf are the accurate ones (the product
// 2 pi u2 is rounded to f32 first).  Nothing depends on the launch geometry.  Valid for t < 2^34 and b < 2^32.
__device__ __forceinline__ void wave_normal4(const uint4 w, float z[4]) {
  const unsigned ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float u1 = (float)((ws[2 * h] >> 8) + 1u) * 5.9604644775390625e-8f, u2 = (float)(ws[2 * h + 1] >> 8) * 5.9604644775390625e-8f;
    const float r = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincosf(6.283185307179586f * u2, &sn, &cs);
    z[2 * h] = r * cs;
    z[2 * h + 1] = r * sn;
  }
}
