// ta355 -- the register sub-transforms of the 400-point mixed-radix FFT (400 = 16 x 25 = (4 x 4) x (5 x 5)), f32 on the VALU.
// Shared by the Whisper-style log-mel front end (logmel.hip) and the ECAPA-TDNN filter bank (ecapa.hip).
#pragma once
#include "common.h"
#include "logmel_twiddles.h"
struct cpx { float re, im; };
__device__ __forceinline__ cpx cmul(cpx a, float wr, float wi) { return {a.re * wr - a.im * wi, a.re * wi + a.im * wr}; }
__device__ __forceinline__ void dft4(const cpx a0, const cpx a1, const cpx a2, const cpx a3, cpx& o0, cpx& o1, cpx& o2, cpx& o3) {
  const cpx s02 = {a0.re + a2.re, a0.im + a2.im}, d02 = {a0.re - a2.re, a0.im - a2.im};
  const cpx s13 = {a1.re + a3.re, a1.im + a3.im}, d13 = {a1.re - a3.re, a1.im - a3.im};
  o0 = {s02.re + s13.re, s02.im + s13.im};
  o2 = {s02.re - s13.re, s02.im - s13.im};
  o1 = {d02.re + d13.im, d02.im - d13.re};          // d02 - i d13
  o3 = {d02.re - d13.im, d02.im + d13.re};          // d02 + i d13
}
__device__ __forceinline__ void dft5(const cpx x0, const cpx x1, const cpx x2, const cpx x3, const cpx x4, cpx& o0, cpx& o1, cpx& o2,
                                     cpx& o3, cpx& o4) {
  const cpx t1 = {x1.re + x4.re, x1.im + x4.im}, t2 = {x2.re + x3.re, x2.im + x3.im};
  const cpx t3 = {x1.re - x4.re, x1.im - x4.im}, t4 = {x2.re - x3.re, x2.im - x3.im};
  o0 = {x0.re + t1.re + t2.re, x0.im + t1.im + t2.im};
  const cpx m1 = {x0.re + R5_C1 * t1.re + R5_C2 * t2.re, x0.im + R5_C1 * t1.im + R5_C2 * t2.im};
  const cpx m2 = {x0.re + R5_C2 * t1.re + R5_C1 * t2.re, x0.im + R5_C2 * t1.im + R5_C1 * t2.im};
  const cpx n1 = {R5_S1 * t3.re + R5_S2 * t4.re, R5_S1 * t3.im + R5_S2 * t4.im};
  const cpx n2 = {R5_S2 * t3.re - R5_S1 * t4.re, R5_S2 * t3.im - R5_S1 * t4.im};
  o1 = {m1.re + n1.im, m1.im - n1.re};              // m1 - i n1
  o4 = {m1.re - n1.im, m1.im + n1.re};              // m1 + i n1
  o2 = {m2.re + n2.im, m2.im - n2.re};
  o3 = {m2.re - n2.im, m2.im + n2.re};
}
// in-register 16-point FFT: n1 = 4p + q, k1 = r + 4s
__device__ __forceinline__ void fft16(cpx* a) {
  cpx u[4][4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    dft4(a[q], a[4 + q], a[8 + q], a[12 + q], u[q][0], u[q][1], u[q][2], u[q][3]);
#pragma unroll
    for (int r = 1; r < 4; ++r)
      if (q > 0) u[q][r] = cmul(u[q][r], W16Q_RE[q][r], W16Q_IM[q][r]);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) dft4(u[0][r], u[1][r], u[2][r], u[3][r], a[r], a[r + 4], a[r + 8], a[r + 12]);
}
// in-register 25-point FFT: n2 = 5p + q, k2 = r + 5s
__device__ __forceinline__ void fft25(cpx* y) {
  cpx u[5][5];
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    dft5(y[q], y[5 + q], y[10 + q], y[15 + q], y[20 + q], u[q][0], u[q][1], u[q][2], u[q][3], u[q][4]);
#pragma unroll
    for (int r = 1; r < 5; ++r)
      if (q > 0) u[q][r] = cmul(u[q][r], W25Q_RE[q][r], W25Q_IM[q][r]);
  }
#pragma unroll
  for (int r = 0; r < 5; ++r) dft5(u[0][r], u[1][r], u[2][r], u[3][r], u[4][r], y[r], y[r + 5], y[r + 10], y[r + 15], y[r + 20]);
}
