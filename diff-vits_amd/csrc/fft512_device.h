// The pieces the 1024-point real transforms share (kernels_mel.hip: forward, kernels_voc.hip: inverse): a 512-point complex
// FFT as three radix-8 passes over 64 lanes x 8 points, exchanged through LDS rows padded by one word per 8 (zpad), and the
// host-side builder of its twiddle tables (fp64 on the host, rounded once).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

__device__ __forceinline__ int zpad(int i) { return i + (i >> 3); }

// b_k = sum_j a_j exp(-2 pi i j k / 8), in place
__device__ __forceinline__ void dft8(float* __restrict__ r, float* __restrict__ i) {
  const float h = 0.70710678118654752440f;
  const float s0r = r[0] + r[4], s0i = i[0] + i[4], d0r = r[0] - r[4], d0i = i[0] - i[4];
  const float s1r = r[1] + r[5], s1i = i[1] + i[5], d1r = r[1] - r[5], d1i = i[1] - i[5];
  const float s2r = r[2] + r[6], s2i = i[2] + i[6], d2r = r[2] - r[6], d2i = i[2] - i[6];
  const float s3r = r[3] + r[7], s3i = i[3] + i[7], d3r = r[3] - r[7], d3i = i[3] - i[7];
  // even outputs: the 4-point transform of s
  const float t0r = s0r + s2r, t0i = s0i + s2i, t1r = s0r - s2r, t1i = s0i - s2i;
  const float t2r = s1r + s3r, t2i = s1i + s3i, t3r = s1r - s3r, t3i = s1i - s3i;
  r[0] = t0r + t2r; i[0] = t0i + t2i;
  r[4] = t0r - t2r; i[4] = t0i - t2i;
  r[2] = t1r + t3i; i[2] = t1i - t3r;            // t1 - i t3
  r[6] = t1r - t3i; i[6] = t1i + t3r;            // t1 + i t3
  // odd outputs: the 4-point transform of (d0, d1 W8, d2 W8^2, d3 W8^3)
  const float e1r = (d1r + d1i) * h, e1i = (d1i - d1r) * h;          // d1 (1 - i) / sqrt 2
  const float e2r = d2i, e2i = -d2r;                                 // -i d2
  const float e3r = (d3i - d3r) * h, e3i = (-d3r - d3i) * h;         // d3 (-1 - i) / sqrt 2
  const float u0r = d0r + e2r, u0i = d0i + e2i, u1r = d0r - e2r, u1i = d0i - e2i;
  const float u2r = e1r + e3r, u2i = e1i + e3i, u3r = e1r - e3r, u3i = e1i - e3i;
  r[1] = u0r + u2r; i[1] = u0i + u2i;
  r[5] = u0r - u2r; i[5] = u0i - u2i;
  r[3] = u1r + u3i; i[3] = u1i - u3r;
  r[7] = u1r - u3i; i[7] = u1i + u3r;
}

// tw512[t] = exp(-2 pi i t / 512), tw1024[t] = exp(-2 pi i t / 1024), t < 512 (host arrays)
inline void fft512_fill_tables(float2* tw512, float2* tw1024) {
  const double two_pi = 6.283185307179586476925286766559;
  for (int t = 0; t < 512; ++t) {
    tw512[t] = make_float2((float)std::cos(two_pi * t / 512.0), (float)-std::sin(two_pi * t / 512.0));
    tw1024[t] = make_float2((float)std::cos(two_pi * t / 1024.0), (float)-std::sin(two_pi * t / 1024.0));
  }
}
