// Known-frame correction of the sampler state (mel infilling): after a step that lands at time t,
//     x[b, :, f] <- alpha_t * known[b, :, f] + sigma_t * eps[b, :, f]     where keep[b, f] != 0
//     x[b, :, f] unchanged (not written)                                   elsewhere
// x, known, eps [rows, C, T] fp32, keep [rows, T] one byte per frame (broadcast over the channels), in place on x.  It is the
// closed form of the correcting_xt_fn that holds a set of frames on the forward process of a known signal (reference
// sampler/dpm_solver.py:384-394, 1180-1238; sampler/uni_pc.py:615-666).  (alpha, sigma) are a row of the plan's table on the
// device, read like k_lincomb reads its row.  The value is fadd(fmul(alpha, known), fmul(sigma, eps)): the three float32
// roundings of the torch expression alpha * known + sigma * eps - no contraction into an fma.
//
// One launch, elementwise, memory-bound; no LDS, no atomics, every element is touched by exactly one thread.
//   T % 4 == 0 (and 16-byte aligned x / known / eps, 4-byte aligned keep): a thread owns four consecutive frames of one channel
//     row - one 4-byte load of their keep bytes; nothing else is read where all four are 0; known / eps as float4; a float4
//     store where all four are kept, single stores of the kept ones otherwise.  x is never read.
//   every other T or alignment: one element per thread and trip.
// (rows * C * T is a multiple of 4 whenever T is: the vector route has no tail.)
#include "dv_common.h"

#include <algorithm>

namespace {

constexpr int KNOWN_THREADS = 256;
constexpr int KNOWN_MAX_WGS = 2048;

// hipcc contracts a * k + s * e into an fma of one product (two roundings, not torch's three), through the rounded intrinsics and
// through `#pragma clang fp contract(off)` once the function is inlined: the empty asm makes both products values of their own.
__device__ __forceinline__ float known_mix(float a, float s, float k, float e) {
  float p = __fmul_rn(a, k), q = __fmul_rn(s, e);
  asm("" : "+v"(p), "+v"(q));
  return __fadd_rn(p, q);
}

// n4 = rows * C * T / 4 quads; T4 = T / 4 quads per channel row
__global__ __launch_bounds__(KNOWN_THREADS) void k_known_frames(float* __restrict__ x, const float* __restrict__ known,
                                                                const float* __restrict__ eps, const uint8_t* __restrict__ keep,
                                                                uint32_t n4, uint32_t C, uint32_t T4,
                                                                const float* __restrict__ coef2) {
  const float a = coef2[0], s = coef2[1];
  const uint32_t* keep4 = reinterpret_cast<const uint32_t*>(keep);
  for (uint32_t q = blockIdx.x * KNOWN_THREADS + threadIdx.x; q < n4; q += gridDim.x * KNOWN_THREADS) {
    const uint32_t rc = q / T4, f4 = q - rc * T4, b = rc / C;       // channel row, quad of frames in it, utterance
    const uint32_t m = keep4[b * T4 + f4];
    if (m == 0u) continue;
    const float4 k = reinterpret_cast<const float4*>(known)[q], e = reinterpret_cast<const float4*>(eps)[q];
    const float4 v = make_float4(known_mix(a, s, k.x, e.x), known_mix(a, s, k.y, e.y), known_mix(a, s, k.z, e.z), known_mix(a, s, k.w, e.w));
    const bool k0 = m & 0xFFu, k1 = m & 0xFF00u, k2 = m & 0xFF0000u, k3 = m & 0xFF000000u;
    if (k0 && k1 && k2 && k3) { reinterpret_cast<float4*>(x)[q] = v; continue; }
    float* o = x + (size_t)q * 4;
    if (k0) o[0] = v.x;
    if (k1) o[1] = v.y;
    if (k2) o[2] = v.z;
    if (k3) o[3] = v.w;
  }
}

__global__ __launch_bounds__(KNOWN_THREADS) void k_known_frames_scalar(float* __restrict__ x, const float* __restrict__ known,
                                                                       const float* __restrict__ eps, const uint8_t* __restrict__ keep,
                                                                       uint32_t n, uint32_t C, uint32_t T,
                                                                       const float* __restrict__ coef2) {
  const float a = coef2[0], s = coef2[1];
  for (uint32_t i = blockIdx.x * KNOWN_THREADS + threadIdx.x; i < n; i += gridDim.x * KNOWN_THREADS) {
    const uint32_t rc = i / T, f = i - rc * T, b = rc / C;
    if (keep[b * T + f]) x[i] = known_mix(a, s, known[i], eps[i]);
  }
}

}  // namespace

hipError_t launch_known_frames(float* x, const float* known, const float* eps, const uint8_t* keep, int rows, int C, int T,
                               const float* coef2, hipStream_t st) {
  if (!x || !known || !eps || !keep || !coef2 || rows < 1 || C < 1 || T < 1) return hipErrorInvalidValue;
  const int64_t n = (int64_t)rows * C * T;
  // (32-bit indices; the grid-stride increment must not wrap either)
  if (n > (int64_t)INT32_MAX || (((uintptr_t)x | (uintptr_t)known | (uintptr_t)eps | (uintptr_t)coef2) & 3u)) return hipErrorInvalidValue;
  const bool vec = T % 4 == 0 && ((((uintptr_t)x | (uintptr_t)known | (uintptr_t)eps) & 15u) == 0) && (((uintptr_t)keep & 3u) == 0);
  const int64_t work = vec ? n / 4 : n;
  const int blocks = (int)std::min<int64_t>((work + KNOWN_THREADS - 1) / KNOWN_THREADS, KNOWN_MAX_WGS);
  if (vec)
    hipLaunchKernelGGL(k_known_frames, dim3(blocks), dim3(KNOWN_THREADS), 0, st, x, known, eps, keep, (uint32_t)(n / 4), (uint32_t)C,
                       (uint32_t)(T / 4), coef2);
  else
    hipLaunchKernelGGL(k_known_frames_scalar, dim3(blocks), dim3(KNOWN_THREADS), 0, st, x, known, eps, keep, (uint32_t)n, (uint32_t)C,
                       (uint32_t)T, coef2);
  return hipGetLastError();
}
