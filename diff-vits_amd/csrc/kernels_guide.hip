// Classifier-free guidance around one denoiser evaluation of the sampler loop (reference sampler/dpm_solver.py:322-330,
// sampler/uni_pc.py:221-229):  x_in = cat([x] * 2), c_in = cat([uncond, cond]), noise_u + g (noise_c - noise_u).
//
// The network predicts x0 and the guided noise is linear in the two predictions,
//     noise_u + g (noise_c - noise_u) = (x - alpha (x0_u + g (x0_c - x0_u))) / sigma,
// so the combination happens on x0 and the plan's history slot receives the guided data prediction directly (the x0 -> noise
// -> x0 round trip is not replayed: sampler.hip).  Two launches per evaluation:
//   k_cfg_pair_in   in [rows, n] -> out [2 rows, n]: rows 0 .. rows-1 and rows .. 2 rows - 1 are both `in` (the unconditional
//                   half first, as the reference orders it).  Also used once per run for the channel-concat condition.
//   k_cfg_combine   pair [2 rows, n] -> out [rows, n]:  u = row b, c = row b + rows,  d = c - u,  out = fmaf(g, d, u)
// Both are elementwise over the flat rows * n floats: a float4 body on the 16-byte aligned middle of the DESTINATION, the (up
// to 3 + 3) elements before and behind it one by one; a source whose address has another 4-byte phase than the destination -
// the second half of a pair when rows * n is no multiple of 4, a caller's unaligned view - is read float by float.  No scratch,
// no atomics; every element is written by exactly one thread.
#include "dv_common.h"

namespace {

constexpr int CFG_THREADS = 256;
constexpr int CFG_MAX_WGS = 2048;

// floats in front of the first 16-byte boundary at or behind p (0..3), capped at n
__device__ __forceinline__ int64_t cfg_head(const float* p, int64_t n) {
  const int64_t h = (int64_t)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2);
  return h < n ? h : n;
}

__device__ __forceinline__ float4 cfg_load4(const float* p, bool aligned) {
  if (aligned) return *reinterpret_cast<const float4*>(p);
  return make_float4(p[0], p[1], p[2], p[3]);
}

__device__ __forceinline__ float cfg_mix(float u, float c, float g) { return fmaf(g, __fsub_rn(c, u), u); }

// blockIdx.y = 0 / 1: the half of `out` this workgroup writes
__global__ __launch_bounds__(CFG_THREADS) void k_cfg_pair_in(const float* __restrict__ in, float* __restrict__ out, int64_t n) {
  float* dst = out + (int64_t)blockIdx.y * n;
  const int64_t head = cfg_head(dst, n), n4 = (n - head) / 4, tail = n - head - n4 * 4;
  const float* src = in + head;
  const bool src_al = ((uintptr_t)src & 15u) == 0;
  float4* d4 = reinterpret_cast<float4*>(dst + head);
  for (int64_t i = (int64_t)blockIdx.x * CFG_THREADS + threadIdx.x; i < n4; i += (int64_t)gridDim.x * CFG_THREADS)
    d4[i] = cfg_load4(src + i * 4, src_al);
  if (blockIdx.x == 0) {
    const int t = threadIdx.x;
    if (t < head) dst[t] = in[t];
    if (t < tail) dst[head + n4 * 4 + t] = in[head + n4 * 4 + t];
  }
}

// u = pair[0 .. n), c = pair[n .. 2 n)
__global__ __launch_bounds__(CFG_THREADS) void k_cfg_combine(const float* __restrict__ pair, float* __restrict__ out, int64_t n, float g) {
  const float* u = pair;
  const float* c = pair + n;
  const int64_t head = cfg_head(out, n), n4 = (n - head) / 4, tail = n - head - n4 * 4;
  const bool u_al = ((uintptr_t)(u + head) & 15u) == 0, c_al = ((uintptr_t)(c + head) & 15u) == 0;
  float4* o4 = reinterpret_cast<float4*>(out + head);
  for (int64_t i = (int64_t)blockIdx.x * CFG_THREADS + threadIdx.x; i < n4; i += (int64_t)gridDim.x * CFG_THREADS) {
    const float4 a = cfg_load4(u + head + i * 4, u_al), b = cfg_load4(c + head + i * 4, c_al);
    o4[i] = make_float4(cfg_mix(a.x, b.x, g), cfg_mix(a.y, b.y, g), cfg_mix(a.z, b.z, g), cfg_mix(a.w, b.w, g));
  }
  if (blockIdx.x == 0) {
    const int t = threadIdx.x;
    if (t < head) out[t] = cfg_mix(u[t], c[t], g);
    if (t < tail) { const int64_t e = head + n4 * 4 + t; out[e] = cfg_mix(u[e], c[e], g); }
  }
}

int cfg_grid(int64_t n) {
  const int64_t wgs = (n / 4 + CFG_THREADS - 1) / CFG_THREADS;
  return (int)(wgs < 1 ? 1 : (wgs > CFG_MAX_WGS ? CFG_MAX_WGS : wgs));
}

}  // namespace

hipError_t launch_cfg_pair_in(const float* in, float* out, int64_t n, hipStream_t st) {
  if (!in || !out || n < 1 || (((uintptr_t)in | (uintptr_t)out) & 3u)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cfg_pair_in, dim3(cfg_grid(n), 2), dim3(CFG_THREADS), 0, st, in, out, n);
  return hipGetLastError();
}

hipError_t launch_cfg_combine(const float* pair, float* out, int64_t n, float g, hipStream_t st) {
  if (!pair || !out || n < 1 || (((uintptr_t)pair | (uintptr_t)out) & 3u)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cfg_combine, dim3(cfg_grid(n)), dim3(CFG_THREADS), 0, st, pair, out, n, g);
  return hipGetLastError();
}
