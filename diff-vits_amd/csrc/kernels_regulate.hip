// Length regulator of the VITS prior at inference (reference model3.py:840-856: exp / ceil / sum / clamp on the durations,
// commons.generate_path, two matmuls of the one-hot alignment [B, T', Tx] against m_p / logs_p, the prior sample).  The alignment
// only picks one token's column for each output frame, so it is a prefix sum and a gather here; the [B, T', Tx] tensor never exists.
//
//   k_dur_scan         one workgroup per utterance:  w = expf(logw) * [j < x_len] * length_scale (fp32, the reference's order),
//                      d = (int)ceilf(w), cum[b, j] = d_0 + ... + d_j (inclusive), y_len[b] = max(cum[b, x_len - 1], 1).
//                      256-token chunks with a carry; inside a chunk a wave64 shuffle scan and one LDS step over the 4 waves.
//                      The sums are integers (the reference sums floats: exact below 2^24 only), 64-bit in registers so that an
//                      utterance whose total leaves int32 is recognised instead of wrapping.  A w that is not in [0, 2^24]
//                      (NaN and +-inf included) is never converted: the utterance is INVALID, y_len[b] = -1, its cum row is
//                      unspecified (finite integers), the other rows are untouched by it.
//   k_regulate_sample  one workgroup per (utterance, 256 output frames), lane = frame:  tok(t) = first j < x_len with
//                      cum[b, j] > t (binary search; the utterance's cum staged in LDS when Tx <= 1024, read from global memory
//                      otherwise; tokens of zero duration can never be the first above t), then over the channels
//                          z[b, c, t] = m_p[b, c, tok] + (noise[b, c, t] * expf(logs_p[b, c, tok])) * noise_scale
//                      rounded in that order.  A frame without a token (t >= cum[b, x_len - 1]: the padding up to Tp and the one
//                      frame of an utterance whose durations are all zero) has an all-zero alignment row in the reference, so
//                      m = logs = 0 there and z = 0 + (noise * 1) * noise_scale - not zeros.  The search is bounded by x_len
//                      whatever cum holds, so an INVALID row reads and writes inside its own slices only.
// Ordering is by kernel boundary alone; nothing allocates, waits or hands over inside a launch.
#include "../../include/dvits_hip.h"
#include "dv_common.h"

#include <cmath>

int dv_fail(int code, const char* fmt, ...);

namespace {

constexpr int REG_THREADS = 256;
constexpr int REG_WAVES = REG_THREADS / 64;
constexpr int REG_LDS_TX = 1024;          // the longest utterance whose cum row the sample kernel stages in LDS
constexpr float REG_MAX_W = 16777216.0f;  // 2^24

__device__ __forceinline__ int reg_clamp_len(int64_t l, int Tx) { return l < 0 ? 0 : (l > Tx ? Tx : (int)l); }

__global__ __launch_bounds__(REG_THREADS) void k_dur_scan(const float* __restrict__ logw, const int64_t* __restrict__ x_lengths,
                                                          int Tx, float length_scale, int32_t* __restrict__ cum,
                                                          int64_t* __restrict__ y_len) {
  __shared__ long long s_wave[REG_WAVES];
  __shared__ int s_bad;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int xl = reg_clamp_len(x_lengths[b], Tx);
  const float* lw = logw + (int64_t)b * Tx;
  int32_t* cb = cum + (int64_t)b * Tx;
  if (tid == 0) s_bad = 0;
  __syncthreads();
  long long carry = 0;
  bool bad = false;
  for (int base = 0; base < Tx; base += REG_THREADS) {
    const int j = base + tid;
    long long v = 0;
    if (j < Tx) {
      const float mask = j < xl ? 1.0f : 0.0f;
      const float w = __fmul_rn(__fmul_rn(expf(lw[j]), mask), length_scale);
      if (w >= 0.0f && w <= REG_MAX_W) v = (long long)(int)ceilf(w);   // the cast only ever sees 0 .. 2^24
      else bad = true;
    }
    // inclusive scan inside the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const long long up = __shfl_up(v, off, 64);
      if (lane >= off) v += up;
    }
    if (lane == 63) s_wave[wave] = v;
    __syncthreads();
    long long before = carry, total = carry;
#pragma unroll
    for (int k = 0; k < REG_WAVES; ++k) {
      const long long s = s_wave[k];
      if (k < wave) before += s;
      total += s;
    }
    v += before;
    if (v > (long long)INT32_MAX) { bad = true; v = INT32_MAX; }
    if (j < Tx) cb[j] = (int32_t)v;
    carry = total;
    __syncthreads();   // s_wave is rewritten by the next chunk
  }
  if (bad) s_bad = 1;
  __syncthreads();
  if (tid == 0) y_len[b] = s_bad ? (int64_t)-1 : (carry > 1 ? (int64_t)carry : (int64_t)1);
}

__global__ __launch_bounds__(REG_THREADS) void k_regulate_sample(const float* __restrict__ m_p, const float* __restrict__ logs_p,
                                                                 const int32_t* __restrict__ cum, const int64_t* __restrict__ x_lengths,
                                                                 const float* __restrict__ noise, float noise_scale, int C, int Tx, int Tp,
                                                                 float* __restrict__ z_p, float* __restrict__ m_exp,
                                                                 float* __restrict__ logs_exp) {
  __shared__ int32_t s_cum[REG_LDS_TX];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int t = blockIdx.x * REG_THREADS + tid;
  const int xl = reg_clamp_len(x_lengths[b], Tx);
  const int32_t* cb = cum + (int64_t)b * Tx;
  const bool staged = Tx <= REG_LDS_TX;     // uniform over the launch
  if (staged) {
    for (int j = tid; j < xl; j += REG_THREADS) s_cum[j] = cb[j];
    __syncthreads();
  }
  if (t >= Tp) return;
  int lo = 0, hi = xl;                      // first j in [0, xl) with cum[j] > t, or xl
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const int32_t cv = staged ? s_cum[mid] : cb[mid];
    if (cv > t) hi = mid; else lo = mid + 1;
  }
  const bool has = lo < xl;
  const int64_t src = (int64_t)b * C * Tx + lo, dst = (int64_t)b * C * Tp + t;
#pragma unroll 4
  for (int c = 0; c < C; ++c) {
    const float m = has ? m_p[src + (int64_t)c * Tx] : 0.0f;
    const float l = has ? logs_p[src + (int64_t)c * Tx] : 0.0f;
    const float n = noise[dst + (int64_t)c * Tp];
    z_p[dst + (int64_t)c * Tp] = __fadd_rn(m, __fmul_rn(__fmul_rn(n, expf(l)), noise_scale));
    if (m_exp) m_exp[dst + (int64_t)c * Tp] = m;
    if (logs_exp) logs_exp[dst + (int64_t)c * Tp] = l;
  }
}

}  // namespace

hipError_t launch_dur_scan(const float* logw, const int64_t* x_lengths, int B, int Tx, float length_scale, int32_t* cum,
                           int64_t* y_len, hipStream_t st) {
  if (!logw || !x_lengths || !cum || !y_len || B < 1 || Tx < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_dur_scan, dim3(B), dim3(REG_THREADS), 0, st, logw, x_lengths, Tx, length_scale, cum, y_len);
  return hipGetLastError();
}

hipError_t launch_regulate_sample(const float* m_p, const float* logs_p, const int32_t* cum, const int64_t* x_lengths,
                                  const float* noise, float noise_scale, int B, int C, int Tx, int Tp, float* z_p, float* m_exp,
                                  float* logs_exp, hipStream_t st) {
  if (!m_p || !logs_p || !cum || !x_lengths || !noise || !z_p || B < 1 || B > 65535 || C < 1 || Tx < 1 || Tp < 1 ||
      Tp > INT32_MAX - REG_THREADS)
    return hipErrorInvalidValue;
  const int blocks = (Tp + REG_THREADS - 1) / REG_THREADS;
  hipLaunchKernelGGL(k_regulate_sample, dim3(blocks, B), dim3(REG_THREADS), 0, st, m_p, logs_p, cum, x_lengths, noise, noise_scale, C,
                     Tx, Tp, z_p, m_exp, logs_exp);
  return hipGetLastError();
}

extern "C" int dv_op_regulate_lengths(const float* logw, const int64_t* x_lengths, int32_t B, int32_t Tx, double length_scale,
                                      int32_t* cum, int64_t* y_len, void* stream) {
  if (!logw || !x_lengths || !cum || !y_len) return dv_fail(DV_ERR_INVALID, "dv_op_regulate_lengths: null argument");
  if (B < 1 || Tx < 1) return dv_fail(DV_ERR_INVALID, "dv_op_regulate_lengths: B = %d, Tx = %d must be >= 1", B, Tx);
  if (!(length_scale >= 0.0) || !std::isfinite((float)length_scale))
    return dv_fail(DV_ERR_INVALID, "dv_op_regulate_lengths: length_scale %g must be finite and >= 0", length_scale);
  hipError_t e = launch_dur_scan(logw, x_lengths, B, Tx, (float)length_scale, cum, y_len, (hipStream_t)stream);
  if (e != hipSuccess) return dv_fail(DV_ERR_HIP, "dv_op_regulate_lengths: launch failed: %s", hipGetErrorString(e));
  return DV_OK;
}

extern "C" int dv_op_regulate_sample(const float* m_p, const float* logs_p, const int32_t* cum, const int64_t* x_lengths,
                                     const float* noise, double noise_scale, int32_t B, int32_t C, int32_t Tx, int32_t Tp,
                                     float* z_p, float* m_p_exp, float* logs_p_exp, void* stream) {
  if (!m_p || !logs_p || !cum || !x_lengths || !noise || !z_p) return dv_fail(DV_ERR_INVALID, "dv_op_regulate_sample: null argument");
  if (B < 1 || C < 1 || Tx < 1 || Tp < 1)
    return dv_fail(DV_ERR_INVALID, "dv_op_regulate_sample: B = %d, C = %d, Tx = %d, Tp = %d must be >= 1", B, C, Tx, Tp);
  if (B > 65535 || Tp > INT32_MAX - 256) return dv_fail(DV_ERR_INVALID, "dv_op_regulate_sample: B = %d exceeds 65535 or Tp = %d exceeds 2^31 - 257", B, Tp);
  if (!std::isfinite((float)noise_scale)) return dv_fail(DV_ERR_INVALID, "dv_op_regulate_sample: noise_scale %g must be finite", noise_scale);
  hipError_t e = launch_regulate_sample(m_p, logs_p, cum, x_lengths, noise, (float)noise_scale, B, C, Tx, Tp, z_p, m_p_exp, logs_p_exp,
                                        (hipStream_t)stream);
  if (e != hipSuccess) return dv_fail(DV_ERR_HIP, "dv_op_regulate_sample: launch failed: %s", hipGetErrorString(e));
  return DV_OK;
}
