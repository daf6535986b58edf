// Dynamic thresholding of a data prediction inside the sampler loop (reference sampler/dpm_solver.py:416-425,
// sampler/uni_pc.py:268-277):  per row (utterance)  s = max(quantile(|x0|, ratio), max_val),  x0 <- clamp(x0, -s, s) / s,
// in place on x0 [rows, n] fp32.
//
// The quantile is exact: a radix select on the bit pattern of |x| (thresh_select.h) follows the two ranks floor(r) and ceil(r)
// through three passes of 11 + 11 + 10 bits.  Five launches, whatever the shape:
//   k_thr_zero   the histograms and the state of every row
//   k_thr_hist1  counts of the top 11 bits                              (+ "the row holds a NaN")
//   k_thr_hist2  picks the bins of both ranks from pass 1; counts of the middle 11 bits of the elements in them
//   k_thr_hist3  picks from pass 2; counts of the low 10 bits
//   k_thr_apply  picks from pass 3: both order statistics are known to the bit; s; clamp and divide
// A row is shared by `wpr` workgroups.  Every workgroup counts into LDS and merges into the row's global histogram with
// integer atomicAdd (counts do not depend on the order of arrival: the result is deterministic); the ordering between the
// passes is the kernel boundary - no workgroup waits for another.  The walk over the previous pass's histogram is redone by
// every workgroup of the next pass; what it found is written once (by the row's first workgroup) for the pass after that.
#include "dv_common.h"
#include "thresh_select.h"

#include <algorithm>

namespace {

constexpr int THR_THREADS = 256;
constexpr int THR_ELEMS_PER_WG = 2048;      // a row longer than this is split over several workgroups
constexpr int THR_MAX_WGS = 2048;           // of one launch (all rows)

struct ThrSel { uint32_t binA, remA, binB, remB; };

// The bins of rankA in histA[nbins] and of rankB in histB[nbins] (histB may be histA), by all 256 threads of the workgroup:
// per-thread sums of nbins / 256 consecutive bins, then wave 0 (rank A) and wave 1 (rank B) scan the 256 sums - four per lane -
// and the lane whose range holds the rank walks its sums and then that sum's bins (thr_pick).  lds: 2 * 256 + 4 words.
__device__ ThrSel thr_block_pick(const uint32_t* histA, const uint32_t* histB, int nbins, uint32_t rankA, uint32_t rankB,
                                 uint32_t* lds) {
  const int t = threadIdx.x, per = nbins / THR_THREADS;
  uint32_t* csum = lds;                      // [2][256]
  uint32_t* out = lds + 2 * THR_THREADS;     // [4]
  {
    uint32_t a = 0, b = 0;
    for (int i = 0; i < per; ++i) { a += histA[t * per + i]; b += histB[t * per + i]; }
    csum[t] = a; csum[THR_THREADS + t] = b;
    if (t < 4) out[t] = 0;
  }
  __syncthreads();
  const int wave = t >> 6, lane = t & 63;
  if (wave < 2) {
    const uint32_t* cs = csum + wave * THR_THREADS + lane * 4;
    const uint32_t* hist = wave == 0 ? histA : histB;
    const uint32_t rank = wave == 0 ? rankA : rankB;
    uint32_t c[4] = {cs[0], cs[1], cs[2], cs[3]};
    const uint32_t tot = c[0] + c[1] + c[2] + c[3];
    uint32_t incl = tot;
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    const uint32_t excl = incl - tot;
    if (rank >= excl && rank < incl) {       // exactly one lane (rank < the row's count)
      uint32_t ci, r2, bi, r3;
      thr_pick(c, 4, rank - excl, &ci, &r2);
      const uint32_t chunk = (uint32_t)lane * 4 + ci;
      thr_pick(hist + chunk * per, per, r2, &bi, &r3);
      out[wave * 2] = chunk * per + bi;
      out[wave * 2 + 1] = r3;
    }
  }
  __syncthreads();
  ThrSel s;
  s.binA = out[0]; s.remA = out[1]; s.binB = out[2]; s.remB = out[3];
  __syncthreads();                           // (lds is reused by the caller)
  return s;
}

__global__ __launch_bounds__(THR_THREADS) void k_thr_zero(uint32_t* ws, size_t words) {
  for (size_t i = (size_t)blockIdx.x * THR_THREADS + threadIdx.x; i < words; i += (size_t)gridDim.x * THR_THREADS) ws[i] = 0u;
}

// LDS counts -> the row's global histogram (empty bins are skipped: most are)
__device__ void thr_merge(const uint32_t* lds_hist, uint32_t* g_hist, int nbins) {
  for (int i = threadIdx.x; i < nbins; i += THR_THREADS) {
    const uint32_t c = lds_hist[i];
    if (c) atomicAdd(g_hist + i, c);
  }
}

__global__ __launch_bounds__(THR_THREADS) void k_thr_hist1(const float* __restrict__ x, uint32_t* ws, int rows, int64_t n, int wpr) {
  __shared__ uint32_t h[THR_BINS1];
  __shared__ uint32_t nan_seen;
  const int row = blockIdx.x / wpr, j = blockIdx.x % wpr, t = threadIdx.x;
  if (row >= rows) return;
  for (int i = t; i < THR_BINS1; i += THR_THREADS) h[i] = 0u;
  if (t == 0) nan_seen = 0u;
  __syncthreads();
  const uint32_t* xr = reinterpret_cast<const uint32_t*>(x) + (size_t)row * n;
  bool nan = false;
  for (int64_t i = (int64_t)j * THR_THREADS + t; i < n; i += (int64_t)wpr * THR_THREADS) {
    const uint32_t key = thr_key(xr[i]);
    nan |= thr_key_is_nan(key);
    atomicAdd(&h[thr_digit1(key)], 1u);
  }
  if (nan) nan_seen = 1u;
  __syncthreads();
  uint32_t* wr = ws + (size_t)row * THR_ROW_WORDS;
  thr_merge(h, wr + THR_H1, THR_BINS1);
  if (t == 0 && nan_seen) atomicOr(wr + THR_META_AT + THR_M_NAN, 1u);
}

__global__ __launch_bounds__(THR_THREADS) void k_thr_hist2(const float* __restrict__ x, uint32_t* ws, int rows, int64_t n, int wpr,
                                                            uint32_t rank_lo, uint32_t rank_hi) {
  __shared__ uint32_t hA[THR_BINS2], hB[THR_BINS2];
  __shared__ uint32_t pick[2 * THR_THREADS + 4];
  const int row = blockIdx.x / wpr, j = blockIdx.x % wpr, t = threadIdx.x;
  if (row >= rows) return;
  uint32_t* wr = ws + (size_t)row * THR_ROW_WORDS;
  const ThrSel s = thr_block_pick(wr + THR_H1, wr + THR_H1, THR_BINS1, rank_lo, rank_hi, pick);
  if (j == 0 && t == 0) {
    uint32_t* st = wr + THR_META_AT + THR_M_ST1;
    st[0] = s.binA; st[1] = s.remA; st[2] = s.binB; st[3] = s.remB;
  }
  for (int i = t; i < THR_BINS2; i += THR_THREADS) { hA[i] = 0u; hB[i] = 0u; }
  __syncthreads();
  const uint32_t* xr = reinterpret_cast<const uint32_t*>(x) + (size_t)row * n;
  const bool same = s.binA == s.binB;
  for (int64_t i = (int64_t)j * THR_THREADS + t; i < n; i += (int64_t)wpr * THR_THREADS) {
    const uint32_t key = thr_key(xr[i]), d1 = thr_digit1(key);
    if (d1 == s.binA) atomicAdd(&hA[thr_digit2(key)], 1u);
    else if (d1 == s.binB) atomicAdd(&hB[thr_digit2(key)], 1u);
  }
  __syncthreads();
  thr_merge(hA, wr + THR_H2A, THR_BINS2);
  if (!same) thr_merge(hB, wr + THR_H2B, THR_BINS2);
}

__global__ __launch_bounds__(THR_THREADS) void k_thr_hist3(const float* __restrict__ x, uint32_t* ws, int rows, int64_t n, int wpr) {
  __shared__ uint32_t hA[THR_BINS3], hB[THR_BINS3];
  __shared__ uint32_t pick[2 * THR_THREADS + 4];
  const int row = blockIdx.x / wpr, j = blockIdx.x % wpr, t = threadIdx.x;
  if (row >= rows) return;
  uint32_t* wr = ws + (size_t)row * THR_ROW_WORDS;
  const uint32_t* st1 = wr + THR_META_AT + THR_M_ST1;
  const uint32_t p1A = st1[0], r1A = st1[1], p1B = st1[2], r1B = st1[3];
  // (both ranks in one bin of pass 1: pass 2 counted that bin into the A histogram only)
  const ThrSel s = thr_block_pick(wr + THR_H2A, wr + (p1A == p1B ? THR_H2A : THR_H2B), THR_BINS2, r1A, r1B, pick);
  const uint32_t preA = (p1A << THR_BITS2) | s.binA, preB = (p1B << THR_BITS2) | s.binB;      // the top 22 bits
  if (j == 0 && t == 0) {
    uint32_t* st = wr + THR_META_AT + THR_M_ST2;
    st[0] = preA; st[1] = s.remA; st[2] = preB; st[3] = s.remB;
  }
  for (int i = t; i < THR_BINS3; i += THR_THREADS) { hA[i] = 0u; hB[i] = 0u; }
  __syncthreads();
  const uint32_t* xr = reinterpret_cast<const uint32_t*>(x) + (size_t)row * n;
  const bool same = preA == preB;
  for (int64_t i = (int64_t)j * THR_THREADS + t; i < n; i += (int64_t)wpr * THR_THREADS) {
    const uint32_t key = thr_key(xr[i]), pre = key >> THR_BITS3;
    if (pre == preA) atomicAdd(&hA[thr_digit3(key)], 1u);
    else if (pre == preB) atomicAdd(&hB[thr_digit3(key)], 1u);
  }
  __syncthreads();
  thr_merge(hA, wr + THR_H3A, THR_BINS3);
  if (!same) thr_merge(hB, wr + THR_H3B, THR_BINS3);
}

// clamp(v, -s, s) / s as torch rounds it; a NaN element stays NaN, a NaN s makes every element NaN
__device__ __forceinline__ float thr_apply1(float v, float s) {
  const float c = (v != v) ? v : fminf(fmaxf(v, -s), s);
  return __fdiv_rn(c, s);
}

__global__ __launch_bounds__(THR_THREADS) void k_thr_apply(float* x, const uint32_t* ws, int rows, int64_t n, int wpr, float w,
                                                            float max_val, float* s_out) {
  __shared__ uint32_t pick[2 * THR_THREADS + 4];
  const int row = blockIdx.x / wpr, j = blockIdx.x % wpr, t = threadIdx.x;
  if (row >= rows) return;
  const uint32_t* wr = ws + (size_t)row * THR_ROW_WORDS;
  const uint32_t* st2 = wr + THR_META_AT + THR_M_ST2;
  const uint32_t preA = st2[0], r2A = st2[1], preB = st2[2], r2B = st2[3];
  const ThrSel sel = thr_block_pick(wr + THR_H3A, wr + (preA == preB ? THR_H3A : THR_H3B), THR_BINS3, r2A, r2B, pick);
  const float s = thr_scale((preA << THR_BITS3) | sel.binA, (preB << THR_BITS3) | sel.binB, w, max_val,
                            wr[THR_META_AT + THR_M_NAN] != 0u);
  if (j == 0 && t == 0 && s_out) s_out[row] = s;
  // float4 over the 16-byte aligned middle of the row; the (up to 3 + 3) elements before and behind it one by one
  float* xr = x + (size_t)row * n;
  int64_t head = (int64_t)(((16u - (unsigned)((uintptr_t)xr & 15u)) & 15u) >> 2);
  if (head > n) head = n;
  const int64_t n4 = (n - head) / 4, tail = n - head - n4 * 4;
  float4* x4 = reinterpret_cast<float4*>(xr + head);
  for (int64_t i = (int64_t)j * THR_THREADS + t; i < n4; i += (int64_t)wpr * THR_THREADS) {
    float4 v = x4[i];
    v.x = thr_apply1(v.x, s); v.y = thr_apply1(v.y, s); v.z = thr_apply1(v.z, s); v.w = thr_apply1(v.w, s);
    x4[i] = v;
  }
  if (j == 0) {
    if (t < head) xr[t] = thr_apply1(xr[t], s);
    if (t < tail) { float* e = xr + head + n4 * 4 + t; *e = thr_apply1(*e, s); }
  }
}

int thr_wgs_per_row(int rows, int64_t n) {
  int64_t wpr = (n + THR_ELEMS_PER_WG - 1) / THR_ELEMS_PER_WG;
  const int64_t cap = std::max<int64_t>(1, THR_MAX_WGS / rows);
  return (int)std::max<int64_t>(1, std::min(wpr, cap));
}

}  // namespace

size_t dyn_thresh_ws_bytes(int rows) { return (size_t)rows * THR_ROW_WORDS * sizeof(uint32_t); }

hipError_t launch_dyn_thresh(float* x, int rows, int64_t n, float ratio, float max_val, uint32_t* ws, float* s_out, hipStream_t st) {
  if (!x || !ws || rows < 1 || rows > THR_MAX_WGS || n < 1 || n > (int64_t)INT32_MAX || ((uintptr_t)x & 3u)) return hipErrorInvalidValue;
  uint32_t lo, hi; float w;
  thr_ranks(ratio, n, &lo, &hi, &w);
  const int wpr = thr_wgs_per_row(rows, n), grid = rows * wpr;
  const size_t words = (size_t)rows * THR_ROW_WORDS;
  const int zgrid = (int)std::min<size_t>((words + THR_THREADS - 1) / THR_THREADS, 1024);
  hipLaunchKernelGGL(k_thr_zero, dim3(zgrid), dim3(THR_THREADS), 0, st, ws, words);
  hipLaunchKernelGGL(k_thr_hist1, dim3(grid), dim3(THR_THREADS), 0, st, x, ws, rows, n, wpr);
  hipLaunchKernelGGL(k_thr_hist2, dim3(grid), dim3(THR_THREADS), 0, st, x, ws, rows, n, wpr, lo, hi);
  hipLaunchKernelGGL(k_thr_hist3, dim3(grid), dim3(THR_THREADS), 0, st, x, ws, rows, n, wpr);
  hipLaunchKernelGGL(k_thr_apply, dim3(grid), dim3(THR_THREADS), 0, st, x, ws, rows, n, wpr, w, max_val, s_out);
  return hipGetLastError();
}
