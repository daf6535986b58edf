// Dynamic thresholding (reference sampler/dpm_solver.py:416-425, sampler/uni_pc.py:268-277): the scalar logic that the host
// launcher and the kernels of kernels_thresh.hip share - ranks of the quantile, the walk over a histogram that picks the bin
// of a rank, and the interpolation between the two order statistics.  Plain C++ (host and device); tools/thresh_select_check.cc
// drives it on the host against a sort.
//
//   s = max(quantile(|x0|, ratio), max_val) per row, as torch.quantile(..., interpolation='linear') computes it on float32:
//   r = float(ratio) * float(n - 1) (one float32 product: its q is a float32 tensor), lo = floor(r), hi = ceil(r), w = r - lo,
//   s = lerp(v[lo], v[hi], w) over the ascending order statistics v of |x0|.
//
// Selection is an exact radix select on the bit pattern of |x| (which orders non-negative floats, NaNs last), most significant
// digit first: THR_BITS1 + THR_BITS2 + THR_BITS3 = 32 bits in three passes.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define THR_HD __host__ __device__ inline
#else
#define THR_HD inline
#endif

enum { THR_BITS1 = 11, THR_BITS2 = 11, THR_BITS3 = 10 };
enum { THR_BINS1 = 1 << THR_BITS1, THR_BINS2 = 1 << THR_BITS2, THR_BINS3 = 1 << THR_BITS3 };
// Workspace of one row, in 32-bit words: the histogram of pass 1, two of pass 2 and two of pass 3 (one per rank: lo and hi can
// part ways in any pass), then THR_META words of state.  All of it is zero before pass 1.
enum { THR_H1 = 0, THR_H2A = THR_H1 + THR_BINS1, THR_H2B = THR_H2A + THR_BINS2, THR_H3A = THR_H2B + THR_BINS2,
       THR_H3B = THR_H3A + THR_BINS3, THR_META_AT = THR_H3B + THR_BINS3, THR_META = 16, THR_ROW_WORDS = THR_META_AT + THR_META };
// state words: [0] a NaN was seen; [4..7] after pass 1: prefix / remaining rank of lo, of hi; [8..11] after pass 2 the same
enum { THR_M_NAN = 0, THR_M_ST1 = 4, THR_M_ST2 = 8 };

THR_HD uint32_t thr_key(uint32_t float_bits) { return float_bits & 0x7FFFFFFFu; }      // bit pattern of |x|
THR_HD uint32_t thr_digit1(uint32_t key) { return key >> (THR_BITS2 + THR_BITS3); }
THR_HD uint32_t thr_digit2(uint32_t key) { return (key >> THR_BITS3) & (THR_BINS2 - 1); }
THR_HD uint32_t thr_digit3(uint32_t key) { return key & (THR_BINS3 - 1); }
THR_HD bool thr_key_is_nan(uint32_t key) { return key > 0x7F800000u; }

// Ranks of the quantile of n >= 1 values: r = ratio * (n - 1) in float32.
THR_HD void thr_ranks(float ratio, int64_t n, uint32_t* lo, uint32_t* hi, float* w) {
  const float last = (float)(n - 1);
  float r = ratio * last;
  if (!(r >= 0.0f)) r = 0.0f;
  if (r > last) r = last;                      // (float(n - 1) can round up past n - 1 only above 2^24; the index below is clamped too)
  int64_t l = (int64_t)r;                       // r >= 0: truncation is floor
  if (l > n - 1) l = n - 1;
  int64_t h = ((float)l < r) ? l + 1 : l;       // ceil
  if (h > n - 1) h = n - 1;
  *lo = (uint32_t)l; *hi = (uint32_t)h;
  *w = r - (float)l;
}

// The bin that holds the element of 0-based rank `rank` among the counts h[0 .. nbins), and the rank that remains inside it.
// False (bin = nbins - 1, rem = 0) if the counts hold fewer than rank + 1 elements.
THR_HD bool thr_pick(const uint32_t* h, int nbins, uint32_t rank, uint32_t* bin, uint32_t* rem) {
  for (int i = 0; i < nbins; ++i) {
    const uint32_t c = h[i];
    if (rank < c) { *bin = (uint32_t)i; *rem = rank; return true; }
    rank -= c;
  }
  *bin = (uint32_t)(nbins - 1); *rem = 0;
  return false;
}

// torch's lerp on float32 (ATen/native/Lerp.h): the form is picked by the weight, every operation rounded on its own.
THR_HD float thr_lerp(float a, float b, float w) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float d = b - a;
  if (w < 0.5f) { const float p = w * d; return a + p; }
  const float q = 1.0f - w, p = d * q;
  return b - p;
}

// s of a row from its two order statistics (as bit patterns of |x|): NaN if the row holds one (torch sorts NaN last and points
// every rank of such a row at it), else max(lerp, max_val).
THR_HD float thr_scale(uint32_t key_lo, uint32_t key_hi, float w, float max_val, bool row_has_nan) {
  union { uint32_t u; float f; } a, b, q;
  if (row_has_nan) { q.u = 0x7FC00000u; return q.f; }
  a.u = key_lo; b.u = key_hi;
  const float s = thr_lerp(a.f, b.f, w);
  if (s != s) return s;
  return s > max_val ? s : max_val;
}
