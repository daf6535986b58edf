// Host check of diff-vits_amd/csrc/thresh_select.h - the rank, histogram-walk and interpolation logic that the dynamic
// thresholding kernels (csrc/kernels_thresh.hip) share with the host - against a full sort.  The three passes are replayed
// here as the kernels run them (one histogram in pass 1, one per rank in passes 2 and 3, shared when both ranks sit in the
// same bin; the remaining rank carried from pass to pass), so a wrong shift, bin count or carried rank shows up without a GPU.
//
//   mkdir -p build && c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/thresh_select_check.cc \
//       -o build/thresh_select_check && build/thresh_select_check
// prints one line per family of rows and exits non-zero if any check failed.
#include "../diff-vits_amd/csrc/thresh_select.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float float_of(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

// the kernels' three passes on one row; returns false if a walk ran off its histogram
static bool select_two(const std::vector<float>& x, uint32_t lo, uint32_t hi, uint32_t* key_lo, uint32_t* key_hi, bool* has_nan) {
  std::vector<uint32_t> ws(THR_ROW_WORDS, 0u);
  *has_nan = false;
  for (float v : x) { const uint32_t k = thr_key(bits_of(v)); *has_nan |= thr_key_is_nan(k); ws[THR_H1 + thr_digit1(k)]++; }
  uint32_t p1A, r1A, p1B, r1B;
  if (!thr_pick(&ws[THR_H1], THR_BINS1, lo, &p1A, &r1A) || !thr_pick(&ws[THR_H1], THR_BINS1, hi, &p1B, &r1B)) return false;
  for (float v : x) {
    const uint32_t k = thr_key(bits_of(v)), d1 = thr_digit1(k);
    if (d1 == p1A) ws[THR_H2A + thr_digit2(k)]++;
    else if (d1 == p1B) ws[THR_H2B + thr_digit2(k)]++;
  }
  uint32_t b2A, r2A, b2B, r2B;
  if (!thr_pick(&ws[THR_H2A], THR_BINS2, r1A, &b2A, &r2A)) return false;
  if (!thr_pick(&ws[p1A == p1B ? THR_H2A : THR_H2B], THR_BINS2, r1B, &b2B, &r2B)) return false;
  const uint32_t preA = (p1A << THR_BITS2) | b2A, preB = (p1B << THR_BITS2) | b2B;
  for (float v : x) {
    const uint32_t k = thr_key(bits_of(v)), pre = k >> THR_BITS3;
    if (pre == preA) ws[THR_H3A + thr_digit3(k)]++;
    else if (pre == preB) ws[THR_H3B + thr_digit3(k)]++;
  }
  uint32_t b3A, r3A, b3B, r3B;
  if (!thr_pick(&ws[THR_H3A], THR_BINS3, r2A, &b3A, &r3A)) return false;
  if (!thr_pick(&ws[preA == preB ? THR_H3A : THR_H3B], THR_BINS3, r2B, &b3B, &r3B)) return false;
  *key_lo = (preA << THR_BITS3) | b3A;
  *key_hi = (preB << THR_BITS3) | b3B;
  return true;
}

static int failures = 0;

static void check_row(const std::string& name, const std::vector<float>& x, float ratio, float max_val) {
  const int64_t n = (int64_t)x.size();
  uint32_t lo, hi; float w;
  thr_ranks(ratio, n, &lo, &hi, &w);
  // independent statement of the ranks: double arithmetic on the float32 product
  const float r = ratio * (float)(n - 1);
  const uint32_t lo_ref = (uint32_t)std::floor((double)r), hi_ref = (uint32_t)std::ceil((double)r);
  bool ok = lo == lo_ref && hi == hi_ref && hi < (uint32_t)n && w == (float)((double)r - (double)lo_ref) && w >= 0.0f && w < 1.0f;
  std::vector<uint32_t> keys;
  for (float v : x) keys.push_back(bits_of(v) & 0x7FFFFFFFu);
  std::sort(keys.begin(), keys.end());
  uint32_t kl = 0, kh = 0; bool nan = false;
  ok = ok && select_two(x, lo, hi, &kl, &kh, &nan);
  ok = ok && kl == keys[lo] && kh == keys[hi];
  const bool nan_ref = keys.back() > 0x7F800000u;
  ok = ok && nan == nan_ref;
  const float s = thr_scale(kl, kh, w, max_val, nan);
  if (nan_ref) ok = ok && std::isnan(s);
  else {
    const double a = float_of(keys[lo]), b = float_of(keys[hi]);
    const double exact = std::max(a + (double)w * (b - a), (double)max_val);
    const float want = (float)exact;
    // one float32 ulp around the exactly rounded value (two roundings in thr_lerp); exact where the weight is 0
    const float up = std::nextafter(want, std::numeric_limits<float>::infinity()), dn = std::nextafter(want, 0.0f);
    // an infinite upper order statistic: torch's lerp gives a + w * inf = inf below w = 0.5 and inf - inf * (1 - w) = NaN from
    // there on, and NaN (0 * (inf - inf)) between two infinities
    if (std::isinf(b) && w != 0.0f) ok = ok && (std::isinf(a) || w >= 0.5f ? std::isnan(s) : std::isinf(s));
    else if (std::isnan(want)) ok = ok && std::isnan(s);
    else ok = ok && (w == 0.0f ? s == want : (s >= dn && s <= up));
  }
  if (!ok) {
    ++failures;
    printf("FAIL %s: n %lld ratio %.9g ranks %u %u (ref %u %u) w %.9g keys %08x %08x (ref %08x %08x) s %.9g\n", name.c_str(), (long long)n,
           (double)ratio, lo, hi, lo_ref, hi_ref, (double)w, kl, kh, keys[lo], keys[hi], (double)s);
  }
}

static void check_family(const std::string& name, const std::vector<float>& x, float max_val = 1e-30f) {
  const int64_t n = (int64_t)x.size();
  const int before = failures;
  std::vector<float> ratios = {0.0f, 1.0f, 0.5f, 0.9f, 0.995f, 0.25f, 0.999999f};
  if (n > 1) for (int64_t k : {(int64_t)1, n / 2, n - 2, n - 1}) ratios.push_back((float)((double)k / (double)(n - 1)));
  for (float q : ratios) check_row(name, x, q, max_val);
  check_row(name + " (floored)", x, 0.5f, 3.0e38f);
  printf("%-44s n %-8lld %s\n", name.c_str(), (long long)n, failures == before ? "ok" : "FAILED");
}

int main() {
  std::mt19937 gen(20240611u);
  std::normal_distribution<float> normal(0.0f, 1.0f);
  const float den = std::numeric_limits<float>::denorm_min();
  check_family("one element", {-0.75f});
  check_family("two elements", {2.0f, -1.0f});
  check_family("three elements", {0.5f, -3.0f, 0.25f});
  check_family("all equal", std::vector<float>(257, -1.25f));
  {
    std::vector<float> x(1001);
    for (size_t i = 0; i < x.size(); ++i) x[i] = i < 300 ? 0.01f * (float)(i + 1) : (i < 900 ? -3.5f : 4.0f + (float)i);      // 600 duplicates
    std::shuffle(x.begin(), x.end(), gen);
    check_family("more than n / 2 duplicates", x);
  }
  check_family("zeros, denormals, one large", {0.0f, -0.0f, den, -den, 3 * den, -0.0f, 1.0e30f, 0.0f, 2 * den, -1.1754942e-38f});
  {
    std::vector<float> x(4097);
    for (float& v : x) v = normal(gen);
    check_family("normal 4097", x);
    check_family("normal 4097, floor applies", x, 100.0f);
    x[1234] = std::numeric_limits<float>::quiet_NaN();
    check_family("with a NaN", x);
    x[1234] = std::numeric_limits<float>::infinity();
    check_family("with an infinity", x);
  }
  {
    // neighbouring ranks in different bins of pass 1, of pass 2 and of pass 3
    std::vector<float> x;
    for (int i = 0; i < 50; ++i) x.push_back(1.0f + (float)i);                           // spread over exponents
    for (int i = 0; i < 50; ++i) x.push_back(-float_of(0x3F800000u + ((uint32_t)i << 10)));      // one pass-1 bin, 50 pass-2 bins
    for (int i = 0; i < 50; ++i) x.push_back(float_of(0x40490000u + (uint32_t)i));          // one pass-2 bin, 50 pass-3 bins
    std::shuffle(x.begin(), x.end(), gen);
    const int before = failures;
    for (int k = 0; k + 1 < (int)x.size(); ++k) check_row("bin boundaries", x, ((float)k + 0.5f) / (float)(x.size() - 1), 1e-30f);
    printf("%-44s n %-8lld %s\n", "bin boundaries, every pair of ranks", (long long)x.size(), failures == before ? "ok" : "FAILED");
  }
  {
    std::vector<float> x(204800);
    for (float& v : x) v = normal(gen);
    check_family("normal 204800", x);
  }
  {
    // thr_pick on counts that do not reach the rank
    uint32_t h[4] = {1, 0, 2, 0}, bin = 77, rem = 77;
    const bool short_ok = !thr_pick(h, 4, 3, &bin, &rem) && bin == 3 && rem == 0 && thr_pick(h, 4, 2, &bin, &rem) && bin == 2 && rem == 1;
    if (!short_ok) ++failures;
    printf("%-44s %s\n", "thr_pick past the counts", short_ok ? "ok" : "FAILED");
  }
  printf(failures ? "%d FAILURES\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}
