// Sample-rate conversion (audio.py Resample: torchaudio.transforms.Resample's documented defaults - sinc_interp_hann, lowpass_filter_width 6,
// rolloff 0.99) for a RAGGED batch of recordings in ONE launch: wave [B, n_max] + n_samples [B] + pair [B] -> out [B, n_out_max] +
// n_out [B].  Every row has its own length and its own reduced rate pair (o, n) = (orig, new) / gcd:
//     y[q n + p] = sum_j h[p][j] x[q o - width + j],   x = 0 outside [0, n_b),   n_out_b = ceil(n n_b / o),
// every element at or past n_out_b exactly zero.
//
//   k_resample  grid (ceil(n_out_max / 512), B), 256 threads: a workgroup owns RS_TILE = 512 neighbouring output samples of one row.
//               Table.  The clamp of the definition makes most of the K = 2 width + o taps of a phase exact zeros; the handle keeps,
//               per phase, the first non-zero tap, the count up to the last one and the taps between them (the idiom of the mel
//               kernel's band ranges: any table is handled), TAP-MAJOR: tab[jj * n + p].  The row's table (R n floats, R = the
//               longest range, about 2 width + 2: at most ~12.2 max(o, n) + 2 n floats) is copied to LDS once per workgroup.
//               Operand.  Output i = q n + p reads samples from floor(i o / n) - width + dmin to floor(i o / n) - width + dmax
//               (dmin / dmax: the extremes of first[p] - floor(p o / n) and last[p] - floor(p o / n) over the phases), so the 512
//               outputs of a tile need 512 o / n + 2 width samples.  They are staged in LDS once, from a start rounded down to four
//               samples: 16-byte loads where the row's base is 16-byte aligned and the four samples lie inside [0, n_b), single
//               guarded loads at the two ends; zeros are substituted outside [0, n_b) and no sample at an index >= n_b is read.
//               Where table + span would not fit the 160 KB of a CU (o / n large) the tile is worked off in chunks of `chunk`
//               outputs, each staged alone; the chunk is the handle's, fixed at create (512 for every audio rate pair).
//               Thread mapping.  Lane = output sample, so neighbouring lanes are neighbouring PHASES of (mostly) one block q:
//                 - tap reads tab[jj * n + p] are consecutive words across the lanes (ds_read_b32: 32 banks per 32-lane half,
//                   conflict-free; where p wraps from n - 1 to 0 inside a half the two runs can share banks, 2-way at worst).  A
//                   PHASE-major table would put the lanes R words apart and R is even for half of the pairs;
//                 - sample reads are at floor(i o / n) + jj + const: when upsampling (o < n) several lanes share a word (broadcast),
//                   when downsampling the lanes step by o / n words: up to ceil(o / n)-way conflicts (2-way for 44.1 -> 24 kHz and
//                   48 -> 24 kHz).  One FMA hangs on the two reads, the kernel moves ~8 bytes per output from HBM and stays
//                   bound by the launch at the product's sizes (profiles/resample_bench.txt), so the operand is left unswizzled.
//               The sum runs over the phase's range in ascending j, starting from the first product (not from +0: a delta table,
//               the pair o = n, copies every bit, -0 included) and continuing with fmaf.  64-bit sample indices: n_max <= 2^30
//               and n <= 1024.  A row whose n_samples is outside [0, n_max] or whose pair is out of range is all zeros with
//               n_out[b] = 0 - a value to check, not a fault.  No atomics, no scratch, nothing allocates or waits: capturable.
// The taps are computed in fp64 on the host in torchaudio's order of operations and rounded once to fp32.
#include "../../include/dvits_hip.h"
#include "dv_common.h"

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

int dv_fail(int code, const char* fmt, ...);

namespace {

constexpr int RS_TILE = 512, RS_THREADS = 256;
constexpr int RS_MAX_RATE = 1024;                 // o, n after reduction
constexpr int RS_MAX_PAIRS = 64;
constexpr int RS_LDS_BYTES = 160 * 1024;
constexpr double RS_LOWPASS_WIDTH = 6.0, RS_ROLLOFF = 0.99;

struct RsPair {
  int o, n, width, R;        // reduced rates, left padding of the definition, longest tap range of a phase
  int dmin, dmax;            // extremes of first[p] - floor(p o / n) / last[p] - floor(p o / n) over the phases
  int chunk, span;           // outputs staged at a time (<= RS_TILE), capacity of the staged span in floats (multiple of 4)
  int tab_off, rng_off;      // this pair's taps (floats) / ranges (int2) inside the handle's tables
  int lds_tab, lds_x;        // byte offsets of the staged table / span behind the ranges in LDS
};

__global__ __launch_bounds__(RS_THREADS) void k_resample(const float* __restrict__ wave, const int64_t* __restrict__ n_samples,
                                                        const int32_t* __restrict__ pair, int n_pairs, int64_t n_max,
                                                        float* __restrict__ out, int64_t n_out_max, int64_t* __restrict__ n_out,
                                                        const RsPair* __restrict__ pairs, const float* __restrict__ tabs,
                                                        const int2* __restrict__ rngs) {
  extern __shared__ __attribute__((aligned(16))) char rs_smem[];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * RS_TILE;
  const int64_t nb64 = n_samples[b];
  const int pi = pair ? pair[b] : 0;
  const bool row_ok = nb64 >= 0 && nb64 <= n_max && pi >= 0 && pi < n_pairs;
  const RsPair pd = pairs[row_ok ? pi : 0];
  const int64_t nb = row_ok ? nb64 : 0;
  const int64_t nob = (nb * pd.n + pd.o - 1) / pd.o;
  if (blockIdx.x == 0 && tid == 0) n_out[b] = nob;
  float* const orow = out + (size_t)b * n_out_max;
  const int tile_n = (int)(n_out_max - i0 < RS_TILE ? n_out_max - i0 : RS_TILE);       // elements of the buffer in this tile
  const int live = nob <= i0 ? 0 : (int)(nob - i0 < tile_n ? nob - i0 : tile_n);       // ... of them the row's own outputs

  if (live > 0) {                                  // workgroup-uniform
    int2* const s_rng = reinterpret_cast<int2*>(rs_smem);
    float* const s_tab = reinterpret_cast<float*>(rs_smem + pd.lds_tab);
    float* const s_x = reinterpret_cast<float*>(rs_smem + pd.lds_x);
    for (int t = tid; t < pd.n; t += RS_THREADS) s_rng[t] = rngs[pd.rng_off + t];
    for (int t = tid; t < pd.R * pd.n; t += RS_THREADS) s_tab[t] = tabs[pd.tab_off + t];

    const int64_t q0 = i0 / pd.n;
    const int r0 = (int)(i0 - q0 * pd.n);          // output i0 + e is phase (r0 + e) % n of block q0 + (r0 + e) / n
    const float* const wrow = wave + (size_t)b * n_max;
    const bool vec = (reinterpret_cast<uintptr_t>(wrow) & 15) == 0;
    for (int c0 = 0; c0 < live; c0 += pd.chunk) {
      const int c1 = c0 + pd.chunk < live ? c0 + pd.chunk : live;
      // floor(i o / n) of the chunk's first and last output; every sample they and the outputs between them read lies in [S0, S0 + len)
      const int64_t g0 = q0 * pd.o + ((int64_t)(r0 + c0) * pd.o) / pd.n;
      const int64_t g1 = q0 * pd.o + ((int64_t)(r0 + c1 - 1) * pd.o) / pd.n;
      const int64_t S0 = (g0 - pd.width + pd.dmin) & ~(int64_t)3;
      const int len = (int)(g1 - pd.width + pd.dmax - S0) + 1;         // <= pd.span - 3 (create)
      __syncthreads();                             // the previous chunk has been read
      for (int t = tid * 4; t < len; t += RS_THREADS * 4) {
        const int64_t s = S0 + t;
        float4 v;
        if (vec && s >= 0 && s + 3 < nb) {
          v = *reinterpret_cast<const float4*>(wrow + s);
        } else {
          v.x = (s >= 0 && s < nb) ? wrow[s] : 0.f;
          v.y = (s + 1 >= 0 && s + 1 < nb) ? wrow[s + 1] : 0.f;
          v.z = (s + 2 >= 0 && s + 2 < nb) ? wrow[s + 2] : 0.f;
          v.w = (s + 3 >= 0 && s + 3 < nb) ? wrow[s + 3] : 0.f;
        }
        *reinterpret_cast<float4*>(s_x + t) = v;
      }
      __syncthreads();
      const int64_t base = q0 * pd.o - pd.width - S0;
      for (int e = c0 + tid; e < c1; e += RS_THREADS) {
        const int pp = r0 + e, dq = pp / pd.n, p = pp - dq * pd.n;
        const int2 rg = s_rng[p];                  // (first tap, taps)
        float acc = 0.f;
        if (rg.y > 0) {
          const float* const xp = s_x + (int)(base + (int64_t)dq * pd.o + rg.x);
          const float* const hp = s_tab + p;
          acc = hp[0] * xp[0];
          for (int j = 1; j < rg.y; ++j) acc = fmaf(hp[j * pd.n], xp[j], acc);
        }
        orow[i0 + e] = acc;
      }
    }
  }
  for (int e = live + tid; e < tile_n; e += RS_THREADS) orow[i0 + e] = 0.f;
}

struct RsHandle {
  int n_pairs = 0;
  int lds_bytes = 0;
  std::vector<RsPair> pairs;       // host copy: n_out_max of a call
  void* slab = nullptr;
  const RsPair* d_pairs = nullptr;
  const float* d_tabs = nullptr;
  const int2* d_rngs = nullptr;
};

int64_t gcd64(int64_t a, int64_t b) {
  while (b) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// h[p][j] of the definition, fp64 in torchaudio's order of operations, rounded once; o == n: the delta at j = width (the identity)
void rs_taps(int o, int n, int width, std::vector<float>& h) {
  const int K = 2 * width + o;
  const double base = (double)(o < n ? o : n) * RS_ROLLOFF, scale = base / (double)o, pi = 3.14159265358979323846;
  h.assign((size_t)n * K, 0.f);
  for (int p = 0; p < n; ++p)
    for (int j = 0; j < K; ++j) {
      if (o == n) {
        h[(size_t)p * K + j] = j == width ? 1.f : 0.f;
        continue;
      }
      double t = ((double)(-p) / (double)n + (double)(j - width) / (double)o) * base;
      t = t < -RS_LOWPASS_WIDTH ? -RS_LOWPASS_WIDTH : (t > RS_LOWPASS_WIDTH ? RS_LOWPASS_WIDTH : t);
      const double c = std::cos(t * pi / RS_LOWPASS_WIDTH / 2.0), window = c * c;
      t *= pi;
      const double k = t == 0.0 ? 1.0 : std::sin(t) / t;
      h[(size_t)p * K + j] = (float)(k * (window * scale));
    }
}

int rs_span(const RsPair& d, int chunk) { return (int)((((int64_t)(chunk - 1) * d.o) / d.n + d.dmax - d.dmin + 6 + 3) / 4 * 4); }

}  // namespace

struct dv_resample { RsHandle h; };

extern "C" int dv_resample_create(const int32_t* orig, const int32_t* new_, int32_t n_pairs, dv_resample** out) {
  if (!orig || !new_ || !out) return dv_fail(DV_ERR_INVALID, "dv_resample_create: null argument");
  *out = nullptr;
  if (n_pairs < 1 || n_pairs > RS_MAX_PAIRS) return dv_fail(DV_ERR_INVALID, "dv_resample_create: n_pairs = %d must be in 1..%d", n_pairs, RS_MAX_PAIRS);
  std::vector<RsPair> pairs(n_pairs);
  std::vector<float> tabs;
  std::vector<int2> rngs;
  int lds_bytes = 0;
  for (int i = 0; i < n_pairs; ++i) {
    if (orig[i] < 1 || new_[i] < 1) return dv_fail(DV_ERR_INVALID, "dv_resample_create: pair %d: rates %d -> %d must be >= 1", i, orig[i], new_[i]);
    const int64_t g = gcd64(orig[i], new_[i]);
    const int64_t o64 = orig[i] / g, n64 = new_[i] / g;
    if (o64 > RS_MAX_RATE || n64 > RS_MAX_RATE)
      return dv_fail(DV_ERR_INVALID, "dv_resample_create: pair %d: %d -> %d reduces to %lld : %lld, both must be <= %d (the table is staged in LDS)", i,
                     orig[i], new_[i], (long long)o64, (long long)n64, RS_MAX_RATE);
    RsPair& d = pairs[i];
    d.o = (int)o64;
    d.n = (int)n64;
    const double base = (double)(d.o < d.n ? d.o : d.n) * RS_ROLLOFF;
    d.width = (int)std::ceil(RS_LOWPASS_WIDTH * d.o / base);
    const int K = 2 * d.width + d.o;
    std::vector<float> h;
    rs_taps(d.o, d.n, d.width, h);
    // per phase: first non-zero tap and the count up to the last one
    std::vector<int2> rg(d.n);
    d.R = 1;
    bool any = false;
    d.dmin = d.dmax = 0;
    for (int p = 0; p < d.n; ++p) {
      int lo = 0, hi = -1;
      for (int j = 0; j < K; ++j)
        if (h[(size_t)p * K + j] != 0.f) {
          if (hi < 0) lo = j;
          hi = j;
        }
      rg[p] = make_int2(lo, hi - lo + 1);
      if (hi < 0) continue;
      if (hi - lo + 1 > d.R) d.R = hi - lo + 1;
      const int c = (int)(((int64_t)p * d.o) / d.n);
      if (!any || lo - c < d.dmin) d.dmin = lo - c;
      if (!any || hi - c > d.dmax) d.dmax = hi - c;
      any = true;
    }
    d.tab_off = (int)tabs.size();
    d.rng_off = (int)rngs.size();
    tabs.resize(tabs.size() + (size_t)d.R * d.n, 0.f);
    for (int p = 0; p < d.n; ++p) {
      rngs.push_back(rg[p]);
      for (int jj = 0; jj < rg[p].y; ++jj) tabs[d.tab_off + (size_t)jj * d.n + p] = h[(size_t)p * K + rg[p].x + jj];
    }
    // LDS: ranges | table | span; the largest chunk of the tile whose span still fits
    d.lds_tab = (d.n * (int)sizeof(int2) + 15) / 16 * 16;
    d.lds_x = d.lds_tab + (d.R * d.n * (int)sizeof(float) + 15) / 16 * 16;
    d.chunk = RS_TILE;
    while (d.chunk >= 1 && (int64_t)d.lds_x + (int64_t)rs_span(d, d.chunk) * 4 > RS_LDS_BYTES) d.chunk = d.chunk > 8 ? d.chunk - 8 : d.chunk - 1;
    if (d.chunk < 1)
      return dv_fail(DV_ERR_INVALID, "dv_resample_create: pair %d: %d -> %d: the table of %d x %d taps and one output's span do not fit %d bytes of LDS", i,
                     orig[i], new_[i], d.R, d.n, RS_LDS_BYTES);
    d.span = rs_span(d, d.chunk);
    const int need = d.lds_x + d.span * 4;
    if (need > lds_bytes) lds_bytes = need;
  }
  // one slab: pair descriptors | taps | ranges
  const size_t o_pairs = 0, o_tabs = (o_pairs + pairs.size() * sizeof(RsPair) + 15) / 16 * 16;
  const size_t o_rngs = (o_tabs + tabs.size() * sizeof(float) + 15) / 16 * 16, bytes = o_rngs + rngs.size() * sizeof(int2);
  std::vector<char> host(bytes, 0);
  std::memcpy(host.data() + o_pairs, pairs.data(), pairs.size() * sizeof(RsPair));
  std::memcpy(host.data() + o_tabs, tabs.data(), tabs.size() * sizeof(float));
  std::memcpy(host.data() + o_rngs, rngs.data(), rngs.size() * sizeof(int2));
  dv_resample* h = new (std::nothrow) dv_resample();
  if (!h) return dv_fail(DV_ERR_INVALID, "dv_resample_create: out of host memory");
  hipError_t e = hipMalloc(&h->h.slab, bytes);
  if (e == hipSuccess) e = hipMemcpy(h->h.slab, host.data(), bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess && lds_bytes > 64 * 1024)
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_resample), hipFuncAttributeMaxDynamicSharedMemorySize, RS_LDS_BYTES);
  if (e != hipSuccess) {
    if (h->h.slab) (void)hipFree(h->h.slab);
    delete h;
    return dv_fail(DV_ERR_HIP, "dv_resample_create: device tables: %s", hipGetErrorString(e));
  }
  char* d = static_cast<char*>(h->h.slab);
  h->h.n_pairs = n_pairs;
  h->h.lds_bytes = lds_bytes;
  h->h.pairs = pairs;
  h->h.d_pairs = reinterpret_cast<const RsPair*>(d + o_pairs);
  h->h.d_tabs = reinterpret_cast<const float*>(d + o_tabs);
  h->h.d_rngs = reinterpret_cast<const int2*>(d + o_rngs);
  *out = h;
  return DV_OK;
}

extern "C" int dv_resample_forward(dv_resample* h, const float* wave, const int64_t* n_samples, const int32_t* pair, int32_t B, int64_t n_max,
                                   float* out, int64_t n_out_max, int64_t* n_out, void* stream) {
  if (!h || !wave || !n_samples || !out || !n_out) return dv_fail(DV_ERR_INVALID, "dv_resample_forward: null argument");
  if (B < 1 || B > 65535) return dv_fail(DV_ERR_INVALID, "dv_resample_forward: B = %d must be in 1..65535", B);
  if (n_max < 1 || n_max > ((int64_t)1 << 30)) return dv_fail(DV_ERR_INVALID, "dv_resample_forward: n_max = %lld must be in 1..2^30", (long long)n_max);
  int64_t want = 0;
  for (const RsPair& d : h->h.pairs) {
    const int64_t v = (n_max * d.n + d.o - 1) / d.o;
    if (v > want) want = v;
  }
  if (n_out_max != want)
    return dv_fail(DV_ERR_INVALID, "dv_resample_forward: n_out_max = %lld, expected the largest ceil(new * n_max / orig) of the handle's pairs = %lld",
                   (long long)n_out_max, (long long)want);
  const int64_t tiles = (n_out_max + RS_TILE - 1) / RS_TILE;
  if (tiles > (1 << 23)) return dv_fail(DV_ERR_INVALID, "dv_resample_forward: n_out_max = %lld is more than one launch covers (2^32 samples)", (long long)n_out_max);
  if ((reinterpret_cast<uintptr_t>(wave) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(pair)) & 3 ||
      (reinterpret_cast<uintptr_t>(n_samples) | reinterpret_cast<uintptr_t>(n_out)) & 7)
    return dv_fail(DV_ERR_INVALID, "dv_resample_forward: misaligned pointer");
  const dim3 grid((unsigned)tiles, B);
  hipLaunchKernelGGL(k_resample, grid, dim3(RS_THREADS), h->h.lds_bytes, static_cast<hipStream_t>(stream), wave, n_samples, pair, h->h.n_pairs, n_max,
                     out, n_out_max, n_out, h->h.d_pairs, h->h.d_tabs, h->h.d_rngs);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return dv_fail(DV_ERR_HIP, "dv_resample_forward: launch failed: %s", hipGetErrorString(e));
  return DV_OK;
}

extern "C" void dv_resample_destroy(dv_resample* h) {
  if (!h) return;
  if (h->h.slab) (void)hipFree(h->h.slab);
  delete h;
}
