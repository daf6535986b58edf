// Log-mel front-end (mel.py MelSpectrogram / reference_mel_prompt: n_fft 1024, hop 256, center with reflect padding, one-sided,
// power 1 or 2, optional log(clip)) for a RAGGED batch of recordings in ONE launch: waveform [B, n_max] + n_samples [B] ->
// out [B, n_mels, L_max] + frames [B], L_b = 1 + n_b / hop, every element at or past L_b exactly zero.
//
//   k_log_mel   grid (ceil(L_max / 4), B), 256 threads: one wavefront per frame, four neighbouring frames of one recording per
//               workgroup, so the 1792 samples they cover (75 % overlap) are read once into LDS - reflected about the RECORDING's
//               own ends (i < 0 -> -i, i >= n_b -> 2 (n_b - 1) - i); no sample at an index >= n_b is ever read.
//               Per frame: the windowed samples packed as z[m] = x[2m] + i x[2m + 1], a 512-point complex FFT as three radix-8
//               Stockham passes (64 lanes x 8 points, exchanged through LDS: the 8-stride store of pass 1 and the 8 / 64-stride store
//               of pass 2 go to rows padded by one word per 8, conflict-free), the untangle to 513 bins with the W_1024 twiddles,
//               sqrtf magnitude (squared for power 2), then per mel band the sum of fb[k, m] * mag[k] over the band's bin range in
//               ascending k (lane = band), optional logf(fmaxf(v, clip)).  The four frames' bands are exchanged once more so that
//               four neighbouring lanes store four neighbouring frames of one band.
//               All of it is fp32 on the vector ALU: a DFT by split bf16 planes on the matrix pipe carries ~2^-16 of the frame's
//               norm per product, which bands 80 dB under the frame's peak do not survive (profiles/mel_reference.txt).
//               A workgroup whose four frames all lie at or past L_b writes zeros and leaves (a workgroup-uniform branch); a row
//               whose n_b is outside [n_fft / 2 + 1, n_max] is all zeros with frames[b] = 0 - a value to check, not a fault.
// Twiddles (fp64 on the host, rounded once), the window and the filterbank are device tables of a handle, built at create from the
// caller's arrays: both backends of mel.py share the constants bit for bit.  The per-band bin range is the first / last non-zero
// row of each fb column; the dense weights inside it are used, so any filterbank is handled, not only triangles.
// Ordering is by kernel boundary alone; nothing allocates, waits or hands over inside a launch.
#include "../../include/dvits_hip.h"
#include "dv_common.h"
#include "fft512_device.h"

#include <cmath>
#include <new>
#include <vector>

int dv_fail(int code, const char* fmt, ...);

namespace {

constexpr int MEL_NFFT = 1024, MEL_HOP = 256, MEL_BINS = 513, MEL_HALF = 512;
constexpr int MEL_FPW = 4;                                            // frames (= wavefronts) per workgroup
constexpr int MEL_THREADS = 64 * MEL_FPW;
constexpr int MEL_STAGE = MEL_NFFT + (MEL_FPW - 1) * MEL_HOP;         // samples the workgroup's frames cover
constexpr int MEL_ZPITCH = MEL_HALF + MEL_HALF / 8;                   // FFT row of 512 words, one pad word per 8
constexpr int MEL_MAX_MELS = 128;

struct MelTables {
  const float2* tw512;     // [512]  exp(-2 pi i t / 512)
  const float2* tw1024;    // [512]  exp(-2 pi i t / 1024)
  const float2* window2;   // [512]  (window[2m], window[2m + 1])
  const float* fb;         // [513, n_mels]
  const int2* band;        // [n_mels] (first, last) non-zero bin; (0, -1): empty band
};

__global__ __launch_bounds__(MEL_THREADS) void k_log_mel(const float* __restrict__ wave, const int64_t* __restrict__ n_samples,
                                                         int n_max, float* __restrict__ out, int64_t* __restrict__ frames, int L_max,
                                                         int n_mels, int do_log, int power2, float clip, MelTables tb) {
  __shared__ __attribute__((aligned(16))) float s_stage[MEL_STAGE];
  __shared__ float s_re[MEL_FPW][MEL_ZPITCH];
  __shared__ float s_im[MEL_FPW][MEL_ZPITCH];
  __shared__ float s_mag[MEL_FPW][MEL_BINS + 7];
  __shared__ float s_mel[MEL_MAX_MELS][MEL_FPW];

  const int b = blockIdx.y, f0 = blockIdx.x * MEL_FPW, tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  const int64_t nb64 = n_samples[b];
  const bool row_ok = nb64 >= MEL_HALF + 1 && nb64 <= (int64_t)n_max;
  const int nb = row_ok ? (int)nb64 : 0;
  const int Lb = row_ok ? 1 + nb / MEL_HOP : 0;
  if (blockIdx.x == 0 && tid == 0) frames[b] = Lb;
  float* const orow = out + (size_t)b * n_mels * L_max;

  if (f0 >= Lb) {                                  // workgroup-uniform: nothing but padding here
    for (int e = tid; e < n_mels * MEL_FPW; e += MEL_THREADS) {
      const int m = e >> 2, f = f0 + (e & 3);
      if (f < L_max) orow[(size_t)m * L_max + f] = 0.f;
    }
    return;
  }

  // the samples of frames f0 .. f0 + 3, reflected about the recording's own ends.  A position that only frames at or past L_b
  // touch can reflect outside [0, n_b): it is staged as zero and its frame's result is discarded below.
  {
    const float* wrow = wave + (size_t)b * n_max;
    const int s0 = f0 * MEL_HOP - MEL_HALF;
    for (int t = tid; t < MEL_STAGE; t += MEL_THREADS) {
      int i = s0 + t;
      if (i < 0) i = -i;
      if (i >= nb) i = 2 * (nb - 1) - i;
      s_stage[t] = (i >= 0 && i < nb) ? wrow[i] : 0.f;
    }
  }
  __syncthreads();

  float xr[8], xi[8];
  float* const re = s_re[w];
  float* const im = s_im[w];
  // pass 1 (length 512, stride 1): lane = p, reads z[p + 64 j], writes y[8 p + k] W_512^(p k)
  {
    const float2* st2 = reinterpret_cast<const float2*>(s_stage) + w * (MEL_HOP / 2);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float2 s = st2[l + 64 * j];
      const float2 wn = tb.window2[l + 64 * j];
      xr[j] = s.x * wn.x;
      xi[j] = s.y * wn.y;
    }
    dft8(xr, xi);
    re[zpad(8 * l)] = xr[0];
    im[zpad(8 * l)] = xi[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) {
      const float2 t = tb.tw512[l * k];
      re[zpad(8 * l + k)] = xr[k] * t.x - xi[k] * t.y;
      im[zpad(8 * l + k)] = xr[k] * t.y + xi[k] * t.x;
    }
  }
  __syncthreads();
  // pass 2 (length 64, stride 8): lane = (p, q) = (l / 8, l % 8), reads x[l + 64 j], writes y[q + 8 (8 p + k)] W_64^(p k)
  {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      xr[j] = re[zpad(l + 64 * j)];
      xi[j] = im[zpad(l + 64 * j)];
    }
    __syncthreads();
    dft8(xr, xi);
    const int p = l >> 3, q = l & 7;
    re[zpad(q + 64 * p)] = xr[0];
    im[zpad(q + 64 * p)] = xi[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) {
      const float2 t = tb.tw512[8 * p * k];
      re[zpad(q + 64 * p + 8 * k)] = xr[k] * t.x - xi[k] * t.y;
      im[zpad(q + 64 * p + 8 * k)] = xr[k] * t.y + xi[k] * t.x;
    }
  }
  __syncthreads();
  // pass 3 (length 8, stride 64): lane = q, reads x[q + 64 j], writes Z[q + 64 k] - the slots this lane has just read
  {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      xr[j] = re[zpad(l + 64 * j)];
      xi[j] = im[zpad(l + 64 * j)];
    }
    dft8(xr, xi);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      re[zpad(l + 64 * k)] = xr[k];
      im[zpad(l + 64 * k)] = xi[k];
    }
  }
  __syncthreads();
  // untangle: X[k] = (Z[k] + conj Z[512 - k]) / 2 + W_1024^k (-i) (Z[k] - conj Z[512 - k]) / 2,  X[512] = Re Z[0] - Im Z[0]
  {
    float* const mag = s_mag[w];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int k = l + 64 * r, k2 = (MEL_HALF - k) & (MEL_HALF - 1);
      const float ar = re[zpad(k)], ai = im[zpad(k)], cr = re[zpad(k2)], ci = -im[zpad(k2)];
      const float er = 0.5f * (ar + cr), ei = 0.5f * (ai + ci);
      const float orr = 0.5f * (ai - ci), oi = -0.5f * (ar - cr);
      const float2 t = tb.tw1024[k];
      const float Xr = er + (orr * t.x - oi * t.y), Xi = ei + (orr * t.y + oi * t.x);
      const float mg = sqrtf(Xr * Xr + Xi * Xi);
      mag[k] = power2 ? mg * mg : mg;
    }
    if (l == 0) {
      const float mg = fabsf(re[0] - im[0]);
      mag[MEL_HALF] = power2 ? mg * mg : mg;
    }
  }
  __syncthreads();
  // mel bands: lane = band, ascending k over the band's own bin range
  {
    const float* const mag = s_mag[w];
    const bool live = f0 + w < Lb;
    for (int m = l; m < n_mels; m += 64) {
      const int2 bd = tb.band[m];
      float acc = 0.f;
      for (int k = bd.x; k <= bd.y; ++k) acc += tb.fb[(size_t)k * n_mels + m] * mag[k];
      if (do_log) acc = logf(fmaxf(acc, clip));
      s_mel[m][w] = live ? acc : 0.f;
    }
  }
  __syncthreads();
  for (int e = tid; e < n_mels * MEL_FPW; e += MEL_THREADS) {
    const int m = e >> 2, f = f0 + (e & 3);
    if (f < L_max) orow[(size_t)m * L_max + f] = s_mel[m][e & 3];
  }
}

struct MelHandle {
  int n_mels = 0;
  float clip = 0.f;
  void* slab = nullptr;
  MelTables tb{};
};

}  // namespace

struct dv_mel { MelHandle h; };

extern "C" int dv_mel_create(const dv_mel_cfg* cfg, const float* window, const float* fb, dv_mel** out) {
  if (!cfg || !window || !fb || !out) return dv_fail(DV_ERR_INVALID, "dv_mel_create: null argument");
  *out = nullptr;
  if (cfg->n_fft != MEL_NFFT || cfg->hop_length != MEL_HOP)
    return dv_fail(DV_ERR_INVALID, "dv_mel_create: n_fft = %d, hop_length = %d: only 1024 / 256 are built", cfg->n_fft, cfg->hop_length);
  if (cfg->center != 1) return dv_fail(DV_ERR_INVALID, "dv_mel_create: center = %d: only centred frames with reflect padding are built", cfg->center);
  if (cfg->n_mels < 1 || cfg->n_mels > MEL_MAX_MELS)
    return dv_fail(DV_ERR_INVALID, "dv_mel_create: n_mels = %d must be in 1..%d", cfg->n_mels, MEL_MAX_MELS);
  if (!(cfg->log_clip > 0.f) || !std::isfinite(cfg->log_clip))
    return dv_fail(DV_ERR_INVALID, "dv_mel_create: log_clip %g must be finite and > 0", (double)cfg->log_clip);
  const int M = cfg->n_mels;
  for (int i = 0; i < MEL_NFFT; ++i)
    if (!std::isfinite(window[i])) return dv_fail(DV_ERR_INVALID, "dv_mel_create: window[%d] is not finite", i);
  for (int64_t i = 0; i < (int64_t)MEL_BINS * M; ++i)
    if (!std::isfinite(fb[i])) return dv_fail(DV_ERR_INVALID, "dv_mel_create: fb[%lld] is not finite", (long long)i);

  // one slab: tw512 | tw1024 | window pairs | fb | bands
  const size_t o_tw512 = 0, o_tw1024 = o_tw512 + 512 * sizeof(float2), o_win = o_tw1024 + 512 * sizeof(float2);
  const size_t o_fb = o_win + 512 * sizeof(float2), o_band = (o_fb + (size_t)MEL_BINS * M * sizeof(float) + 15) / 16 * 16;
  const size_t bytes = o_band + (size_t)M * sizeof(int2);
  std::vector<char> host(bytes, 0);
  float2* tw512 = reinterpret_cast<float2*>(host.data() + o_tw512);
  float2* tw1024 = reinterpret_cast<float2*>(host.data() + o_tw1024);
  float2* win2 = reinterpret_cast<float2*>(host.data() + o_win);
  float* fbh = reinterpret_cast<float*>(host.data() + o_fb);
  int2* band = reinterpret_cast<int2*>(host.data() + o_band);
  fft512_fill_tables(tw512, tw1024);
  for (int t = 0; t < 512; ++t) win2[t] = make_float2(window[2 * t], window[2 * t + 1]);
  for (int64_t i = 0; i < (int64_t)MEL_BINS * M; ++i) fbh[i] = fb[i];
  for (int m = 0; m < M; ++m) {
    int lo = 0, hi = -1;
    for (int k = 0; k < MEL_BINS; ++k)
      if (fb[(size_t)k * M + m] != 0.f) {
        if (hi < 0) lo = k;
        hi = k;
      }
    band[m] = make_int2(lo, hi);
  }
  dv_mel* h = new (std::nothrow) dv_mel();
  if (!h) return dv_fail(DV_ERR_INVALID, "dv_mel_create: out of host memory");
  hipError_t e = hipMalloc(&h->h.slab, bytes);
  if (e == hipSuccess) e = hipMemcpy(h->h.slab, host.data(), bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (h->h.slab) (void)hipFree(h->h.slab);
    delete h;
    return dv_fail(DV_ERR_HIP, "dv_mel_create: device tables: %s", hipGetErrorString(e));
  }
  char* d = static_cast<char*>(h->h.slab);
  h->h.n_mels = M;
  h->h.clip = cfg->log_clip;
  h->h.tb.tw512 = reinterpret_cast<const float2*>(d + o_tw512);
  h->h.tb.tw1024 = reinterpret_cast<const float2*>(d + o_tw1024);
  h->h.tb.window2 = reinterpret_cast<const float2*>(d + o_win);
  h->h.tb.fb = reinterpret_cast<const float*>(d + o_fb);
  h->h.tb.band = reinterpret_cast<const int2*>(d + o_band);
  *out = h;
  return DV_OK;
}

extern "C" int dv_mel_forward(dv_mel* h, const float* wave, const int64_t* n_samples, int32_t B, int32_t n_max, float* out,
                              int64_t* frames, int32_t L_max, int32_t flags, void* stream) {
  if (!h || !wave || !n_samples || !out || !frames) return dv_fail(DV_ERR_INVALID, "dv_mel_forward: null argument");
  if (B < 1 || B > 65535) return dv_fail(DV_ERR_INVALID, "dv_mel_forward: B = %d must be in 1..65535", B);
  if (n_max < MEL_HALF + 1 || n_max > (1 << 30))
    return dv_fail(DV_ERR_INVALID, "dv_mel_forward: n_max = %d must be in %d..2^30 (reflect padding needs n_fft / 2 + 1 samples)", n_max, MEL_HALF + 1);
  if (L_max != 1 + n_max / MEL_HOP) return dv_fail(DV_ERR_INVALID, "dv_mel_forward: L_max = %d, expected 1 + n_max / hop = %d", L_max, 1 + n_max / MEL_HOP);
  if (flags & ~(DV_MEL_LOG | DV_MEL_POWER2)) return dv_fail(DV_ERR_INVALID, "dv_mel_forward: unknown flag bits 0x%x", flags);
  if ((reinterpret_cast<uintptr_t>(wave) | reinterpret_cast<uintptr_t>(out)) & 3 || (reinterpret_cast<uintptr_t>(n_samples) | reinterpret_cast<uintptr_t>(frames)) & 7)
    return dv_fail(DV_ERR_INVALID, "dv_mel_forward: misaligned pointer");
  const dim3 grid((L_max + MEL_FPW - 1) / MEL_FPW, B);
  hipLaunchKernelGGL(k_log_mel, grid, dim3(MEL_THREADS), 0, static_cast<hipStream_t>(stream), wave, n_samples, n_max, out, frames, L_max,
                     h->h.n_mels, (flags & DV_MEL_LOG) ? 1 : 0, (flags & DV_MEL_POWER2) ? 1 : 0, h->h.clip, h->h.tb);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return dv_fail(DV_ERR_HIP, "dv_mel_forward: launch failed: %s", hipGetErrorString(e));
  return DV_OK;
}

extern "C" void dv_mel_destroy(dv_mel* h) {
  if (!h) return;
  if (h->h.slab) (void)hipFree(h->h.slab);
  delete h;
}
