// Kernels of the native vocoder (voc.hip: the Vocos ConvNeXt-1D backbone and its ISTFT head; n_fft 1024, hop 256), over
// channels-last rows m = b * T + t of a RAGGED batch: utterance b holds L_b = lengths[b] frames (null lengths: T), a row with
// L_b outside [2, T] holds none.  Every row is its own utterance: a filter tap at t < 0 or t >= L_b reads zero, the overlap-add
// and its envelope use L_b frames, padding rows and the samples at or past n_b = (L_b - 1) * 256 are exact zeros.
//
//   k_voc_pack    mel [B, n_mels, T] -> split planes [B T, Kp] (32 x 32 transposes through LDS), keep mask [B T]
//   k_dw7_ln      depthwise 7-tap convolution + LayerNorm over the channels in one launch.  grid (ceil(T / 16), B), 256 threads:
//                 a workgroup stages its 16 rows and the +-3 halo once (zero outside [0, L_b)), a wave owns 4 of the rows, a lane
//                 the channels lane + 64 i (weights, gain and bias in registers, reused over the rows).  The row's mean and its
//                 variance about that mean (two passes over registers) are reduced within the wave (DPP, fixed order).  All fp32
//                 on the vector ALU: 7 MACs per element is not matrix-pipe work.
//   k_voc_gelu    fp32 [M, I] -> exact-erf GELU (gelu_erf, dv_device.h) -> split planes: the epilogue of pwconv1, as a kernel of the
//                 vocoder's own so that k_gemm's instantiations stay what they are.
//   k_istft_head  logits [B T, 1026] (log-magnitude | phase) -> waveform [B, (T - 1) 256] + samples [B].  grid (ceil((T - 1) / 9),
//                 B), 256 threads: a workgroup owns 9 consecutive 256-sample output blocks of one utterance and computes the 12
//                 frames that touch them (the three-frame halo is recomputed), three per wave.  Per frame: S = min(expf(m), 1e2)
//                 (cos p + i sin p) with the full-precision functions (phases reach tens of radians), the packed 512-point
//                 spectrum Z[k] = E[k] + i O[k] rebuilt with the W_1024 twiddles (the mirror image of k_log_mel's untangle; the
//                 imaginary parts of bins 0 and 512 are dropped as a C2R transform drops them), the inverse transform as the
//                 forward three radix-8 passes on conj Z, conjugated back (= conjugated twiddles), x 1 / 512, x window -> LDS.
//                 Then every thread sums, in ascending frame order, the up to four frames that cover each of its samples, divides
//                 by the squared-window envelope of the SAME frames (the utterance's own L_b) and stores coalesced.  No
//                 floating-point atomics: bit-reproducible.
// Ordering is by kernel boundary alone; nothing allocates, waits or hands over inside a launch.
#include "../../include/dvits_hip.h"
#include "dv_common.h"
#include "dv_device.h"
#include "fft512_device.h"

#include <vector>

namespace {

constexpr int VOC_NFFT = 1024, VOC_HOP = 256, VOC_HALF = 512, VOC_BINS = 513;
constexpr int VOC_ZPITCH = VOC_HALF + VOC_HALF / 8;         // FFT row of 512 words, one pad word per 8
constexpr int IST_BLOCKS = 9;                               // 256-sample output blocks per workgroup
constexpr int IST_FRAMES = IST_BLOCKS + 3;                  // frames that touch them
constexpr int DW_ROWS = 16, DW_HALO = 3, DW_STAGE = DW_ROWS + 2 * DW_HALO, DW_MAX_C = 512;

__device__ __forceinline__ int voc_len(const int64_t* __restrict__ lengths, int b, int T) {
  const long long L = lengths ? (long long)lengths[b] : (long long)T;
  return (L >= 2 && L <= (long long)T) ? (int)L : 0;
}
__device__ __forceinline__ void voc_split1(float v, bf16_t& h, bf16_t& l) {
  const unsigned hh = dv_cvt_pk_bf16(v, 0.f) & 0xffffu;
  h = (bf16_t)hh;
  l = (bf16_t)(dv_cvt_pk_bf16(v - __uint_as_float(hh << 16), 0.f) & 0xffffu);
}
__device__ __forceinline__ void voc_split4(const float4 v, uint2& hi, uint2& lo) {
  hi.x = dv_cvt_pk_bf16(v.x, v.y);
  hi.y = dv_cvt_pk_bf16(v.z, v.w);
  lo.x = dv_cvt_pk_bf16(v.x - __uint_as_float(hi.x << 16), v.y - __uint_as_float(hi.x & 0xffff0000u));
  lo.y = dv_cvt_pk_bf16(v.z - __uint_as_float(hi.y << 16), v.w - __uint_as_float(hi.y & 0xffff0000u));
}

__global__ __launch_bounds__(256) void k_voc_pack(const float* __restrict__ mel, const int64_t* __restrict__ lengths,
                                                   bf16_t* __restrict__ hi, bf16_t* __restrict__ lo, float* __restrict__ keep, int Cin,
                                                   int T, int Kp) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5, t0 = blockIdx.x * 32, b = blockIdx.y;
  const int Lb = voc_len(lengths, b, T);
  if (threadIdx.x < 32 && t0 + tx < T) keep[(size_t)b * T + t0 + tx] = t0 + tx < Lb ? 1.f : 0.f;
  for (int c0 = 0; c0 < Kp; c0 += 32) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = c0 + ty + 8 * i, t = t0 + tx;
      tile[ty + 8 * i][tx] = (c < Cin && t < Lb) ? mel[((size_t)b * Cin + c) * T + t] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int t = t0 + ty + 8 * i, c = c0 + tx;
      if (t < T) {
        bf16_t h, l;
        voc_split1(tile[tx][ty + 8 * i], h, l);
        const size_t o = ((size_t)b * T + t) * Kp + c;
        hi[o] = h;
        lo[o] = l;
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_dw7_ln(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                                 const int64_t* __restrict__ lengths, int T, int C, float eps, float* __restrict__ y,
                                                 bf16_t* __restrict__ y_hi, bf16_t* __restrict__ y_lo) {
  __shared__ __attribute__((aligned(16))) float s_x[DW_STAGE * DW_MAX_C];
  const int b = blockIdx.y, t0 = blockIdx.x * DW_ROWS, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const int Lb = voc_len(lengths, b, T);
  const int nc = C >> 6, c4n = C >> 2;
  const size_t row0 = (size_t)b * T;

  if (t0 >= Lb) {                                  // workgroup-uniform: nothing but padding rows here
    const int rows = min(DW_ROWS, T - t0);
    for (int e = tid; e < rows * c4n; e += 256) {
      const size_t o = (row0 + t0) * C + (size_t)e * 4;
      if (y) *reinterpret_cast<float4*>(y + o) = make_float4(0.f, 0.f, 0.f, 0.f);
      if (y_hi) *reinterpret_cast<uint2*>(y_hi + o) = make_uint2(0u, 0u);
      if (y_lo) *reinterpret_cast<uint2*>(y_lo + o) = make_uint2(0u, 0u);
    }
    return;
  }
  // rows t0 - 3 .. t0 + 18, zero outside the utterance's own [0, L_b)
  for (int e = tid; e < DW_STAGE * c4n; e += 256) {
    const int r = e / c4n, c4 = e - r * c4n, t = t0 - DW_HALO + r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t >= 0 && t < Lb) v = *reinterpret_cast<const float4*>(x + (row0 + t) * C + (size_t)c4 * 4);
    *reinterpret_cast<float4*>(s_x + r * C + c4 * 4) = v;
  }
  float wt[8][7], bs[8], gm[8], bt[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = lane + 64 * i;
    const bool on = i < nc;
#pragma unroll
    for (int k = 0; k < 7; ++k) wt[i][k] = on ? w[(size_t)c * 7 + k] : 0.f;
    bs[i] = on ? bias[c] : 0.f;
    gm[i] = on ? gamma[c] : 0.f;
    bt[i] = on ? beta[c] : 0.f;
  }
  __syncthreads();
  const float inv_c = 1.0f / (float)C;
  for (int rr = 0; rr < DW_ROWS / 4; ++rr) {
    const int r = wv * (DW_ROWS / 4) + rr, t = t0 + r;
    if (t >= T) break;                             // (wave-uniform)
    const size_t o = (row0 + t) * C;
    if (t >= Lb) {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (i < nc) {
          const int c = lane + 64 * i;
          if (y) y[o + c] = 0.f;
          if (y_hi) y_hi[o + c] = 0;
          if (y_lo) y_lo[o + c] = 0;
        }
      continue;
    }
    float v[8], d2[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      v[i] = 0.f;
      if (i < nc) {
        const float* col = s_x + r * C + lane + 64 * i;
        float a = bs[i];
#pragma unroll
        for (int k = 0; k < 7; ++k) a = fmaf(wt[i][k], col[k * C], a);
        v[i] = a;
      }
    }
    // (a pairwise tree: a row of equal values sums exactly where C / 64 is a power of two, so its variance is exactly 0)
    const float s = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    const float mu = wave_sum64(s) * inv_c;
#pragma unroll
    for (int i = 0; i < 8; ++i) { const float d = i < nc ? v[i] - mu : 0.f; d2[i] = d * d; }
    const float q = ((d2[0] + d2[1]) + (d2[2] + d2[3])) + ((d2[4] + d2[5]) + (d2[6] + d2[7]));
    const float rs = 1.0f / sqrtf(wave_sum64(q) * inv_c + eps);
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < nc) {
        const int c = lane + 64 * i;
        const float yv = fmaf((v[i] - mu) * rs, gm[i], bt[i]);
        if (y) y[o + c] = yv;
        if (y_hi) {
          bf16_t h, l;
          voc_split1(yv, h, l);
          y_hi[o + c] = h;
          if (y_lo) y_lo[o + c] = l;
        }
      }
  }
}

__global__ __launch_bounds__(256) void k_voc_gelu(const float* __restrict__ in, bf16_t* __restrict__ hi, bf16_t* __restrict__ lo, int64_t n4) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const float4 a = reinterpret_cast<const float4*>(in)[i];
    const float4 g = make_float4(gelu_erf(a.x), gelu_erf(a.y), gelu_erf(a.z), gelu_erf(a.w));
    uint2 h, l;
    voc_split4(g, h, l);
    reinterpret_cast<uint2*>(hi)[i] = h;
    reinterpret_cast<uint2*>(lo)[i] = l;
  }
}

// W'[n, :] = gamma[n] W[n, :] (one fp32 rounding), b'[n] = gamma[n] b[n]: the layer scale folded into pwconv2
__global__ void k_voc_fold_gamma(const float* __restrict__ W, const float* __restrict__ bvec, const float* __restrict__ gamma,
                                 float* __restrict__ Wo, float* __restrict__ bo, int N, int K) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)N * K) return;
  const int n = (int)(i / K);
  Wo[i] = gamma[n] * W[i];
  if (i - (size_t)n * K == 0) bo[n] = gamma[n] * bvec[n];
}

// S[k] of one frame: min(expf(m), 1e2) (cos p, sin p)
__device__ __forceinline__ void voc_bin(const float* __restrict__ row, int k, float& xr, float& xi) {
  const float mag = fminf(expf(row[k]), 1e2f);
  float sn, cs;
  sincosf(row[VOC_BINS + k], &sn, &cs);
  xr = mag * cs;
  xi = mag * sn;
}
// conj Z[k] and conj Z[512 - k] of the packed spectrum from A = S[k], B = S[512 - k]:
//   E = (A + conj B) / 2, O = (A - conj B) / 2 * conj W_1024^k, Z[k] = E + i O, Z[512 - k] = conj E + i conj O
__device__ __forceinline__ void voc_tangle(float ar, float ai, float br, float bi, float2 t, float& zr, float& zi, float& z2r, float& z2i) {
  const float er = 0.5f * (ar + br), ei = 0.5f * (ai - bi);
  const float dr = 0.5f * (ar - br), di = 0.5f * (ai + bi);
  const float orr = dr * t.x + di * t.y, oi = di * t.x - dr * t.y;       // D * conj t
  zr = er - oi; zi = -(ei + orr);
  z2r = er + oi; z2i = ei - orr;
}

__global__ __launch_bounds__(256) void k_istft_head(const float* __restrict__ logits, int ld, const float* __restrict__ window,
                                                     const int64_t* __restrict__ lengths, int T, float* __restrict__ wave,
                                                     int64_t* __restrict__ samples, const float2* __restrict__ tw512,
                                                     const float2* __restrict__ tw1024) {
  __shared__ float s_f[IST_FRAMES][2][VOC_ZPITCH];
  const int b = blockIdx.y, j0 = blockIdx.x * IST_BLOCKS, tid = threadIdx.x, wv = tid >> 6, l = tid & 63;
  const int Lb = voc_len(lengths, b, T);
  const int nb = Lb > 0 ? (Lb - 1) * VOC_HOP : 0;
  const int n_out = (T - 1) * VOC_HOP;
  if (blockIdx.x == 0 && tid == 0) samples[b] = nb;
  float* const orow = wave + (size_t)b * n_out;

  if (j0 * VOC_HOP >= nb) {                        // workgroup-uniform: nothing but padding here
    for (int jj = 0; jj < IST_BLOCKS; ++jj) {
      const int j = j0 + jj;
      if (j >= T - 1) break;
      orow[(size_t)j * VOC_HOP + tid] = 0.f;
    }
    return;
  }

  const float2* const win2 = reinterpret_cast<const float2*>(window);
  float xr[8], xi[8];
  for (int it = 0; it < IST_FRAMES / 4; ++it) {
    const int slot = wv + 4 * it, f = j0 - 1 + slot;
    const bool live = f >= 0 && f < Lb;            // (wave-uniform)
    float* const re = s_f[slot][0];
    float* const im = s_f[slot][1];
    if (live) {
      const float* const row = logits + ((size_t)b * T + f) * ld;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = l + 64 * r, k2 = VOC_HALF - k;
        float ar, ai, br, bi, zr, zi, z2r, z2i;
        voc_bin(row, k, ar, ai);
        voc_bin(row, k2, br, bi);
        if (k == 0) { ai = 0.f; bi = 0.f; }        // bins 0 and 512 are real
        voc_tangle(ar, ai, br, bi, tw1024[k], zr, zi, z2r, z2i);
        re[zpad(k)] = zr; im[zpad(k)] = zi;
        if (k != 0) { re[zpad(k2)] = z2r; im[zpad(k2)] = z2i; }
      }
      if (l == 0) {                                // k = 256 pairs with itself: Z[256] = conj S[256]
        float ar, ai;
        voc_bin(row, 256, ar, ai);
        re[zpad(256)] = ar; im[zpad(256)] = ai;    // (stored conjugated: conj conj S)
      }
    } else {
#pragma unroll
      for (int r = 0; r < 8; ++r) { re[zpad(l + 64 * r)] = 0.f; im[zpad(l + 64 * r)] = 0.f; }
    }
    __syncthreads();
    // pass 1 (length 512, stride 1): lane = p, reads z[p + 64 j], writes y[8 p + k] W_512^(p k)
#pragma unroll
    for (int j = 0; j < 8; ++j) { xr[j] = re[zpad(l + 64 * j)]; xi[j] = im[zpad(l + 64 * j)]; }
    __syncthreads();
    dft8(xr, xi);
    re[zpad(8 * l)] = xr[0];
    im[zpad(8 * l)] = xi[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) {
      const float2 t = tw512[l * k];
      re[zpad(8 * l + k)] = xr[k] * t.x - xi[k] * t.y;
      im[zpad(8 * l + k)] = xr[k] * t.y + xi[k] * t.x;
    }
    __syncthreads();
    // pass 2 (length 64, stride 8): lane = (p, q) = (l / 8, l % 8), reads x[l + 64 j], writes y[q + 8 (8 p + k)] W_64^(p k)
#pragma unroll
    for (int j = 0; j < 8; ++j) { xr[j] = re[zpad(l + 64 * j)]; xi[j] = im[zpad(l + 64 * j)]; }
    __syncthreads();
    dft8(xr, xi);
    {
      const int p = l >> 3, q = l & 7;
      re[zpad(q + 64 * p)] = xr[0];
      im[zpad(q + 64 * p)] = xi[0];
#pragma unroll
      for (int k = 1; k < 8; ++k) {
        const float2 t = tw512[8 * p * k];
        re[zpad(q + 64 * p + 8 * k)] = xr[k] * t.x - xi[k] * t.y;
        im[zpad(q + 64 * p + 8 * k)] = xr[k] * t.y + xi[k] * t.x;
      }
    }
    __syncthreads();
    // pass 3 (length 8, stride 64): lane = q, reads x[q + 64 j], writes the slots it has just read: z[m] = conj(Y[m]) / 512, so
    // samples 2 m = Re Y / 512, 2 m + 1 = -Im Y / 512, each times its window value
#pragma unroll
    for (int j = 0; j < 8; ++j) { xr[j] = re[zpad(l + 64 * j)]; xi[j] = im[zpad(l + 64 * j)]; }
    dft8(xr, xi);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int m = l + 64 * k;
      const float2 wn = win2[m];
      re[zpad(m)] = live ? (xr[k] * (1.0f / 512.0f)) * wn.x : 0.f;
      im[zpad(m)] = live ? (xi[k] * (-1.0f / 512.0f)) * wn.y : 0.f;
    }
  }
  __syncthreads();
  // overlap-add: sample n of block j lies at position n + 512 of the untrimmed signal, offset tid + 768 - 256 s of frame j - 1 + s
  for (int jj = 0; jj < IST_BLOCKS; ++jj) {
    const int j = j0 + jj;
    if (j >= T - 1) break;
    const int n = j * VOC_HOP + tid;
    float v = 0.f;
    if (n < nb) {
      float env = 0.f;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int f = j - 1 + s;
        if (f >= 0 && f < Lb) {
          const int o = tid + 768 - 256 * s, m = o >> 1;
          v += s_f[jj + s][o & 1][zpad(m)];
          const float wn = window[o];
          env = fmaf(wn, wn, env);
        }
      }
      v = v / env;
    }
    orow[n] = v;
  }
}

struct VocTables { float2* slab = nullptr; };
VocTables g_voc_tab;

}  // namespace

hipError_t voc_init() {
  if (g_voc_tab.slab) return hipSuccess;
  std::vector<float2> host(1024);
  fft512_fill_tables(host.data(), host.data() + 512);
  float2* d = nullptr;
  hipError_t e = hipMalloc((void**)&d, host.size() * sizeof(float2));
  if (e != hipSuccess) return e;
  e = hipMemcpy(d, host.data(), host.size() * sizeof(float2), hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(d); return e; }
  g_voc_tab.slab = d;
  return hipSuccess;
}

hipError_t launch_voc_pack(const float* mel, const int64_t* lengths, bf16_t* hi, bf16_t* lo, float* keep, int B, int Cin, int T, int Kp,
                           hipStream_t st) {
  if (B < 1 || B > 65535 || T < 1 || Cin < 1 || Kp % 32 != 0 || Kp < Cin) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_voc_pack, dim3((T + 31) / 32, B), dim3(256), 0, st, mel, lengths, hi, lo, keep, Cin, T, Kp);
  return hipGetLastError();
}

bool dw7_ln_supported(int C) { return C >= 64 && C <= DW_MAX_C && C % 64 == 0; }

hipError_t launch_dw7_ln(const float* x, const float* w, const float* bias, const float* gamma, const float* beta, const int64_t* lengths,
                         int B, int T, int C, float eps, float* y, bf16_t* y_hi, bf16_t* y_lo, hipStream_t st) {
  if (B < 1 || B > 65535 || T < 1 || !dw7_ln_supported(C) || (y_lo && !y_hi)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_dw7_ln, dim3((T + DW_ROWS - 1) / DW_ROWS, B), dim3(256), 0, st, x, w, bias, gamma, beta, lengths, T, C, eps, y,
                     y_hi, y_lo);
  return hipGetLastError();
}

hipError_t launch_voc_gelu(const float* in, bf16_t* hi, bf16_t* lo, int64_t n, hipStream_t st) {
  if (n < 4 || n % 4 != 0) return hipErrorInvalidValue;
  const int64_t n4 = n / 4;
  const int64_t blocks = (n4 + 255) / 256;
  hipLaunchKernelGGL(k_voc_gelu, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, st, in, hi, lo, n4);
  return hipGetLastError();
}

hipError_t launch_voc_fold_gamma(const float* W, const float* b, const float* gamma, float* Wo, float* bo, int N, int K, hipStream_t st) {
  const size_t n = (size_t)N * K;
  hipLaunchKernelGGL(k_voc_fold_gamma, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, W, b, gamma, Wo, bo, N, K);
  return hipGetLastError();
}

hipError_t launch_istft_head(const float* logits, int ld, const float* window, const int64_t* lengths, int B, int T, float* wave,
                             int64_t* samples, hipStream_t st) {
  if (B < 1 || B > 65535 || T < 1 || T > (1 << 22) || ld < 2 * VOC_BINS || !g_voc_tab.slab) return hipErrorInvalidValue;
  const int gx = T > 1 ? (T - 1 + IST_BLOCKS - 1) / IST_BLOCKS : 1;
  hipLaunchKernelGGL(k_istft_head, dim3(gx, B), dim3(256), 0, st, logits, ld, window, lengths, T, wave, samples, g_voc_tab.slab,
                     g_voc_tab.slab + 512);
  return hipGetLastError();
}
