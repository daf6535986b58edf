// The posterior encoder's WaveNet stack on gfx950 (MI355X): reference modules.WN (modules.py:133-210) under
// model3.PosteriorEncoder (model3.py:526-572), as the forced aligner runs it (k = 5, dilation 1, H = 256, 16 layers).
//
// k_wn_layer<H> - ONE launch per WaveNet layer.  Rows are channels-last, m = b * T + t (row pitch T, no padding rows between
// utterances); a workgroup owns BM = 64 rows of ONE utterance (grid = B * ceil(T / 64); the last tile of an utterance is
// short: its rows beyond T are computed on zeros and never stored), 8 waves:
//   1. the tile's rows and a two-row halo on each side (68 rows) are staged into LDS as hi / lo bf16 planes.  A row whose
//      frame lies outside [0, lengths[b]) is written as zeros - it is never read from memory, so it is neither the
//      neighbouring utterance's row nor an out-of-bounds address;
//   2. the five-tap contraction [64 x 5H] x [5H x 2H]: three bf16 products per 16-deep k-step (hi*lo + lo*hi + hi*hi, fp32
//      accumulation), K order (tap, channel).  The weights never touch LDS: fragment-major (launch_relayout_frag), packed
//      like the GEGLU tiles of k_gemm - rows [64 j, 64 j + 32) are the tanh channels 32 j .. 32 j + 31, the next 32 the
//      sigmoid channels H + 32 j ..: wave j multiplies both fragments with both row fragments and so holds both halves of
//      every gate pair of its 32 channels;
//   3. epilogue: + bias + the utterance's conditioning slice cond[b, 2H i + c] (none without g), then
//      acts = tanh(a_c) * sigmoid(a_{c + H}) in fp32 (forms and error below), times the row's keep flag;
//   4. the gated activations go to LDS as split planes - they never go to memory (keep mode: a copy for the probe);
//   5. the 1x1 contraction [64 x H] x [H x 2H] (last layer: H x H): wave j takes output fragment j (residual half) and
//      H / 32 + j (skip half);
//   6. epilogue: x_next = (x + rs[:, :H]) * keep is written to the OTHER x buffer (fp32 + planes) - neighbouring tiles still
//      read this layer's input as their halo; skip += rs[:, H:] * keep in place on the tile's own rows (first layer: skip =);
//      last layer: every output column goes to skip, x is not written, and the split planes of the finished skip sum are
//      written for proj.
// LDS: (68 + 64) rows x (2 H + 16) bytes x 2 planes = 136.1 KiB at H = 256 (the 16 bytes of padding per row spread the rows of
// a fragment read over the banks).
//
// Transcendentals (fp32, accurate expf - not the hardware approximation):
//   tanh(a)    = sign(a) * (1 - e) / (1 + e),  e = expf(-2 |a|)      |error| <= 2.5e-7 absolute (expf: 1 ulp of e <= 1, the
//                                                                     difference 1 - e and the division: 0.5 ulp of <= 1 each)
//   sigmoid(b) = 1 / (1 + expf(-b))                                   |error| <= 2e-7 absolute (expf(-b) = inf for b < -88.7
//                                                                     gives exactly 0, as the reference's float32 does)
// so |error of tanh(a) * sigmoid(b)| <= 4.5e-7 on top of what the errors of a and b themselves contribute (WN_ACT_ERR in tests/qenc_cases.py, whose
// host emulation of this arithmetic sets the per-frame bound of the layerN.acts probes).
//
// Launches per forward: n_layers + 4, with or without g, with or without kept intermediates:
//   k_wn_pack (mel -> channels-last planes padded to K = 128, keep mask; its tail blocks are the conditioning 1x1 g -> [B, 2H L])
//   k_gemm pre (row mask) -> n_layers x k_wn_layer -> k_gemm proj (row mask) -> k_wn_store (m, logs, z channels-first).
#include "dv_common.h"
#include "dv_device.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

namespace {

constexpr int WN_BM = 64, WN_HALO = 2, WN_XR = WN_BM + 2 * WN_HALO, WN_NT = 512;
template <int H>
struct WnGeom {
  static constexpr int RS = 2 * H + 16;              // bytes of one LDS row of one plane
  static constexpr int X_PL = WN_XR * RS;            // bytes of one plane of the staged rows
  static constexpr int A_PL = WN_BM * RS;            // ... of the gated activations
  static constexpr int SMEM = 2 * X_PL + 2 * A_PL;
  static constexpr int KPT = H / 16;                 // 16-deep k-steps per tap
  static constexpr int KS1 = 5 * KPT, KS2 = KPT;
  static_assert(H % 32 == 0 && H / 32 == WN_NT / 64 && SMEM <= 160 * 1024, "one wave per 32 gate pairs; the two images fit the LDS");
};

__device__ __forceinline__ float wn_tanh(float a) {
  const float e = expf(-2.0f * fabsf(a));
  return copysignf((1.0f - e) / (1.0f + e), a);
}
__device__ __forceinline__ float wn_sigmoid(float b) { return 1.0f / (1.0f + expf(-b)); }

__device__ __forceinline__ int wn_len(const int64_t* lengths, int b, int T) {
  const long long l = lengths[b];
  return (int)(l < 0 ? 0 : (l > T ? T : l));
}

struct WFrag { bf16x8 h, l; };

template <int H>
__global__ __launch_bounds__(WN_NT) void k_wn_layer(const WnLayerParams p) {
  using G = WnGeom<H>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const xs = smem;
  char* const gs = smem + 2 * G::X_PL;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, lh = lane >> 5;
  const int b = blockIdx.x / p.tiles_per_utt, t0 = (blockIdx.x - b * p.tiles_per_utt) * WN_BM;
  const int len = wn_len(p.lengths, b, p.T);
  const size_t mb = (size_t)b * p.T;

  // ---- 1. rows [t0 - 2, t0 + 66) of the utterance, both planes; frames outside [0, len) are zeros and are not read ----
  {
    constexpr int PIECES = H / 8, PER_PL = WN_XR * PIECES;
    for (int i = tid; i < 2 * PER_PL; i += WN_NT) {
      const int pl = i / PER_PL, rem = i - pl * PER_PL, r = rem / PIECES, pc = rem - r * PIECES;
      const int t = t0 - WN_HALO + r;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (t >= 0 && t < len) v = *reinterpret_cast<const uint4*>((pl ? p.xl_in : p.xh_in) + (mb + t) * H + pc * 8);
      *reinterpret_cast<uint4*>(xs + pl * G::X_PL + r * G::RS + pc * 16) = v;
    }
  }
  __syncthreads();

  // ---- 2. five taps: acc[cf][rf] += W[fragment 2 wave + cf][k-step] x A^T[row fragment rf][k-step] ----
  f32x16 acc[2][2];
#pragma unroll
  for (int cf = 0; cf < 2; ++cf)
#pragma unroll
    for (int rf = 0; rf < 2; ++rf)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[cf][rf][r] = 0.f;
  {
    const size_t w0 = ((size_t)(2 * wave) * G::KS1 * 64 + lane) * 8;
    const bf16_t* const wh = p.w1_hi + w0;
    const bf16_t* const wl = p.w1_lo + w0;
    auto load_w = [&](int ks, WFrag (&f)[2]) {
#pragma unroll
      for (int cf = 0; cf < 2; ++cf) {
        f[cf].h = *reinterpret_cast<const bf16x8*>(wh + ((size_t)cf * G::KS1 + ks) * 512);
        f[cf].l = *reinterpret_cast<const bf16x8*>(wl + ((size_t)cf * G::KS1 + ks) * 512);
      }
    };
    const int rbase = l31 * G::RS + lh * 16;
    WFrag cur[2], nxt[2];
    load_w(0, cur);
#pragma unroll 2
    for (int ks = 0; ks < G::KS1; ++ks) {
      load_w(ks + 1 < G::KS1 ? ks + 1 : ks, nxt);
      const int tap = ks / G::KPT, cs = ks - tap * G::KPT;
      bf16x8 ah[2], al[2];
#pragma unroll
      for (int rf = 0; rf < 2; ++rf) {
        const int off = rbase + (rf * 32 + tap) * G::RS + cs * 32;   // LDS row 0 is frame t0 - 2: tap k reads frame t + k - 2
        ah[rf] = *reinterpret_cast<const bf16x8*>(xs + off);
        al[rf] = *reinterpret_cast<const bf16x8*>(xs + G::X_PL + off);
      }
#pragma unroll
      for (int cf = 0; cf < 2; ++cf)
#pragma unroll
        for (int rf = 0; rf < 2; ++rf) {
          acc[cf][rf] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cur[cf].h, al[rf], acc[cf][rf], 0, 0, 0);
          acc[cf][rf] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cur[cf].l, ah[rf], acc[cf][rf], 0, 0, 0);
          acc[cf][rf] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cur[cf].h, ah[rf], acc[cf][rf], 0, 0, 0);
        }
      cur[0] = nxt[0]; cur[1] = nxt[1];
    }
  }

  // ---- 3. / 4. bias + conditioning, gate, split planes into LDS.  acc[.][rf][4 g + e] = row rf * 32 + l31, channel 32 wave + 8 g + 4 lh + e
  {
    const float* const cnd = p.cond ? p.cond + (size_t)b * p.ld_cond + p.cond_off : nullptr;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int c0 = 32 * wave + 8 * g + 4 * lh;
      float4 ba = *reinterpret_cast<const float4*>(p.b1 + c0), bg = *reinterpret_cast<const float4*>(p.b1 + H + c0);
      if (cnd) {
        const float4 ca = *reinterpret_cast<const float4*>(cnd + c0), cg = *reinterpret_cast<const float4*>(cnd + H + c0);
        // (the reference adds the bias inside the convolution, then the slice: two roundings in that order)
#pragma unroll
        for (int rf = 0; rf < 2; ++rf) {
          acc[0][rf][4 * g] = (acc[0][rf][4 * g] + ba.x) + ca.x; acc[0][rf][4 * g + 1] = (acc[0][rf][4 * g + 1] + ba.y) + ca.y;
          acc[0][rf][4 * g + 2] = (acc[0][rf][4 * g + 2] + ba.z) + ca.z; acc[0][rf][4 * g + 3] = (acc[0][rf][4 * g + 3] + ba.w) + ca.w;
          acc[1][rf][4 * g] = (acc[1][rf][4 * g] + bg.x) + cg.x; acc[1][rf][4 * g + 1] = (acc[1][rf][4 * g + 1] + bg.y) + cg.y;
          acc[1][rf][4 * g + 2] = (acc[1][rf][4 * g + 2] + bg.z) + cg.z; acc[1][rf][4 * g + 3] = (acc[1][rf][4 * g + 3] + bg.w) + cg.w;
        }
      } else {
#pragma unroll
        for (int rf = 0; rf < 2; ++rf) {
          acc[0][rf][4 * g] += ba.x; acc[0][rf][4 * g + 1] += ba.y; acc[0][rf][4 * g + 2] += ba.z; acc[0][rf][4 * g + 3] += ba.w;
          acc[1][rf][4 * g] += bg.x; acc[1][rf][4 * g + 1] += bg.y; acc[1][rf][4 * g + 2] += bg.z; acc[1][rf][4 * g + 3] += bg.w;
        }
      }
    }
#pragma unroll
    for (int rf = 0; rf < 2; ++rf) {
      const int r = rf * 32 + l31, t = t0 + r;
      const float kp = t < len ? 1.f : 0.f;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c0 = 32 * wave + 8 * g + 4 * lh;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = wn_tanh(acc[0][rf][4 * g + e]) * wn_sigmoid(acc[1][rf][4 * g + e]) * kp;
        const unsigned h01 = dv_cvt_pk_bf16(v[0], v[1]), h23 = dv_cvt_pk_bf16(v[2], v[3]);
        const unsigned l01 = dv_cvt_pk_bf16(v[0] - __uint_as_float(h01 << 16), v[1] - __uint_as_float(h01 & 0xffff0000u));
        const unsigned l23 = dv_cvt_pk_bf16(v[2] - __uint_as_float(h23 << 16), v[3] - __uint_as_float(h23 & 0xffff0000u));
        *reinterpret_cast<uint2*>(gs + r * G::RS + c0 * 2) = make_uint2(h01, h23);
        *reinterpret_cast<uint2*>(gs + G::A_PL + r * G::RS + c0 * 2) = make_uint2(l01, l23);
        if (p.acts_out && t < p.T) *reinterpret_cast<float4*>(p.acts_out + (mb + t) * H + c0) = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
  }
  __syncthreads();

  // ---- 5. the 1x1: output fragment `wave` (residual half; last layer: the only one) and H / 32 + wave (skip half) ----
  const int nf2 = p.last ? 1 : 2;                      // (uniform over the launch)
#pragma unroll
  for (int cf = 0; cf < 2; ++cf)
#pragma unroll
    for (int rf = 0; rf < 2; ++rf)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[cf][rf][r] = 0.f;
  {
    const int rbase = l31 * G::RS + lh * 16;
#pragma unroll 2
    for (int ks = 0; ks < G::KS2; ++ks) {
      bf16x8 ah[2], al[2];
#pragma unroll
      for (int rf = 0; rf < 2; ++rf) {
        const int off = rbase + rf * 32 * G::RS + ks * 32;
        ah[rf] = *reinterpret_cast<const bf16x8*>(gs + off);
        al[rf] = *reinterpret_cast<const bf16x8*>(gs + G::A_PL + off);
      }
#pragma unroll
      for (int cf = 0; cf < 2; ++cf) {
        if (cf < nf2) {
          const size_t wo = (((size_t)(cf * (H / 32) + wave) * G::KS2 + ks) * 64 + lane) * 8;
          const bf16x8 fh = *reinterpret_cast<const bf16x8*>(p.w2_hi + wo), fl = *reinterpret_cast<const bf16x8*>(p.w2_lo + wo);
#pragma unroll
          for (int rf = 0; rf < 2; ++rf) {
            acc[cf][rf] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh, al[rf], acc[cf][rf], 0, 0, 0);
            acc[cf][rf] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fl, ah[rf], acc[cf][rf], 0, 0, 0);
            acc[cf][rf] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh, ah[rf], acc[cf][rf], 0, 0, 0);
          }
        }
      }
    }
  }

  // ---- 6. residual stream to the other buffer, skip sum in place; rows beyond T belong to nobody ----
  const int cs_ = p.last ? 0 : 1;                      // accumulator that carries the skip columns
#pragma unroll
  for (int rf = 0; rf < 2; ++rf) {
    const int t = t0 + rf * 32 + l31;
    if (t >= p.T) continue;                            // (both lanes of a pair share the row: store_planes16 sees whole pairs)
    const float kp = t < len ? 1.f : 0.f;
    const size_t o = (mb + t) * H + 32 * wave;
    float vx[16], vs[16];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int cc = 8 * g + 4 * lh;
      const float4 bs = *reinterpret_cast<const float4*>(p.b2 + (p.last ? 0 : H) + 32 * wave + cc);
      float4 sk = make_float4(0.f, 0.f, 0.f, 0.f);
      if (!p.first) sk = *reinterpret_cast<const float4*>(p.skip_in + o + cc);
      vs[4 * g] = sk.x + (acc[cs_][rf][4 * g] + bs.x) * kp; vs[4 * g + 1] = sk.y + (acc[cs_][rf][4 * g + 1] + bs.y) * kp;
      vs[4 * g + 2] = sk.z + (acc[cs_][rf][4 * g + 2] + bs.z) * kp; vs[4 * g + 3] = sk.w + (acc[cs_][rf][4 * g + 3] + bs.w) * kp;
      dv_st16(p.skip_out + o + cc, make_float4(vs[4 * g], vs[4 * g + 1], vs[4 * g + 2], vs[4 * g + 3]));
      if (!p.last) {
        const float4 bx = *reinterpret_cast<const float4*>(p.b2 + 32 * wave + cc);
        const float4 xi = *reinterpret_cast<const float4*>(p.x_in + o + cc);
        vx[4 * g] = (xi.x + (acc[0][rf][4 * g] + bx.x)) * kp; vx[4 * g + 1] = (xi.y + (acc[0][rf][4 * g + 1] + bx.y)) * kp;
        vx[4 * g + 2] = (xi.z + (acc[0][rf][4 * g + 2] + bx.z)) * kp; vx[4 * g + 3] = (xi.w + (acc[0][rf][4 * g + 3] + bx.w)) * kp;
        dv_st16(p.x_out + o + cc, make_float4(vx[4 * g], vx[4 * g + 1], vx[4 * g + 2], vx[4 * g + 3]));
      }
    }
    if (!p.last) store_planes16(p.xh_out, p.xl_out, o, lh, vx);
    else store_planes16(p.sh_out, p.sl_out, o, lh, vs);
  }
}

// Channels-first mel y [B, Cin, T] -> channels-last split planes [B * T, Kp] (channels [Cin, Kp) zeros) through 32 x 32 LDS
// tiles, and keep[m] = t < lengths[b].  Blocks [n_pack, gridDim.x) are the conditioning 1x1 (one wave per output column n,
// exact fp32 FMA dots, fixed-order wave sum - the scheme of k_small_linear): cond[b, n] = sum_k g[b, k] Wc[n, k] + bc[n].
__global__ __launch_bounds__(256) void k_wn_pack(const float* __restrict__ y, const int64_t* __restrict__ lengths, bf16_t* __restrict__ hi,
                                                  bf16_t* __restrict__ lo, float* __restrict__ keep, int B, int Cin, int T, int Kp, int n_pack,
                                                  const float* __restrict__ g, const float* __restrict__ Wc, const float* __restrict__ bc,
                                                  float* __restrict__ cond, int gin, int Nc) {
  __shared__ float tile[32][33];
  if ((int)blockIdx.x < n_pack) {
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int nct = Kp / 32, ntt = (T + 31) / 32;
    int bid = blockIdx.x;
    const int b = bid / (nct * ntt); bid -= b * nct * ntt;
    const int ct = bid / ntt, t0 = (bid - ct * ntt) * 32, c0 = ct * 32;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = c0 + ty + 8 * i, t = t0 + tx;
      tile[ty + 8 * i][tx] = (c < Cin && t < T) ? y[((size_t)b * Cin + c) * T + t] : 0.f;
    }
    __syncthreads();
    const int len = wn_len(lengths, b, T);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int t = t0 + ty + 8 * i, c = c0 + tx;
      if (t >= T) continue;
      const float v = tile[tx][ty + 8 * i];
      const unsigned h = dv_cvt_pk_bf16(v, 0.f) & 0xffffu;
      const unsigned l = dv_cvt_pk_bf16(v - __uint_as_float(h << 16), 0.f) & 0xffffu;
      const size_t o = ((size_t)b * T + t) * Kp + c;
      hi[o] = (bf16_t)h; lo[o] = (bf16_t)l;
      if (ct == 0 && tx == 0) keep[(size_t)b * T + t] = t < len ? 1.f : 0.f;
    }
    return;
  }
  const int lane = threadIdx.x & 63, n = ((int)blockIdx.x - n_pack) * 4 + (threadIdx.x >> 6);
  if (n >= Nc) return;
  const float* w = Wc + (size_t)n * gin;
  for (int b = 0; b < B; ++b) {
    float a = 0.f;
    for (int k = lane; k < gin; k += 64) a = fmaf(g[(size_t)b * gin + k], w[k], a);
    a = wave_sum64(a);
    if (lane == 0) cond[(size_t)b * Nc + n] = a + bc[n];
  }
}

// proj's statistics rows z [B * T, 2C] (m | logs, padding rows zero) -> the reference's channels-first outputs through 32 x 32
// LDS tiles: m, logs and the draw zo = (m + noise * expf(logs)) * keep, all [B, C, T]
__global__ __launch_bounds__(256) void k_wn_store(const float* __restrict__ z, const float* __restrict__ noise, const int64_t* __restrict__ lengths,
                                                   float* __restrict__ zo, float* __restrict__ m_out, float* __restrict__ logs_out, int T, int C) {
  __shared__ float tm[32][33], tl[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int t0 = blockIdx.x * 32, c0 = blockIdx.y * 32, b = blockIdx.z;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int t = t0 + ty + 8 * i, c = c0 + tx;
    float a = 0.f, s = 0.f;
    if (t < T && c < C) {
      const size_t o = ((size_t)b * T + t) * (2 * C) + c;
      a = z[o]; s = z[o + C];
    }
    tm[ty + 8 * i][tx] = a; tl[ty + 8 * i][tx] = s;
  }
  __syncthreads();
  const int len = wn_len(lengths, b, T);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = c0 + ty + 8 * i, t = t0 + tx;
    if (t >= T || c >= C) continue;
    const float a = tm[tx][ty + 8 * i], s = tl[tx][ty + 8 * i];
    const size_t o = ((size_t)b * C + c) * T + t;
    m_out[o] = a; logs_out[o] = s;
    zo[o] = t < len ? a + noise[o] * expf(s) : 0.f;
  }
}

// weight norm folded at pack time: w[n, :] = v[n, :] * (g[n] / ||v[n, :]||), the norm over everything but the output channel, fp32
__global__ __launch_bounds__(256) void k_wn_fold(const float* __restrict__ v, const float* __restrict__ g, float* __restrict__ w, int per_row) {
  __shared__ float part[4];
  const int n = blockIdx.x, tid = threadIdx.x;
  const float* r = v + (size_t)n * per_row;
  float a = 0.f;
  for (int i = tid; i < per_row; i += 256) a = fmaf(r[i], r[i], a);
  a = wave_sum64(a);
  if ((tid & 63) == 0) part[tid >> 6] = a;
  __syncthreads();
  const float s = g[n] / sqrtf((part[0] + part[1]) + (part[2] + part[3]));
  for (int i = tid; i < per_row; i += 256) w[(size_t)n * per_row + i] = r[i] * s;
}

}  // namespace

bool wn_layer_supported(int H) { return H == 256; }

hipError_t wn_init() {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(k_wn_layer<256>), hipFuncAttributeMaxDynamicSharedMemorySize, WnGeom<256>::SMEM);
}

hipError_t launch_wn_layer(const WnLayerParams& p, int H, hipStream_t st) {
  if (H != 256 || p.B < 1 || p.T < 1 || p.tiles_per_utt != (p.T + WN_BM - 1) / WN_BM) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_wn_layer<256>, dim3((unsigned)(p.B * p.tiles_per_utt)), dim3(WN_NT), WnGeom<256>::SMEM, st, p);
  return hipGetLastError();
}

hipError_t launch_wn_pack(const float* y, const int64_t* lengths, bf16_t* hi, bf16_t* lo, float* keep, int B, int Cin, int T, int Kp,
                          const float* g, const float* Wc, const float* bc, float* cond, int gin, int Nc, hipStream_t st) {
  const int n_pack = B * (Kp / 32) * ((T + 31) / 32), n_cond = g ? (Nc + 3) / 4 : 0;
  hipLaunchKernelGGL(k_wn_pack, dim3((unsigned)(n_pack + n_cond)), dim3(256), 0, st, y, lengths, hi, lo, keep, B, Cin, T, Kp, n_pack, g, Wc, bc,
                     cond, gin, Nc);
  return hipGetLastError();
}

hipError_t launch_wn_store(const float* z, const float* noise, const int64_t* lengths, float* zo, float* m_out, float* logs_out, int B, int T,
                           int C, hipStream_t st) {
  hipLaunchKernelGGL(k_wn_store, dim3((T + 31) / 32, (C + 31) / 32, B), dim3(256), 0, st, z, noise, lengths, zo, m_out, logs_out, T, C);
  return hipGetLastError();
}

hipError_t launch_wn_fold(const float* v, const float* g, float* w, int N, int per_row, hipStream_t st) {
  hipLaunchKernelGGL(k_wn_fold, dim3(N), dim3(256), 0, st, v, g, w, per_row);
  return hipGetLastError();
}
