// Text encoder `enc_p` behind the C ABI (dv_tenc_*, include/dvits_hip.h): TextEncoder over the relative-position Encoder
// (reference model3.py:322-381, attentions.py:37-88, 142-300, 322-380; restated in oracle/text_enc_ref.py).
//
// An engine of its own beside the prompt encoder's: dv_tenc_prepare() turns (config, state dict, B, T) into a static list of
// kernel launches over channels-last rows m = b * T + t (the unpadded row space of the prompt encoder; a k = 3 tap of an
// utterance's first / last token reads the GEMM's zero page, as the prompt encoder's nine-tap feed-forward does).  Every
// dependency is a kernel boundary - nothing here waits inside a launch.  Per forward:
//   k_tenc_embed                      three embedding gathers, summed, x sqrt(H), row mask -> fp32 + split planes, keep mask
//   [k_small_linear + k_tenc_add_rows at layer cond_layer_idx: x <- (x + spk_emb_linear(g)) * mask]
//   per layer: k_gemm q|k|v (N = 3H, d^-1/2 folded into the packed q rows) -> k_rel_attention -> k_gemm conv_o + residual ->
//              k_ln_affine -> k_gemm conv_1 (k taps, ReLU, row mask, planes) -> k_gemm conv_2 (k taps) + residual -> k_ln_affine
//   k_gemm proj (N = 2C, row mask) -> k_tenc_store_nct: x * mask, m, logs channels-first
// Padding rows are kept at zero after every step (the reference lets them drift and masks them where they are read: keys, the
// feed-forward's input, the outputs - no valid row ever depends on one).
#include "engine_core.h"

#include <cmath>

namespace {

// (not misc_body.h's split4: this one rounds with integer arithmetic, that one with the packed hardware convert - they may differ on NaN)
__device__ __forceinline__ void tenc_split4(const float4 v, uint2& h, uint2& l) {
  auto rne = [](float f) { unsigned u = __float_as_uint(f); u += 0x7fffu + ((u >> 16) & 1u); return u >> 16; };
  const unsigned h0 = rne(v.x), h1 = rne(v.y), h2 = rne(v.z), h3 = rne(v.w);
  h.x = h0 | (h1 << 16); h.y = h2 | (h3 << 16);
  const unsigned l0 = rne(v.x - __uint_as_float(h0 << 16)), l1 = rne(v.y - __uint_as_float(h1 << 16));
  const unsigned l2 = rne(v.z - __uint_as_float(h2 << 16)), l3 = rne(v.w - __uint_as_float(h3 << 16));
  l.x = l0 | (l1 << 16); l.y = l2 | (l3 << 16);
}

// One wave per token row m = (b, t): x = (emb[id] + tone_emb[tone] + language_emb[lang]) * sqrt(H) * keep, keep = t < lengths[b].
// Indices are clamped into their tables (the host mirror refuses out-of-range ones; nothing is read out of bounds here).
__global__ __launch_bounds__(256) void k_tenc_embed(const int64_t* __restrict__ ids, const int64_t* __restrict__ tone,
                                                     const int64_t* __restrict__ lang, const int64_t* __restrict__ lengths,
                                                     const float* __restrict__ e_id, const float* __restrict__ e_tone,
                                                     const float* __restrict__ e_lang, int n_id, int n_tone, int n_lang,
                                                     float* __restrict__ x, bf16_t* __restrict__ hi, bf16_t* __restrict__ lo,
                                                     float* __restrict__ keep, int B, int T, int H, float scale) {
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (m >= B * T) return;
  const int b = m / T, t = m - b * T;
  const long long len = lengths[b];
  const float kp = (long long)t < len ? 1.f : 0.f;
  auto clampi = [](long long v, int n) { return (int)(v < 0 ? 0 : (v >= n ? n - 1 : v)); };
  const float* r0 = e_id + (size_t)clampi(ids[m], n_id) * H;
  const float* r1 = e_tone + (size_t)clampi(tone[m], n_tone) * H;
  const float* r2 = e_lang + (size_t)clampi(lang[m], n_lang) * H;
  if (lane == 0) keep[m] = kp;
  for (int c = lane * 4; c < H; c += 256) {
    const float4 a = *reinterpret_cast<const float4*>(r0 + c), d = *reinterpret_cast<const float4*>(r1 + c),
                 e = *reinterpret_cast<const float4*>(r2 + c);
    float4 v;
    v.x = ((a.x + d.x) + e.x) * scale * kp; v.y = ((a.y + d.y) + e.y) * scale * kp;
    v.z = ((a.z + d.z) + e.z) * scale * kp; v.w = ((a.w + d.w) + e.w) * scale * kp;
    const size_t o = (size_t)m * H + c;
    *reinterpret_cast<float4*>(x + o) = v;
    uint2 h2, l2;
    tenc_split4(v, h2, l2);
    *reinterpret_cast<uint2*>(hi + o) = h2;
    *reinterpret_cast<uint2*>(lo + o) = l2;
  }
}

// y[m, :] = (x[m, :] + add[b, :]) * keep[m] (fp32 + split planes; y may be x: every element is read and written by one
// thread): the speaker conditioning of layer cond_layer_idx.  add == null: y = x * keep.
__global__ __launch_bounds__(256) void k_tenc_add_rows(const float* x, float* y, bf16_t* hi, bf16_t* lo, const float* __restrict__ add,
                                                        const float* __restrict__ keep, int B, int T, int H) {
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (m >= B * T) return;
  const int b = m / T;
  const float kp = keep[m];
  for (int c = lane * 4; c < H; c += 256) {
    const size_t o = (size_t)m * H + c;
    const float4 a = *reinterpret_cast<const float4*>(x + o);
    const float4 g = add ? *reinterpret_cast<const float4*>(add + (size_t)b * H + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 v;
    v.x = (a.x + g.x) * kp; v.y = (a.y + g.y) * kp; v.z = (a.z + g.z) * kp; v.w = (a.w + g.w) * kp;
    *reinterpret_cast<float4*>(y + o) = v;
    uint2 h2, l2;
    tenc_split4(v, h2, l2);
    *reinterpret_cast<uint2*>(hi + o) = h2;
    *reinterpret_cast<uint2*>(lo + o) = l2;
  }
}

// channels-last rows -> the reference's channels-first outputs, 32 x 32 tiles through LDS: virtual channel cc < H is
// x[m, cc] -> x_out [B, H, T]; H <= cc < H + C is z[m, cc - H] -> m_out [B, C, T]; the rest z[m, cc - H] -> logs_out [B, C, T]
__global__ __launch_bounds__(256) void k_tenc_store_nct(const float* __restrict__ x, const float* __restrict__ z,
                                                         float* __restrict__ x_out, float* __restrict__ m_out,
                                                         float* __restrict__ logs_out, int T, int H, int C) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int t0 = blockIdx.x * 32, c0 = blockIdx.y * 32, b = blockIdx.z, Ct = H + 2 * C;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int t = t0 + ty + 8 * i, cc = c0 + tx;
    float v = 0.f;
    if (t < T && cc < Ct) {
      const size_t m = (size_t)b * T + t;
      v = cc < H ? x[m * H + cc] : z[m * (2 * C) + (cc - H)];
    }
    tile[ty + 8 * i][tx] = v;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int cc = c0 + ty + 8 * i, t = t0 + tx;
    if (t < T && cc < Ct) {
      const float v = tile[tx][ty + 8 * i];
      if (cc < H) x_out[((size_t)b * H + cc) * T + t] = v;
      else if (cc < H + C) m_out[((size_t)b * C + (cc - H)) * T + t] = v;
      else logs_out[((size_t)b * C + (cc - H - C)) * T + t] = v;
    }
  }
}

__global__ void k_tenc_scale(const float* __restrict__ in, float* __restrict__ out, float s, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = in[i] * s;
}

}  // namespace

struct dv_tenc : RowEngine {
  dv_tenc_cfg cfg{};
  std::map<std::string, void*> bufs;         // (in `owned`)
  float* qscale_vec = nullptr;               // (in `owned_w`)
  struct { const int64_t* ids = nullptr; const int64_t* tone = nullptr; const int64_t* lang = nullptr; const int64_t* lengths = nullptr;
           const float* g = nullptr; float* x = nullptr; float* m = nullptr; float* logs = nullptr; } io;
};

namespace {

void tenc_release_prepared(dv_tenc* t, bool keep_packed) {
  t->release_prepared();
  t->bufs.clear();
  if (!keep_packed) { t->release_packed(); t->qscale_vec = nullptr; }
}

// The planner of one prepare: packs the weights (once per weight set), sizes the buffers, emits the launches.
struct TPlan : RowPlan {
  dv_tenc* t;
  int H, F, C, nh, d, ks, win, L;

  // activation buffers: one set shared by all layers, or (DVITS_KEEP_INTERMEDIATES=1) one per layer so that probes stay valid
  template <typename X> X* buf(const std::string& name, int layer, size_t elems) {
    const std::string key = t->keep ? name + "." + std::to_string(layer) : name;
    auto it = t->bufs.find(key);
    if (it != t->bufs.end()) return reinterpret_cast<X*>(it->second);
    X* p = dmalloc<X>(elems, t->owned, false);
    t->bufs[key] = p;
    return p;
  }
  struct Piece { std::string w; int N, kind, Cw, taps, n_off; const float* kscale; };
  struct BiasPiece { const float* p; int N, n_off; };
  const PackedW3* pack(const std::string& key, int N, int Kp, const std::vector<Piece>& pieces, const std::vector<BiasPiece>& biases) {
    auto it = t->packed.find(key);
    if (it != t->packed.end()) return &it->second;
    PackedW3 pw;
    pw.N = N; pw.Kp = Kp; pw.N_pad = rup(N, 128);
    const size_t elems = (size_t)pw.N_pad * Kp;
    pw.hi = dmalloc<bf16_t>(elems, t->owned_w, true);
    pw.lo = dmalloc<bf16_t>(elems, t->owned_w, true);
    pw.bias = dmalloc<float>((size_t)pw.N_pad, t->owned_w, true);
    if (!pw.hi || !pw.lo || !pw.bias) return nullptr;
    for (const Piece& pc : pieces) {
      const RawW* r = raw(pc.w, (size_t)pc.N * pc.Cw * pc.taps);
      if (!r) return nullptr;
      PackSpec s{};
      s.src = r->p; s.N = pc.N; s.kind = pc.kind; s.C = pc.Cw; s.taps = pc.taps; s.c_pad = pc.Cw; s.k_off = 0; s.n_off = pc.n_off;
      s.kscale = pc.kscale; s.geglu = 0;
      if (launch_pack_weight(s, pw.hi, pw.lo, Kp, st) != hipSuccess) { err.set(DV_ERR_HIP, "pack_weight launch failed"); return nullptr; }
    }
    for (const BiasPiece& bp : biases) {
      if (!bp.p) return nullptr;
      if (hipMemcpyAsync(pw.bias + bp.n_off, bp.p, (size_t)bp.N * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) { err.set(DV_ERR_HIP, "bias copy failed"); return nullptr; }
    }
    t->packed[key] = pw;
    return &t->packed[key];
  }

  int build() {
    dv_tenc* tt = t;
    const dv_tenc_cfg& c = t->cfg;
    const int Bn = B, Tn = T, Hn = H;
    if (!zero_page()) return err.fail();
    if (!t->qscale_vec) {
      t->qscale_vec = dmalloc<float>((size_t)H, t->owned_w, false);
      if (!t->qscale_vec) return err.fail();
      (void)launch_fill_f32(t->qscale_vec, 1.0f / sqrtf((float)d), H, st);
    }
    const float* e_id = W("emb.weight", (size_t)c.n_vocab * H);
    const float* e_tone = W("tone_emb.weight", (size_t)c.n_tones * H);
    const float* e_lang = W("language_emb.weight", (size_t)c.n_languages * H);
    if (!e_id || !e_tone || !e_lang) return err.fail();

    float* keep = buf<float>("keep", 0, (size_t)M);
    float* x = buf<float>("x", -1, (size_t)M * H);
    bf16_t* x_hi = buf<bf16_t>("x_hi", -1, (size_t)M * H);
    bf16_t* x_lo = buf<bf16_t>("x_lo", -1, (size_t)M * H);
    if (!keep || !x || !x_hi || !x_lo) return err.fail();
    {
      const int nv = c.n_vocab, ntn = c.n_tones, nl = c.n_languages;
      const float sc = sqrtf((float)H);
      t->ops.push_back([=](hipStream_t s) {
        hipLaunchKernelGGL(k_tenc_embed, dim3((Bn * Tn + 3) / 4), dim3(256), 0, s, tt->io.ids, tt->io.tone, tt->io.lang, tt->io.lengths,
                           e_id, e_tone, e_lang, nv, ntn, nl, x, x_hi, x_lo, keep, Bn, Tn, Hn, sc);
        return hipGetLastError();
      });
    }
    probe("emb", x, H);

    float* gl = nullptr;
    const float* w_spk = nullptr; const float* b_spk = nullptr;
    if (c.gin_channels > 0) {
      w_spk = W("encoder.spk_emb_linear.weight", (size_t)H * c.gin_channels);
      b_spk = W("encoder.spk_emb_linear.bias", (size_t)H);
      gl = buf<float>("gl", 0, (size_t)B * H);
      if (!w_spk || !b_spk || !gl) return err.fail();
    }

    for (int i = 0; i < L; ++i) {
      const std::string li = std::to_string(i);
      const std::string pa = "encoder.attn_layers." + li + ".", pf = "encoder.ffn_layers." + li + ".";
      const std::string n1 = "encoder.norm_layers_1." + li + ".", n2 = "encoder.norm_layers_2." + li + ".";
      // d^-1/2 rides on the packed q rows (a constant per-source-channel factor) and on the q bias
      float* bq = nullptr;
      if (!t->packed.count(pa + "qkv")) {
        const float* bq_raw = W(pa + "conv_q.bias", (size_t)H);
        bq = dmalloc<float>((size_t)H, t->owned_w, false);
        if (!bq_raw || !bq) return err.fail();
        hipLaunchKernelGGL(k_tenc_scale, dim3((H + 255) / 256), dim3(256), 0, st, bq_raw, bq, 1.0f / sqrtf((float)d), H);
      }
      const PackedW3* w_qkv = pack(pa + "qkv", 3 * H, H,
                                  {{pa + "conv_q.weight", H, 0, H, 1, 0, t->qscale_vec}, {pa + "conv_k.weight", H, 0, H, 1, H, nullptr},
                                   {pa + "conv_v.weight", H, 0, H, 1, 2 * H, nullptr}},
                                  {{bq, H, 0}, {W(pa + "conv_k.bias", (size_t)H), H, H}, {W(pa + "conv_v.bias", (size_t)H), H, 2 * H}});
      const PackedW3* w_o = pack(pa + "o", H, H, {{pa + "conv_o.weight", H, 0, H, 1, 0, nullptr}}, {{W(pa + "conv_o.bias", (size_t)H), H, 0}});
      const PackedW3* w_f1 = pack(pf + "c1", F, ks * H, {{pf + "conv_1.weight", F, 1, H, ks, 0, nullptr}}, {{W(pf + "conv_1.bias", (size_t)F), F, 0}});
      const PackedW3* w_f2 = pack(pf + "c2", H, ks * F, {{pf + "conv_2.weight", H, 1, F, ks, 0, nullptr}}, {{W(pf + "conv_2.bias", (size_t)H), H, 0}});
      const float* ek = W(pa + "emb_rel_k", (size_t)(2 * win + 1) * d);
      const float* ev = W(pa + "emb_rel_v", (size_t)(2 * win + 1) * d);
      const float* g1 = W(n1 + "gamma", (size_t)H); const float* b1 = W(n1 + "beta", (size_t)H);
      const float* g2 = W(n2 + "gamma", (size_t)H); const float* b2 = W(n2 + "beta", (size_t)H);
      if (!w_qkv || !w_o || !w_f1 || !w_f2 || !ek || !ev || !g1 || !b1 || !g2 || !b2)
        return err.fail();

      // the layer's input: x (fp32: conv_o's residual) and its split planes (the q|k|v operand)
      if (i == c.cond_layer_idx && c.gin_channels > 0) {
        const int gin = c.gin_channels;
        t->ops.push_back([=](hipStream_t s) {
          if (!tt->io.g) return hipSuccess;            // (no speaker vector in this call)
          return launch_small_linear(tt->io.g, gin, w_spk, b_spk, nullptr, gl, Hn, Bn, gin, Hn, 0, 0, s);
        });
        t->flops += 2.0 * B * (double)gin * H;
        // in place, or (probes kept) into buffers of its own so that the previous layer's probe stays what it was; without
        // a speaker vector the in-place form has nothing to do
        const float* xin = x;
        float* xc = t->keep ? buf<float>("xc", i, (size_t)M * H) : x;
        bf16_t* xh = t->keep ? buf<bf16_t>("xc_hi", i, (size_t)M * H) : x_hi;
        bf16_t* xl = t->keep ? buf<bf16_t>("xc_lo", i, (size_t)M * H) : x_lo;
        if (!xc || !xh || !xl) return err.fail();
        t->ops.push_back([=](hipStream_t s) {
          if (!tt->io.g && xin == xc) return hipSuccess;
          hipLaunchKernelGGL(k_tenc_add_rows, dim3((Bn * Tn + 3) / 4), dim3(256), 0, s, xin, xc, xh, xl, tt->io.g ? gl : (const float*)nullptr,
                             keep, Bn, Tn, Hn);
          return hipGetLastError();
        });
        x = xc; x_hi = xh; x_lo = xl;
      }
      float* qkv = buf<float>("qkv", i, (size_t)M * 3 * H);
      bf16_t* ao_hi = buf<bf16_t>("ao_hi", i, (size_t)M * H); bf16_t* ao_lo = buf<bf16_t>("ao_lo", i, (size_t)M * H);
      float* x1 = buf<float>("x1", i, (size_t)M * H);
      float* y1 = buf<float>("y1", i, (size_t)M * H);
      bf16_t* y1_hi = buf<bf16_t>("y1_hi", i, (size_t)M * H); bf16_t* y1_lo = buf<bf16_t>("y1_lo", i, (size_t)M * H);
      bf16_t* hh_hi = buf<bf16_t>("hh_hi", i, (size_t)M * F); bf16_t* hh_lo = buf<bf16_t>("hh_lo", i, (size_t)M * F);
      float* x2 = buf<float>("x2", i, (size_t)M * H);
      float* xn = buf<float>("x", i, (size_t)M * H);
      bf16_t* xn_hi = buf<bf16_t>("x_hi", i, (size_t)M * H); bf16_t* xn_lo = buf<bf16_t>("x_lo", i, (size_t)M * H);
      if (!qkv || !ao_hi || !ao_lo || !x1 || !y1 || !y1_hi || !y1_lo || !hh_hi || !hh_lo || !x2 || !xn || !xn_hi || !xn_lo)
        return err.fail();

      { GemmParams g = gp(3 * H); g.seg[0] = seg1(x_hi, x_lo, H, 1, 0); g.out = qkv; gemm(g, w_qkv, H); }
      {
        RelAttnParams a{};
        a.q = qkv; a.k = qkv + H; a.v = qkv + 2 * H; a.ldq = a.ldk = a.ldv = 3 * H;
        a.emb_k = ek; a.emb_v = ev; a.o = nullptr; a.o_hi = ao_hi; a.o_lo = ao_lo; a.ldo = H;
        a.B = B; a.H = nh; a.T = T; a.d = d; a.window = win; a.scale = 1.0f;
        t->ops.push_back([a, tt](hipStream_t s) { RelAttnParams a2 = a; a2.lengths = tt->io.lengths; return launch_rel_attention(a2, s); });
        t->flops += 4.0 * B * nh * (double)T * T * d;
      }
      { GemmParams g = gp(H); g.seg[0] = seg1(ao_hi, ao_lo, H, 1, 0); g.epi = EPI_RESIDUAL; g.res = x; g.out = x1; g.rowmask = keep; gemm(g, w_o, H); }
      probe("layer" + li + ".attn", x1, H);
      t->ops.push_back([=](hipStream_t s) { return launch_ln_affine(x1, g1, b1, keep, y1, y1_hi, y1_lo, Bn * Tn, Hn, 1e-5f, s); });
      probe("layer" + li + ".ln1", y1, H);
      { GemmParams g = gp(F); g.seg[0] = seg1(y1_hi, y1_lo, H, ks, (ks - 1) / 2); g.relu = 1; g.rowmask = keep; g.out_hi = hh_hi; g.out_lo = hh_lo; gemm(g, w_f1, ks * H); }
      if (t->keep) t->probes.push_back(RowProbe{"layer" + li + ".ffn1", nullptr, hh_hi, hh_lo, F});
      { GemmParams g = gp(H); g.seg[0] = seg1(hh_hi, hh_lo, F, ks, (ks - 1) / 2); g.epi = EPI_RESIDUAL; g.res = y1; g.out = x2; g.rowmask = keep; gemm(g, w_f2, ks * F); }
      t->ops.push_back([=](hipStream_t s) { return launch_ln_affine(x2, g2, b2, keep, xn, xn_hi, xn_lo, Bn * Tn, Hn, 1e-5f, s); });
      probe("layer" + li, xn, H);
      x = xn; x_hi = xn_hi; x_lo = xn_lo;
    }

    const PackedW3* w_p = pack("proj", 2 * C, H, {{"proj.weight", 2 * C, 0, H, 1, 0, nullptr}}, {{W("proj.bias", (size_t)2 * C), 2 * C, 0}});
    float* z = buf<float>("z", 0, (size_t)M * 2 * C);
    if (!w_p || !z) return err.fail();
    { GemmParams g = gp(2 * C); g.seg[0] = seg1(x_hi, x_lo, H, 1, 0); g.out = z; g.rowmask = keep; gemm(g, w_p, H); }
    probe("proj", z, 2 * C);
    {
      const float* xf = x;
      const int Cn = C;
      t->ops.push_back([=](hipStream_t s) {
        hipLaunchKernelGGL(k_tenc_store_nct, dim3((Tn + 31) / 32, (Hn + 2 * Cn + 31) / 32, Bn), dim3(256), 0, s, xf, z, tt->io.x, tt->io.m,
                           tt->io.logs, Tn, Hn, Cn);
        return hipGetLastError();
      });
    }
    if (err) return err.fail();
    return DV_OK;
  }
};

}  // namespace

extern "C" int dv_tenc_create(const dv_tenc_cfg* cfg, dv_tenc** out) {
  if (!cfg || !out) return dv_fail(DV_ERR_INVALID, "dv_tenc_create: null argument");
  if (cfg->n_vocab <= 0 || cfg->n_tones <= 0 || cfg->n_languages <= 0) return dv_fail(DV_ERR_INVALID, "vocabulary sizes must be positive");
  if (cfg->hidden_channels <= 0 || cfg->hidden_channels % 32 != 0 || cfg->hidden_channels > 2048)
    return dv_fail(DV_ERR_INVALID, "hidden_channels must be a positive multiple of 32, <= 2048");
  if (cfg->filter_channels <= 0 || cfg->filter_channels % 32 != 0 || cfg->filter_channels > 8192)
    return dv_fail(DV_ERR_INVALID, "filter_channels must be a positive multiple of 32, <= 8192");
  if (cfg->out_channels <= 0 || cfg->out_channels % 2 != 0) return dv_fail(DV_ERR_INVALID, "out_channels must be positive and even");
  if (cfg->n_heads <= 0 || cfg->hidden_channels % cfg->n_heads != 0) return dv_fail(DV_ERR_INVALID, "n_heads must divide hidden_channels");
  const int d = cfg->hidden_channels / cfg->n_heads;
  if (d != 32 && d != 64 && d != 128) return dv_fail(DV_ERR_INVALID, "head dim %d: k_rel_attention is built for 32, 64 and 128", d);
  if (cfg->n_layers < 1 || cfg->n_layers > 64) return dv_fail(DV_ERR_INVALID, "n_layers out of range");
  if (cfg->kernel_size < 1 || cfg->kernel_size > 9 || cfg->kernel_size % 2 != 1) return dv_fail(DV_ERR_INVALID, "kernel_size must be odd, 1..9");
  if (cfg->window_size < 0 || cfg->window_size > DV_RELATTN_MAX_WINDOW)
    return dv_fail(DV_ERR_INVALID, "window_size must be 0..%d", (int)DV_RELATTN_MAX_WINDOW);
  if (cfg->gin_channels < 0 || cfg->gin_channels > 4096) return dv_fail(DV_ERR_INVALID, "gin_channels out of range");
  if (cfg->gin_channels > 0 && (cfg->cond_layer_idx < 0 || cfg->cond_layer_idx >= cfg->n_layers))
    return dv_fail(DV_ERR_INVALID, "cond_layer_idx must be less than n_layers");
  dv_tenc* t = new dv_tenc();
  t->cfg = *cfg;
  *out = t;
  return DV_OK;
}

extern "C" void dv_tenc_destroy(dv_tenc* t) {
  if (!t) return;
  (void)hipDeviceSynchronize();
  tenc_release_prepared(t, false);
  t->w.free_all();
  delete t;
}

extern "C" int dv_tenc_set_weight(dv_tenc* t, const char* name, const void* dev_ptr, const int64_t* shape, int32_t ndim) {
  return row_set_weight(t, name, dev_ptr, shape, ndim, "dv_tenc_set_weight");
}

extern "C" int dv_tenc_prepare(dv_tenc* t, int32_t B, int32_t T, int32_t precision) {
  if (!t) return dv_fail(DV_ERR_INVALID, "dv_tenc_prepare: null handle");
  if (B <= 0 || T <= 0) return dv_fail(DV_ERR_INVALID, "dv_tenc_prepare: B, T must be positive");
  if (precision == DV_PREC_BF16)
    return dv_fail(DV_ERR_INVALID, "dv_tenc_prepare: DV_PREC_BF16 is unsupported by the text encoder (split-bf16 DV_PREC_BF16X3 only)");
  if (precision != DV_PREC_BF16X3) return dv_fail(DV_ERR_INVALID, "unknown precision %d", precision);
  if (T > DV_RELATTN_MAX_T) return dv_fail(DV_ERR_INVALID, "dv_tenc_prepare: T = %d exceeds the %d tokens k_rel_attention is tested to", T, (int)DV_RELATTN_MAX_T);
  if (B > 65535) return dv_fail(DV_ERR_INVALID, "dv_tenc_prepare: B = %d exceeds 65535", B);
  if ((size_t)B * (size_t)(t->cfg.gin_channels > 0 ? t->cfg.gin_channels : 1) * sizeof(float) > 64 * 1024)
    return dv_fail(DV_ERR_INVALID, "dv_tenc_prepare: B x gin_channels = %d x %d floats exceed the 64 KiB k_small_linear stages", B, t->cfg.gin_channels);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(gemm_init());
  gemm_env_refresh();
  tenc_release_prepared(t, !t->weights_dirty);
  t->B = B; t->T = T; t->precision = precision;
  const char* keep = getenv("DVITS_KEEP_INTERMEDIATES");
  t->keep = keep && keep[0] == '1';
  TPlan pl{};
  pl.t = t; pl.e = t; pl.B = B; pl.T = T; pl.M = B * T;
  pl.H = t->cfg.hidden_channels; pl.F = t->cfg.filter_channels; pl.C = t->cfg.out_channels; pl.nh = t->cfg.n_heads;
  pl.d = pl.H / pl.nh; pl.ks = t->cfg.kernel_size; pl.win = t->cfg.window_size; pl.L = t->cfg.n_layers;
  int rc = pl.build();
  if (rc != DV_OK) { tenc_release_prepared(t, false); t->weights_dirty = true; return rc; }
  HIPCHK(hipDeviceSynchronize());
  t->prepared = true;
  t->weights_dirty = false;
  return DV_OK;
}

extern "C" int dv_tenc_forward(dv_tenc* t, const int64_t* ids, const int64_t* tone, const int64_t* language, const int64_t* lengths,
                               const float* g, float* x, float* m, float* logs, void* stream) {
  if (!t || !ids || !tone || !language || !lengths || !x || !m || !logs) return dv_fail(DV_ERR_INVALID, "dv_tenc_forward: null argument");
  if (!t->prepared) return dv_fail(DV_ERR_STATE, "dv_tenc_forward before dv_tenc_prepare");
  t->io.ids = ids; t->io.tone = tone; t->io.lang = language; t->io.lengths = lengths; t->io.g = g;
  t->io.x = x; t->io.m = m; t->io.logs = logs;
  return run_ops(t->ops, (hipStream_t)stream, "text encoder");
}

extern "C" int dv_tenc_stats(dv_tenc* t, int64_t* n_launch, double* flops) { return row_stats(t, n_launch, flops, "dv_tenc"); }

extern "C" int dv_tenc_probe(dv_tenc* t, const char* name, float* host_out, int64_t capacity, int64_t* dims) {
  return row_probe(t, name, host_out, capacity, dims, "dv_tenc");
}

extern "C" int dv_op_rel_attention(const float* q, const float* k, const float* v, const float* emb_k, const float* emb_v,
                                   const int64_t* lengths, float* o, int32_t B, int32_t H, int32_t T, int32_t d, int32_t window,
                                   void* stream) {
  if (!q || !k || !v || !emb_k || !emb_v || !lengths || !o) return dv_fail(DV_ERR_INVALID, "dv_op_rel_attention: null argument");
  if (d != 32 && d != 64 && d != 128) return dv_fail(DV_ERR_INVALID, "dv_op_rel_attention: d = %d must be 32, 64 or 128", d);
  if (B <= 0 || B > 65535 || H <= 0 || H > 65535) return dv_fail(DV_ERR_INVALID, "dv_op_rel_attention: B, H must be 1..65535");
  if (T <= 0 || T > DV_RELATTN_MAX_T) return dv_fail(DV_ERR_INVALID, "dv_op_rel_attention: T = %d must be 1..%d (the largest tested length)", T, (int)DV_RELATTN_MAX_T);
  if (window < 0 || window > DV_RELATTN_MAX_WINDOW) return dv_fail(DV_ERR_INVALID, "dv_op_rel_attention: window = %d must be 0..%d", window, (int)DV_RELATTN_MAX_WINDOW);
  RelAttnParams a{};
  a.q = q; a.k = k; a.v = v; a.ldq = a.ldk = a.ldv = a.ldo = H * d;
  a.emb_k = emb_k; a.emb_v = emb_v; a.lengths = lengths; a.o = o;
  a.B = B; a.H = H; a.T = T; a.d = d; a.window = window; a.scale = 1.0f / sqrtf((float)d);
  hipError_t e = launch_rel_attention(a, (hipStream_t)stream);
  if (e != hipSuccess) return dv_fail(DV_ERR_HIP, "dv_op_rel_attention: launch failed: %s (pointers must be 16-byte aligned)", hipGetErrorString(e));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return DV_OK;
}
