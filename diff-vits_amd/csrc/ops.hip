// Single-operator entry points behind the C ABI (dv_op_*, include/dvits_hip.h): one kernel, or the short launch sequence of one
// route of the forward, on the caller's device tensors - what the operator-parity tests call, and model3.py's k = 1 Conv1d.
// Every entry point validates first (a refusal touches no device), then plans its scratch and launches, runs them on the
// caller's stream and waits.  Host code only: no kernel lives here.
#include "engine_core.h"

#include <algorithm>
#include <cmath>

struct Planes {
  bf16_t* hi = nullptr; bf16_t* lo = nullptr;
  Planes at(size_t off) const { return Planes{hi ? hi + off : nullptr, lo ? lo + off : nullptr}; }
};

// Scratch and launch list of one call, planned like a prepare: every buffer is allocated (and zeroed, or handed to DVITS_POISON)
// as it is requested, every launch is only recorded; run() asks ONCE whether an allocation or a fill failed, then enqueues the
// launches in the order they were recorded and waits.  The buffers are freed when the call returns.  UNWRITTEN memory is what
// DVITS_POISON fills and dv_unwritten_bytes() counts; OUTSIDE is neither (profiles/poison_audit.txt).
struct OpScratch {
  enum Fill { UNWRITTEN, ZEROED, OUTSIDE };
  const char* what;
  hipStream_t st;
  bool x3;                        // split planes and packed weights carry a lo plane
  bool failed = false;            // the first allocation or fill that failed
  std::vector<void*> ptrs;
  const bf16_t* zp = nullptr;     // one zero page per call
  std::vector<std::pair<const char*, OpFn>> ops;   // (what the failure message calls it, the launch)
  OpScratch(const char* what_, void* stream, int precision = DV_PREC_BF16X3) : what(what_), st((hipStream_t)stream), x3(precision == DV_PREC_BF16X3) {}
  ~OpScratch() { for (void* p : ptrs) (void)hipFree(p); }

  template <typename T> T* get(size_t bytes, Fill fill = UNWRITTEN) {
    void* p = nullptr;
    if (!bytes) bytes = 16;
    if (hipMalloc(&p, bytes) != hipSuccess) { failed = true; return nullptr; }
    ptrs.push_back(p);
    if (fill == ZEROED) (void)hipMemsetAsync(p, 0, bytes, st);
    else if (fill == UNWRITTEN && poison_fill(p, bytes, st) != hipSuccess) failed = true;   // (DVITS_POISON)
    return reinterpret_cast<T*>(p);
  }
  // the one-time kernel attributes and launch_gemm's environment knobs, as every prepare sets them up
  int start() { HIPCHK(gemm_init()); gemm_env_refresh(); HIPCHK(attn_init()); return DV_OK; }
  void op(const char* stage, OpFn f) { ops.emplace_back(stage, std::move(f)); }
  int run() {
    if (failed) return dv_fail(DV_ERR_HIP, "%s: hipMalloc failed", what);
    for (auto& o : ops) {
      const hipError_t e = o.second(st);
      if (e != hipSuccess) return dv_fail(DV_ERR_HIP, "%s: %slaunch failed: %s", what, o.first, hipGetErrorString(e));
    }
    HIPCHK(hipStreamSynchronize(st));
    return DV_OK;
  }

  // split planes of `elems` values: hi, and lo in bf16x3 mode only
  Planes planes(size_t elems, Fill fill = UNWRITTEN) { return Planes{get<bf16_t>(elems * 2, fill), x3 ? get<bf16_t>(elems * 2, fill) : nullptr}; }
  // ... those of the fp32 tensor `src` (k_split), with `guard` elements of bf16 NaN behind them
  Planes split(const float* src, size_t elems, size_t guard = 0) {
    const Planes p = planes(elems + guard);
    op("k_split ", [=](hipStream_t s) { return launch_split(src, p.hi, p.lo, (int64_t)elems, s); });
    for (bf16_t* q : {p.hi, p.lo})
      if (guard && q) op("guard fill ", [=](hipStream_t s) { return hipMemsetD16Async((hipDeviceptr_t)(q + elems), 0x7fc1, guard, s); });
    return p;
  }
  // zeroed packed weight planes [N rounded up to 128, Kp]; own_bias: a zeroed bias of their own, for fold_bias
  PackedW3 weights(int N, int Kp, bool own_bias = false) {
    PackedW3 w;
    w.N = N; w.N_pad = rup(N, 128); w.Kp = Kp;
    const Planes p = planes((size_t)w.N_pad * Kp, ZEROED);
    w.hi = p.hi; w.lo = p.lo;
    if (own_bias) w.bias = get<float>((size_t)w.N_pad * 4, ZEROED);
    return w;
  }
  // one k-segment of w's planes from packed column k_off on: `src` is linear [N, C] (kind 0) or conv [N, C, taps] (kind 1);
  // kscale folds a LayerNorm gamma in, geglu packs the rows as [32 value | 32 gate] blocks
  void pack(const PackedW3& w, const float* src, int kind, int C, int taps, int c_pad, int k_off = 0, const float* kscale = nullptr, int geglu = 0) {
    PackSpec s{};
    s.src = src; s.N = w.N; s.kind = kind; s.C = C; s.taps = taps; s.c_pad = c_pad; s.k_off = k_off; s.kscale = kscale; s.geglu = geglu;
    op("weight packing ", [=](hipStream_t t) { return launch_pack_weight(s, w.hi, w.lo, w.Kp, t); });
  }
  // w's own bias = bias + W beta (a LayerNorm's beta fold), or (geglu) the bias in the packed [32 value | 32 gate] column order
  void fold_bias(const PackedW3& w, const float* W, const float* bias, const float* beta, int geglu) {
    op("bias fold ", [=](hipStream_t s) { return launch_fold_bias(W, bias, beta, w.bias, w.N, w.Kp, 0, geglu, s); });
  }
  // g against w, the zero page and w's own bias where it has one, else `bias`
  void gemm(GemmParams g, const PackedW3& w, const float* bias, int precision, const char* stage = "") {
    g.w_hi = w.hi; g.w_lo = w.lo; g.Kp = w.Kp; g.N_pad = w.N_pad; g.bias = w.bias ? w.bias : bias;
    g.zero_page = zero_page();
    op(stage, [=](hipStream_t s) { return launch_gemm(g, precision, s); });
  }
  const bf16_t* zero_page() { return zp ? zp : (zp = get<bf16_t>(DV_ZERO_PAGE_BYTES, ZEROED)); }
};

extern "C" int dv_op_conv1d(const float* x, const float* w, const float* bias, float* y, int32_t B, int32_t Cin, int32_t T,
                            int32_t Cout, int32_t k, int32_t stride, int32_t up_T, int32_t precision, void* stream) {
  if (!x || !w || !y || (k != 1 && k != 3) || (stride != 1 && stride != 2)) return dv_fail(DV_ERR_INVALID, "dv_op_conv1d: bad argument");
  const int cpad = rup(Cin, 32);
  if (2 * (size_t)cpad + 256 > DV_ZERO_PAGE_BYTES)
    return dv_fail(DV_ERR_INVALID, "dv_op_conv1d: Cin = %d exceeds the %d channels one source tensor may have", Cin, (DV_ZERO_PAGE_BYTES - 256) / 2);
  OpScratch sc("dv_op_conv1d", stream, precision);
  if (int rc = sc.start()) return rc;
  const Planes a = sc.planes((size_t)B * T * cpad);
  sc.op("k_pack_input ", [=](hipStream_t s) { return launch_pack_input(x, Cin, nullptr, 0, a.hi, a.lo, cpad, B, T, s); });
  const PackedW3 pw = sc.weights(Cout, k * cpad);
  sc.pack(pw, w, 1, Cin, k, cpad);
  GemmParams g{};
  g.seg[0] = seg1(a.hi, a.lo, cpad, k, (k - 1) / 2);
  g.nseg = 1; g.B = B; g.T_in = T;
  g.T_virt = up_T > 0 ? up_T : T;
  g.up_mode = up_T > 0 ? UP_SIZE : UP_NONE;
  g.up_scale = up_T > 0 ? (float)T / (float)up_T : 1.f;
  g.stride = stride;
  g.T_out = (g.T_virt + 2 * g.seg[0].pad - k) / stride + 1;
  g.M = B * g.T_out; g.N = Cout; g.epi = EPI_STORE_NCT; g.out = y; g.ldo = Cout;
  sc.gemm(g, pw, bias, precision);
  return sc.run();
}

// ---- the row GEMMs: y = x W^T + bias through k_gemm, as fp32 [M, ldo] (y) and / or split bf16 planes [M, ldo] (y_hi, y_lo) ----
// The one body of dv_op_linear, dv_op_linear_planes and dv_op_gemm.  g is the validated launch without its operands: the shape,
// the widths c0 | c1 of the source(s) x [M, c0 + c1], the epilogue with its tensors, the outputs and the tile; splitk as
// dv_op_gemm takes it.  GEGLU: W = [value rows | gate rows] (N = 2 x N_out, reference activations GEGLU: hidden * gelu(gate)).
static int row_gemm(const char* what, GemmParams g, const float* x, const float* w, const float* bias, int splitk, int precision, void* stream) {
  OpScratch sc(what, stream, precision);
  if (int rc = sc.start()) return rc;
  const int M = g.M, N = g.N, c0 = g.seg[0].c0, c1 = g.seg[0].c1, K = c0 + c1, geglu = g.epi == EPI_GEGLU;
  const int fused = splitk & DV_GEMM_SPLITK_FUSED, slices = splitk & ~DV_GEMM_SPLITK_FUSED;
  const size_t el = (size_t)M * K;
  if (c1 > 0) {   // the two sources, each contiguous: [M, c0] then [M, c1] (k_split is elementwise: the planes keep that layout)
    float* xs = sc.get<float>(el * 4);
    sc.op("source copy ", [=](hipStream_t s) { return hipMemcpy2DAsync(xs, (size_t)c0 * 4, x, (size_t)K * 4, (size_t)c0 * 4, M, hipMemcpyDeviceToDevice, s); });
    sc.op("source copy ", [=](hipStream_t s) { return hipMemcpy2DAsync(xs + (size_t)M * c0, (size_t)c1 * 4, x + c0, (size_t)K * 4, (size_t)c1 * 4, M, hipMemcpyDeviceToDevice, s); });
    x = xs;
  }
  const Planes a = sc.split(x, el), a1 = c1 > 0 ? a.at((size_t)M * c0) : Planes{};
  g.seg[0].a0_hi = a.hi; g.seg[0].a0_lo = a.lo; g.seg[0].a1_hi = a1.hi; g.seg[0].a1_lo = a1.lo;
  const PackedW3 pw = sc.weights(N, K, geglu && bias);
  sc.pack(pw, w, 0, K, 1, K, 0, nullptr, geglu);
  if (pw.bias) sc.fold_bias(pw, nullptr, bias, nullptr, 1);
  if (slices) {
    g.sk_split = slices;
    g.sk_buf = sc.get<float>(gemm_splitk_bytes(M, N, slices));
    g.sk_ticket = fused ? sc.get<unsigned>(4096 * sizeof(unsigned), OpScratch::ZEROED) : nullptr;
  }
  sc.gemm(g, pw, bias, precision);
  return sc.run();
}

// dv_op_linear / dv_op_linear_planes: one source, the automatic tile, no split-K, any row count
static int linear(const float* x, const float* w, const float* bias, float* y, bf16_t* y_hi, bf16_t* y_lo, int M, int K, int N, int ldo, int geglu,
                  int precision, void* stream, const char* what) {
  if (!x || !w || (!y && !y_hi) || K % 32 != 0) return dv_fail(DV_ERR_INVALID, "%s: K must be a multiple of 32 (and an output is needed)", what);
  if (geglu && (N % 64 != 0 || y)) return dv_fail(DV_ERR_INVALID, "%s: GEGLU needs N %% 64 == 0 and writes planes only", what);
  const int n_out = geglu ? N / 2 : N;
  if (ldo < n_out) return dv_fail(DV_ERR_INVALID, "%s: ldo %d < %d output columns", what, ldo, n_out);
  if (2 * (size_t)K + 256 > DV_ZERO_PAGE_BYTES) return dv_fail(DV_ERR_INVALID, "%s: K = %d exceeds the %d channels one source tensor may have", what, K, (DV_ZERO_PAGE_BYTES - 256) / 2);
  GemmParams g = row_gemm_params(1, M, N, nullptr);
  g.seg[0] = seg1(nullptr, nullptr, K, 1, 0);
  g.epi = geglu ? EPI_GEGLU : EPI_STORE; g.out = y; g.out_hi = y_hi; g.out_lo = y_lo; g.ldo = ldo;
  return row_gemm(what, g, x, w, bias, 0, precision, stream);
}

extern "C" int dv_op_linear(const float* x, const float* w, const float* bias, float* y, int32_t M, int32_t K, int32_t N,
                            int32_t precision, void* stream) {
  return linear(x, w, bias, y, nullptr, nullptr, M, K, N, N, 0, precision, stream, "dv_op_linear");
}

extern "C" int dv_op_linear_planes(const float* x, const float* w, const float* bias, float* y, uint16_t* y_hi, uint16_t* y_lo, int32_t M,
                                   int32_t K, int32_t N, int32_t ldo, int32_t geglu, int32_t precision, void* stream) {
  if (!y_hi || (precision == DV_PREC_BF16X3 && !y_lo)) return dv_fail(DV_ERR_INVALID, "dv_op_linear_planes: plane outputs are required");
  return linear(x, w, bias, y, y_hi, precision == DV_PREC_BF16X3 ? y_lo : nullptr, M, K, N, ldo, geglu, precision, stream, "dv_op_linear_planes");
}

static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---- dv_op_gemm: k_gemm on a chosen menu entry, k-split form, epilogue and source layout (include/dvits_hip.h) ----
static_assert(DV_GT_AUTO == GT_AUTO && DV_GT_T0 == GT_T0 && DV_GT_T1 == GT_T1 && DV_GT_T2 == GT_T2 && DV_GT_T2S == GT_T2S && DV_GT_T2G == GT_T2G &&
              DV_GT_T3 == GT_T3 && DV_GT_T4 == GT_T4 && DV_GT_T4G == GT_T4G && DV_GT_T0S == GT_T0S && DV_GT_BK64 == GT_BK64, "public tile ids");
static_assert(DV_GEMM_STORE == EPI_STORE && DV_GEMM_RESIDUAL == EPI_RESIDUAL && DV_GEMM_GEGLU == EPI_GEGLU, "public epilogue ids");

// Checks everything launch_gemm / k_gemm need of the shape and fills the host-only fields of g (no pointers, nothing launched): the
// requirements are read from gemm_tile.h and launch_gemm, never found by launching.  0, or DV_ERR_INVALID with the message set.
static int gemm_op_shape(GemmParams& g, int M, int K, int N, int K0, int epi, int tile, int splitk, int precision, const char* what) {
  if (M <= 0 || N <= 0 || K <= 0 || M > 32768 || N > 32768) return dv_fail(DV_ERR_INVALID, "%s: M = %d, N = %d, K = %d: 1 .. 32768 rows and columns", what, M, N, K);
  if (precision != DV_PREC_BF16X3 && precision != DV_PREC_BF16) return dv_fail(DV_ERR_INVALID, "%s: precision %d is not a DV_PREC_*", what, precision);
  if (epi != DV_GEMM_STORE && epi != DV_GEMM_RESIDUAL && epi != DV_GEMM_GEGLU) return dv_fail(DV_ERR_INVALID, "%s: epilogue %d is not a DV_GEMM_*", what, epi);
  if (K0 < 0 || K0 >= K) return dv_fail(DV_ERR_INVALID, "%s: K0 = %d must be 0 or inside (0, K = %d)", what, K0, K);
  const int c0 = K0 > 0 ? K0 : K, c1 = K0 > 0 ? K - K0 : 0;
  if (c0 % 32 != 0 || c1 % 32 != 0) return dv_fail(DV_ERR_INVALID, "%s: source widths %d and %d must be multiples of 32 (the k-tile)", what, c0, c1);
  if (2 * (size_t)c0 + 256 > DV_ZERO_PAGE_BYTES || 2 * (size_t)c1 + 256 > DV_ZERO_PAGE_BYTES)
    return dv_fail(DV_ERR_INVALID, "%s: a source of %d channels exceeds the %d one source tensor may have", what, c0 > c1 ? c0 : c1, (DV_ZERO_PAGE_BYTES - 256) / 2);
  const int ft = tile & 0xff;
  if ((tile & ~(0xff | GT_BK64)) != 0 || ft > GT_T0S || (ft == GT_AUTO && tile != 0)) return dv_fail(DV_ERR_INVALID, "%s: tile 0x%x is not 0 or a DV_GT_* id (| DV_GT_BK64)", what, tile);
  if (tile & GT_BK64) {
    if (ft == GT_T0 || ft == GT_T0S) return dv_fail(DV_ERR_INVALID, "%s: the 128x128 tiles exist with 32-deep k-tiles only", what);
    if (c0 % 64 != 0 || c1 % 64 != 0) return dv_fail(DV_ERR_INVALID, "%s: 64-deep k-tiles need source widths that are multiples of 64, not %d and %d", what, c0, c1);
  }
  if (epi == DV_GEMM_GEGLU) {
    if (N % 64 != 0) return dv_fail(DV_ERR_INVALID, "%s: GEGLU needs N %% 64 == 0 ([32 value | 32 gate] column blocks), not N = %d", what, N);
    if (ft != GT_AUTO && !gemm_tile_geglu_ok(ft)) return dv_fail(DV_ERR_INVALID, "%s: GEGLU needs a tile with a 64-column block per wave (T0, T0S, T1, T2G, T4G), not tile %d", what, ft);
  }
  const int fused = splitk & DV_GEMM_SPLITK_FUSED, slices = splitk & ~DV_GEMM_SPLITK_FUSED;
  if (splitk != 0) {
    if (fused ? slices != 2 : (slices != 2 && slices != 3)) return dv_fail(DV_ERR_INVALID, "%s: splitk 0x%x: 2 or 3 slices in two launches, or 2 | DV_GEMM_SPLITK_FUSED", what, splitk);
    if (epi == DV_GEMM_GEGLU) return dv_fail(DV_ERR_INVALID, "%s: split-K runs the store and residual epilogues only (gemm_splitk_plan)", what);
    if (K / 64 < slices) return dv_fail(DV_ERR_INVALID, "%s: K = %d has fewer 64-deep k-tiles than the %d slices", what, K, slices);
    if (fused && ((M + 31) / 32) * ((N + 31) / 32) > 4096) return dv_fail(DV_ERR_INVALID, "%s: the fused pair has 4096 tile counters; M = %d, N = %d need more", what, M, N);
  }
  g = GemmParams{};
  g.seg[0].c0 = c0; g.seg[0].c1 = c1; g.seg[0].taps = 1;
  g.nseg = 1; g.B = 1; g.T_in = g.T_out = g.T_virt = M; g.stride = 1;
  g.Kp = K; g.N_pad = rup(N, 128); g.M = M; g.N = N; g.epi = epi; g.force_tile = tile;
  return DV_OK;
}

extern "C" int dv_op_gemm_variant(int32_t M, int32_t K, int32_t N, int32_t K0, int32_t epi, int32_t tile, int32_t splitk, int32_t precision,
                                  int32_t* variant, int32_t* tile_kind, int32_t* nsplit) {
  if (!variant || !tile_kind || !nsplit) return dv_fail(DV_ERR_INVALID, "dv_op_gemm_variant: null argument");
  GemmParams g;
  if (int rc = gemm_op_shape(g, M, K, N, K0, epi, tile, splitk, precision, "dv_op_gemm_variant")) return rc;
  const int v = gemm_variant(g);
  const int kind = gemm_variant_tile(g, v);
  if (v < 0 || kind < 0) return dv_fail(DV_ERR_INVALID, "dv_op_gemm_variant: no instantiation for tile 0x%x", tile);
  *variant = v; *tile_kind = kind; *nsplit = precision == DV_PREC_BF16X3 ? 3 : 1;
  return DV_OK;
}

extern "C" int dv_op_gemm(const float* x, const float* w, const float* bias, const float* res, const float* rowmask, float* y, uint16_t* y_hi,
                          uint16_t* y_lo, int32_t M, int32_t K, int32_t N, int32_t K0, int32_t ldo, int32_t ldres, int32_t epi, int32_t relu,
                          int32_t tile, int32_t splitk, int32_t precision, void* stream) {
  const char* what = "dv_op_gemm";
  GemmParams g;
  if (int rc = gemm_op_shape(g, M, K, N, K0, epi, tile, splitk, precision, what)) return rc;
  const bool x3 = precision == DV_PREC_BF16X3;
  if (!x || !w || (!y && !y_hi)) return dv_fail(DV_ERR_INVALID, "%s: x, w and an output (y and / or y_hi) are required", what);
  if (y_hi && x3 && !y_lo) return dv_fail(DV_ERR_INVALID, "%s: bf16x3 plane output needs y_lo", what);
  if (!y_hi && y_lo) return dv_fail(DV_ERR_INVALID, "%s: y_lo without y_hi", what);
  const int n_out = epi == DV_GEMM_GEGLU ? N / 2 : N;
  if (ldo < n_out) return dv_fail(DV_ERR_INVALID, "%s: ldo %d < %d output columns", what, ldo, n_out);
  if (epi == DV_GEMM_RESIDUAL ? (!res || ldres < N) : (res != nullptr)) return dv_fail(DV_ERR_INVALID, "%s: res [M, ldres >= N] goes with DV_GEMM_RESIDUAL, and only with it", what);
  if (relu != 0 && relu != 1) return dv_fail(DV_ERR_INVALID, "%s: relu is 0 or 1", what);
  if (epi == DV_GEMM_GEGLU && (relu || rowmask)) return dv_fail(DV_ERR_INVALID, "%s: the GEGLU epilogue has no ReLU / row mask", what);
  // 16-byte epilogue accesses are taken on the pitches alone (gemm_tile.h vec4 / al8): the bases must allow them
  if (!al16(y) || !al16(res) || !al16(y_hi) || !al16(y_lo) || !al16(x)) return dv_fail(DV_ERR_INVALID, "%s: x, res and the outputs must be 16-byte aligned", what);
  g.res = res; g.ldres = ldres; g.relu = relu; g.rowmask = rowmask;
  g.out = y; g.out_hi = y_hi; g.out_lo = x3 ? y_lo : nullptr; g.ldo = ldo;
  return row_gemm(what, g, x, w, bias, splitk, precision, stream);
}

// ---- dv_op_conv_rows: k_gemm's convolution operand path (gemm_tile.h prep_a / advance / utt_of) as Builder::resample and the resnet
// fallback launch it: channels-last sources in a padded row space, taps, stride 2, nearest upsampling, [a0 | a1], a second k-segment ----
static_assert(DV_UP_NONE == UP_NONE && DV_UP_X2 == UP_X2 && DV_UP_SIZE == UP_SIZE, "public upsampling modes");
constexpr int CONV_ROWS_GUARD = 32;   // rows of NaN behind every operand plane the kernel reads

// Checks the shape and fills the host-only fields of g (no pointers, nothing launched).  0, or DV_ERR_INVALID with the message set.
static int conv_rows_shape(GemmParams& g, int B, int T, int Tp_in, int c0, int c1, int c_sc, int Cout, int taps, int stride, int up_mode,
                           int up_T, int Tp_out, int with_stats, int tile, int precision, const char* what) {
  if (B <= 0 || T <= 0 || Tp_in < T || Tp_in > 32768 || c0 <= 0 || c1 < 0 || c_sc < 0 || Cout <= 0 || Tp_out <= 0 || Tp_out > 32768)
    return dv_fail(DV_ERR_INVALID, "%s: B = %d, T = %d, Tp_in = %d, c0 = %d, c1 = %d, c_sc = %d, Cout = %d, Tp_out = %d: positive sizes, T <= Tp_in <= 32768", what, B, T, Tp_in, c0, c1, c_sc, Cout, Tp_out);
  if (taps != 1 && taps != 3) return dv_fail(DV_ERR_INVALID, "%s: taps = %d is not 1 or 3", what, taps);
  if (stride != 1 && stride != 2) return dv_fail(DV_ERR_INVALID, "%s: stride = %d is not 1 or 2", what, stride);
  if (up_mode != DV_UP_NONE && up_mode != DV_UP_X2 && up_mode != DV_UP_SIZE) return dv_fail(DV_ERR_INVALID, "%s: up_mode %d is not a DV_UP_*", what, up_mode);
  if (up_mode == DV_UP_SIZE ? (up_T <= 0 || up_T > 32768) : up_T != 0) return dv_fail(DV_ERR_INVALID, "%s: up_T = %d goes with DV_UP_SIZE (1 .. 32768 frames), and only with it", what, up_T);
  if (up_mode != DV_UP_NONE && stride != 1) return dv_fail(DV_ERR_INVALID, "%s: upsampling runs with stride 1 only", what);
  if (c_sc > 0 && (stride != 1 || up_mode != DV_UP_NONE)) return dv_fail(DV_ERR_INVALID, "%s: the second k-segment needs stride 1 and no upsampling (its rows are gathered like the first's)", what);
  if (c_sc % 32 != 0) return dv_fail(DV_ERR_INVALID, "%s: source widths %d, %d and %d must be multiples of 32 (the k-tile)", what, c0, c1, c_sc);
  if (2 * (size_t)c_sc + 256 > DV_ZERO_PAGE_BYTES) return dv_fail(DV_ERR_INVALID, "%s: a source of %d channels exceeds the %d one source tensor may have", what, c_sc, (DV_ZERO_PAGE_BYTES - 256) / 2);
  if ((tile & GT_BK64) && c_sc % 64 != 0) return dv_fail(DV_ERR_INVALID, "%s: 64-deep k-tiles need source widths that are multiples of 64, not %d", what, c_sc);
  const int pad = (taps - 1) / 2;
  const int T_virt = up_mode == DV_UP_X2 ? 2 * T : (up_mode == DV_UP_SIZE ? up_T : T);
  const int Tv_out = (T_virt + 2 * pad - taps) / stride + 1;
  if (Tp_out < Tv_out) return dv_fail(DV_ERR_INVALID, "%s: Tp_out = %d < the %d output frames", what, Tp_out, Tv_out);
  if ((long long)B * Tp_out > 32768) return dv_fail(DV_ERR_INVALID, "%s: B x Tp_out = %lld rows: at most 32768", what, (long long)B * Tp_out);
  if (with_stats && (Cout % 16 != 0 || Tp_out % 32 != 0 || Tv_out <= Tp_out - 32))
    return dv_fail(DV_ERR_INVALID, "%s: stats16 needs Cout %% 16 == 0 and Tp_out = the %d frames rounded up to 32, not Cout = %d, Tp_out = %d", what, Tv_out, Cout, Tp_out);
  // (tile, precision, the widths of [a0 | a1]: op_gemm's checks on the same launch shape)
  if (int rc = gemm_op_shape(g, B * Tp_out, c0 + c1, Cout, c1 > 0 ? c0 : 0, DV_GEMM_STORE, tile, 0, precision, what)) return rc;
  g.seg[0].taps = taps; g.seg[0].pad = pad;
  if (c_sc > 0) { g.seg[1].c0 = c_sc; g.seg[1].taps = 1; g.seg[1].pad = 0; g.nseg = 2; }
  g.B = B; g.T_in = Tp_in; g.Tv_in = T; g.T_virt = T_virt; g.Tv_out = Tv_out; g.T_out = Tp_out;
  g.stride = stride; g.up_mode = up_mode;
  g.up_scale = up_mode == DV_UP_SIZE ? (float)T / (float)up_T : 1.f;
  g.Kp = taps * (c0 + c1) + c_sc; g.ldo = Cout;
  return DV_OK;
}

extern "C" int dv_op_conv_rows_variant(int32_t B, int32_t T, int32_t Tp_in, int32_t c0, int32_t c1, int32_t c_sc, int32_t Cout, int32_t taps,
                                       int32_t stride, int32_t up_mode, int32_t up_T, int32_t Tp_out, int32_t tile, int32_t precision,
                                       int32_t* variant, int32_t* tile_kind, int32_t* nsplit, int32_t* candidates, int32_t cap) {
  const char* what = "dv_op_conv_rows_variant";
  if (!variant || !tile_kind || !nsplit || cap < 0 || (cap > 0 && !candidates)) return dv_fail(DV_ERR_INVALID, "%s: null argument", what);
  GemmParams g;
  if (int rc = conv_rows_shape(g, B, T, Tp_in, c0, c1, c_sc, Cout, taps, stride, up_mode, up_T, Tp_out, 0, tile, precision, what)) return rc;
  const int v = gemm_variant(g);
  const int kind = gemm_variant_tile(g, v);
  if (v < 0 || kind < 0) return dv_fail(DV_ERR_INVALID, "%s: no instantiation for tile 0x%x", what, tile);
  *variant = v; *tile_kind = kind; *nsplit = precision == DV_PREC_BF16X3 ? 3 : 1;
  int cand[16];
  const int n = gemm_candidates(g, cand, 16);
  for (int i = 0; i < cap; ++i) candidates[i] = i < n ? cand[i] : 0;   // (0 = DV_GT_AUTO ends the list)
  return DV_OK;
}

extern "C" int dv_op_conv_rows(const float* x0, const float* x1, const float* w, const float* bias, const float* x_sc, const float* w_sc,
                               float* y, uint16_t* y_hi, uint16_t* y_lo, float* stats16, int32_t B, int32_t T, int32_t Tp_in, int32_t c0,
                               int32_t c1, int32_t c_sc, int32_t Cout, int32_t taps, int32_t stride, int32_t up_mode, int32_t up_T,
                               int32_t Tp_out, int32_t tile, int32_t precision, void* stream) {
  const char* what = "dv_op_conv_rows";
  GemmParams g;
  if (int rc = conv_rows_shape(g, B, T, Tp_in, c0, c1, c_sc, Cout, taps, stride, up_mode, up_T, Tp_out, stats16 != nullptr, tile, precision, what)) return rc;
  const bool x3 = precision == DV_PREC_BF16X3;
  if (!x0 || !w || (!y && !y_hi)) return dv_fail(DV_ERR_INVALID, "%s: x0, w and an output (y and / or y_hi) are required", what);
  if ((c1 > 0) != (x1 != nullptr)) return dv_fail(DV_ERR_INVALID, "%s: x1 goes with c1 > 0, and only with it", what);
  if (c_sc > 0 ? (!x_sc || !w_sc) : (x_sc || w_sc)) return dv_fail(DV_ERR_INVALID, "%s: x_sc and w_sc go with c_sc > 0, and only with it", what);
  if (y_hi && x3 && !y_lo) return dv_fail(DV_ERR_INVALID, "%s: bf16x3 plane output needs y_lo", what);
  if (!y_hi && y_lo) return dv_fail(DV_ERR_INVALID, "%s: y_lo without y_hi", what);
  if (!al16(y) || !al16(y_hi) || !al16(y_lo) || !al16(x0) || !al16(x1) || !al16(x_sc) || !al16(stats16))
    return dv_fail(DV_ERR_INVALID, "%s: the sources and the outputs must be 16-byte aligned", what);
  OpScratch sc(what, stream, precision);
  if (int rc = sc.start()) return rc;
  // every operand plane: [B * Tp_in rows | CONV_ROWS_GUARD rows of bf16 NaN] - a gather that runs past the last utterance shows
  const size_t rows = (size_t)B * Tp_in;
  auto operand = [&](const float* src, int c) { return c > 0 ? sc.split(src, rows * c, (size_t)CONV_ROWS_GUARD * c) : Planes{}; };
  const Planes a0 = operand(x0, c0), a1 = operand(x1, c1), a2 = operand(x_sc, c_sc);
  g.seg[0].a0_hi = a0.hi; g.seg[0].a0_lo = a0.lo; g.seg[0].a1_hi = a1.hi; g.seg[0].a1_lo = a1.lo;
  g.seg[1].a0_hi = a2.hi; g.seg[1].a0_lo = a2.lo;
  const PackedW3 pw = sc.weights(Cout, g.Kp);
  sc.pack(pw, w, 1, c0 + c1, taps, c0 + c1);
  if (c_sc > 0) sc.pack(pw, w_sc, 1, c_sc, 1, c_sc, taps * (c0 + c1));
  g.out = y; g.out_hi = y_hi; g.out_lo = x3 ? y_lo : nullptr; g.stats16 = stats16;
  sc.gemm(g, pw, bias, precision);   // (no fragment-major weights: always k_gemm)
  return sc.run();
}

extern "C" int dv_op_group_stats(const float* x, float* mean, float* rstd, int32_t B, int32_t T, int32_t C, int32_t groups,
                                 float eps, void* stream) {
  if (!x || !mean || !rstd || C % groups != 0 || (C / groups) % 4 != 0 || groups > 64)
    return dv_fail(DV_ERR_INVALID, "dv_op_group_stats: bad argument");
  OpScratch sc("dv_op_group_stats", stream);
  const int nchunk = std::max(1, std::min(64, (T + 63) / 64));
  double* part = sc.get<double>((size_t)B * nchunk * groups * 2 * sizeof(double), OpScratch::OUTSIDE);   // (k_gn_partial writes all of it)
  sc.op("k_gn_partial ", [=](hipStream_t s) { return launch_gn_partial(x, C, nullptr, 0, part, B, T, groups, nchunk, s); });
  sc.op("k_gn_finalize ", [=](hipStream_t s) {
    return launch_gn_finalize(part, nchunk, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, mean, rstd, B, T, C, groups, eps, s);
  });
  return sc.run();
}

extern "C" int dv_op_attention_prec(const float* q, const float* k, const float* v, const float* bias, float* o, int32_t B,
                                    int32_t H, int32_t Tq, int32_t Tk, int32_t d, int32_t precision, void* stream) {
  if (!q || !k || !v || !o) return dv_fail(DV_ERR_INVALID, "dv_op_attention: null argument");
  if (precision != DV_PREC_BF16X3 && precision != DV_PREC_BF16) return dv_fail(DV_ERR_INVALID, "dv_op_attention: precision %d is not a DV_PREC_*", precision);
  if (B <= 0 || H <= 0 || Tq <= 0 || Tk <= 0) return dv_fail(DV_ERR_INVALID, "dv_op_attention: B, H, Tq and Tk must be positive");
  AttnParams a{};
  a.q = q; a.k = k; a.v = v; a.bias = bias; a.o = o; a.o_hi = nullptr; a.o_lo = nullptr;
  a.ldq = a.ldk = a.ldv = a.ldo = H * d;
  a.B = B; a.H = H; a.Tq = Tq; a.Tk = Tk; a.d = d; a.scale = 1.0f / sqrtf((float)d); a.nsplit = precision == DV_PREC_BF16X3 ? 3 : 1;
  HIPCHK(attn_init());
  hipError_t e = launch_attention(a, (hipStream_t)stream);
  if (e != hipSuccess) return dv_fail(DV_ERR_HIP, "attention launch failed: %s (d must be a multiple of 4, <= 64)", hipGetErrorString(e));
  return DV_OK;
}

extern "C" int dv_op_attention(const float* q, const float* k, const float* v, const float* bias, float* o, int32_t B,
                               int32_t H, int32_t Tq, int32_t Tk, int32_t d, void* stream) {
  return dv_op_attention_prec(q, k, v, bias, o, B, H, Tq, Tk, d, DV_PREC_BF16X3, stream);
}

// k_attention_frag as the forward runs its cross attention: K | V -> split fragments in the hoisted layout (launch_kv_frag), the
// key bias as log2-domain rows of whole 32-key tiles (launch_xbias), then launch_attention_frag's own choice of instantiation
extern "C" int dv_op_attention_frag(const float* q, const float* k, const float* v, const float* bias, float* o, int32_t B,
                                    int32_t H, int32_t Tq, int32_t Tk, int32_t d, void* stream) {
  if (!q || !k || !v || !o || B <= 0 || H <= 0 || Tq <= 0 || Tk <= 0) return dv_fail(DV_ERR_INVALID, "dv_op_attention_frag: bad argument");
  if (d <= 0 || d % 16 != 0 || d > 64) return dv_fail(DV_ERR_INVALID, "dv_op_attention_frag: d = %d must be a multiple of 16, <= 64", d);
  OpScratch sc("dv_op_attention_frag", stream);
  HIPCHK(attn_init());
  const int C = H * d, nT = (Tk + 31) / 32, KSq = d / 16, NBv = (d + 31) / 32;
  const size_t rows = (size_t)B * Tk;
  float* kv = sc.get<float>(rows * 2 * C * 4);
  const Planes kf = sc.planes((size_t)B * H * nT * KSq * 64 * 8), vf = sc.planes((size_t)B * H * nT * 2 * NBv * 64 * 8);
  float* xb = sc.get<float>((size_t)B * nT * 32 * 4);
  sc.op("K copy ", [=](hipStream_t s) { return hipMemcpy2DAsync(kv, (size_t)2 * C * 4, k, (size_t)C * 4, (size_t)C * 4, rows, hipMemcpyDeviceToDevice, s); });
  sc.op("V copy ", [=](hipStream_t s) { return hipMemcpy2DAsync(kv + C, (size_t)2 * C * 4, v, (size_t)C * 4, (size_t)C * 4, rows, hipMemcpyDeviceToDevice, s); });
  sc.op("k_kv_frag ", [=](hipStream_t s) { return launch_kv_frag(kv, kf.hi, kf.lo, vf.hi, vf.lo, B, Tk, C, H, s); });
  sc.op("k_xbias ", [=](hipStream_t s) { return launch_xbias(bias, xb, B, Tk, nT, s); });
  AttnFragParams a{};
  a.q = q; a.ldq = C;
  a.kf_hi = kf.hi; a.kf_lo = kf.lo; a.vf_hi = vf.hi; a.vf_lo = vf.lo;
  a.k_b = H * nT * KSq; a.k_h = nT * KSq; a.k_t = KSq;
  a.v_b = H * nT * 2 * NBv; a.v_h = nT * 2 * NBv; a.v_t = 2 * NBv; a.v_kb = NBv; a.v_nb = 1; a.self_layout = 0;
  a.bias = xb; a.bias_ld = nT * 32;
  a.o = o; a.o_hi = nullptr; a.o_lo = nullptr; a.ldo = C;
  a.B = B; a.H = H; a.Tq = Tq; a.Tk = Tk; a.d = d; a.scale = 1.0f / sqrtf((float)d); a.nsplit = 3;
  sc.op("", [=](hipStream_t s) { return launch_attention_frag(a, s); });
  return sc.run();
}

// The k = 3 convolutions of ResnetBlock2D / Upsample2D as the forward launches them: split planes of a channels-last input in a
// (padded) row space, packed weights AND their fragment-major copies, through launch_gemm - which then routes to k_conv3 /
// k_conv3s / k_conv3u.  A shape launch_gemm would hand to k_gemm is refused.
extern "C" int dv_op_conv3(const float* x, const float* w, const float* bias, const float* x_sc, const float* w_sc, float* y, int32_t B,
                           int32_t Cin, int32_t T, int32_t Tp, int32_t Cout, int32_t Csc, int32_t up2, void* stream) {
  if (!x || !w || !y || B <= 0 || Cin <= 0 || T <= 0 || Tp < T || Cout <= 0 || Csc < 0 || (Csc > 0 && (!x_sc || !w_sc || up2)))
    return dv_fail(DV_ERR_INVALID, "dv_op_conv3: bad argument");
  if (Cin % 64 != 0 || Csc % 64 != 0 || 2 * (size_t)std::max(Cin, Csc) + 256 > DV_ZERO_PAGE_BYTES)
    return dv_fail(DV_ERR_INVALID, "dv_op_conv3: Cin = %d / Csc = %d must be multiples of 64 within one source tensor's width", Cin, Csc);
  OpScratch sc("dv_op_conv3", stream);
  if (int rc = sc.start()) return rc;
  const int Kp = 3 * Cin + Csc;
  const int Tv_out = up2 ? 2 * T : T, T_out = up2 ? rup(2 * T, 32) : Tp;
  GemmParams g{};
  g.nseg = Csc > 0 ? 2 : 1; g.B = B;
  g.T_in = Tp; g.Tv_in = T; g.T_out = T_out; g.Tv_out = g.T_virt = Tv_out;
  g.stride = 1; g.up_mode = up2 ? UP_X2 : UP_NONE;
  g.M = B * T_out; g.N = Cout; g.epi = EPI_STORE; g.ldo = Cout; g.ldres = Cout; g.Kp = Kp; g.N_pad = rup(Cout, 128); g.out = y;
  g.seg[0] = seg1(nullptr, nullptr, Cin, 3, 1);
  if (Csc > 0) g.seg[1] = seg1(nullptr, nullptr, Csc, 1, 0);
  const int route = gemm_conv3_up_ok(g) ? 2 : ((gemm_conv3_shape_ok(g) && Kp == gemm_conv3_k(g)) ? 1 : 0);
  if (route == 0)
    return dv_fail(DV_ERR_INVALID, "dv_op_conv3: B=%d Cin=%d T=%d Tp=%d Cout=%d Csc=%d up2=%d is not a shape of the convolution kernels "
                   "(it would run on k_gemm)", B, Cin, T, Tp, Cout, Csc, up2);
  const Planes a = sc.split(x, (size_t)B * Tp * Cin), s = Csc > 0 ? sc.split(x_sc, (size_t)B * Tp * Csc) : Planes{};
  g.seg[0].a0_hi = a.hi; g.seg[0].a0_lo = a.lo; g.seg[1].a0_hi = s.hi; g.seg[1].a0_lo = s.lo;
  const PackedW3 pw = sc.weights(Cout, Kp);
  sc.pack(pw, w, 1, Cin, 3, Cin);
  if (Csc > 0) sc.pack(pw, w_sc, 1, Csc, 1, Csc, 3 * Cin);
  const Planes f = sc.planes((size_t)pw.N_pad * Kp);   // the weights fragment-major
  sc.op("k_relayout_frag ", [=](hipStream_t t) { return launch_relayout_frag(pw.hi, f.hi, pw.N_pad, Kp, t); });
  sc.op("k_relayout_frag ", [=](hipStream_t t) { return launch_relayout_frag(pw.lo, f.lo, pw.N_pad, Kp, t); });
  g.wf_hi = f.hi; g.wf_lo = f.lo;
  if (route == 1) {   // the 128-frame level's long-K convolutions run as a fused split-K pair on the streaming kernel: here too
    int dev = 0, n_cu = 0;
    (void)hipGetDevice(&dev); (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev);
    if (gemm_conv3_split(g, n_cu) == 2 && ((g.M + 31) / 32) * ((g.N + 31) / 32) <= 4096) {
      g.sk_split = 2;
      g.sk_buf = sc.get<float>(gemm_conv3_split_bytes(g));
      g.sk_ticket = sc.get<unsigned>(4096 * sizeof(unsigned), OpScratch::ZEROED);
    }
  }
  sc.gemm(g, pw, bias, DV_PREC_BF16X3);
  return sc.run();
}

// ----------------------------------------------------------------------------- normalisation entry points
// The LayerNorm / GroupNorm routes of the forward through the launchers the engine calls (include/dvits_hip.h).

extern "C" int dv_op_layer_norm(const float* x, const float* gamma, const float* beta, const float* rowmask, float* y, uint16_t* y_hi,
                                uint16_t* y_lo, float* mean, float* rstd, int32_t M, int32_t C, float eps, int32_t route, void* stream) {
  if (!x || M <= 0 || C <= 0 || !(eps >= 0.f) || !std::isfinite(eps)) return dv_fail(DV_ERR_INVALID, "dv_op_layer_norm: bad argument");
  if (C % 4 != 0 || C > 2048) return dv_fail(DV_ERR_INVALID, "dv_op_layer_norm: C = %d must be a multiple of 4, <= 2048", C);
  if (!al16(x) || !al16(gamma) || !al16(beta) || !al16(y) || !al16(y_hi) || !al16(y_lo))
    return dv_fail(DV_ERR_INVALID, "dv_op_layer_norm: x, gamma, beta and the outputs must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipError_t e;
  switch (route) {
    case DV_LN_STATS:
      if (!mean || !rstd || y || y_hi || y_lo || rowmask) return dv_fail(DV_ERR_INVALID, "dv_op_layer_norm: DV_LN_STATS writes mean and rstd only");
      e = launch_ln_stats(x, mean, rstd, M, C, eps, st);
      break;
    case DV_LN_ROWS:
      if (!gamma || !beta || !y || y_hi || y_lo || mean || rstd || rowmask) return dv_fail(DV_ERR_INVALID, "dv_op_layer_norm: DV_LN_ROWS needs gamma, beta and y only");
      e = launch_layernorm_rows(x, gamma, beta, y, M, C, eps, st);
      break;
    case DV_LN_APPLY:
      if (!y_hi || y || gamma || beta || mean || rstd || rowmask) return dv_fail(DV_ERR_INVALID, "dv_op_layer_norm: DV_LN_APPLY writes planes only, without affine");
      e = launch_ln_apply(x, y_hi, y_lo, M, C, eps, st);
      break;
    case DV_LN_AFFINE:
      if (!gamma || !beta || (!y && !y_hi) || (y_lo && !y_hi) || mean || rstd) return dv_fail(DV_ERR_INVALID, "dv_op_layer_norm: DV_LN_AFFINE needs gamma, beta and y and / or planes");
      e = launch_ln_affine(x, gamma, beta, rowmask, y, y_hi, y_lo, M, C, eps, st);
      break;
    default:
      return dv_fail(DV_ERR_INVALID, "dv_op_layer_norm: route %d is not one of DV_LN_*", route);
  }
  if (e != hipSuccess) return dv_fail(DV_ERR_HIP, "dv_op_layer_norm: launch failed: %s", hipGetErrorString(e));
  HIPCHK(hipStreamSynchronize(st));
  return DV_OK;
}

extern "C" int dv_op_layer_norm_into(const float* x, const float* gamma, const float* beta, float* y, int32_t M, int32_t C, float eps,
                                     int32_t rows_per_batch, int32_t out_rows_per_batch, int32_t out_row_off, void* stream) {
  if (!x || !gamma || !beta || !y || M <= 0 || C <= 0 || !(eps >= 0.f) || !std::isfinite(eps)) return dv_fail(DV_ERR_INVALID, "dv_op_layer_norm_into: bad argument");
  if (C % 4 != 0 || C > 2048) return dv_fail(DV_ERR_INVALID, "dv_op_layer_norm_into: C = %d must be a multiple of 4, <= 2048", C);
  if (rows_per_batch <= 0 || M % rows_per_batch != 0 || out_row_off < 0 || out_row_off > out_rows_per_batch - rows_per_batch)
    return dv_fail(DV_ERR_INVALID, "dv_op_layer_norm_into: %d rows per utterance do not fit slots of %d rows at offset %d (M = %d)", rows_per_batch,
                   out_rows_per_batch, out_row_off, M);
  if (!al16(x) || !al16(gamma) || !al16(beta) || !al16(y)) return dv_fail(DV_ERR_INVALID, "dv_op_layer_norm_into: pointers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = launch_layernorm_rows_into(x, gamma, beta, y, M, C, eps, rows_per_batch, out_rows_per_batch, out_row_off, st);
  if (e != hipSuccess) return dv_fail(DV_ERR_HIP, "dv_op_layer_norm_into: launch failed: %s", hipGetErrorString(e));
  HIPCHK(hipStreamSynchronize(st));
  return DV_OK;
}

extern "C" int dv_op_prompt_pre(const float* prompt, const float* keep, const float* gamma, const float* beta, uint16_t* hi, uint16_t* lo,
                                float* key_bias, int32_t B, int32_t C, int32_t L, int32_t cpad, float eps, void* stream) {
  if (!prompt || !keep || !gamma || !beta || !hi || !key_bias || B <= 0 || L <= 0 || !(eps >= 0.f) || !std::isfinite(eps))
    return dv_fail(DV_ERR_INVALID, "dv_op_prompt_pre: bad argument");
  if (C < 1 || C > 512 || cpad < C || cpad > 512) return dv_fail(DV_ERR_INVALID, "dv_op_prompt_pre: 1 <= C = %d <= cpad = %d <= 512 is required", C, cpad);
  if ((int64_t)B * L > INT32_MAX / 512) return dv_fail(DV_ERR_INVALID, "dv_op_prompt_pre: B * L = %lld exceeds %d", (long long)B * L, INT32_MAX / 512);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = launch_prompt_pre(prompt, keep, gamma, beta, hi, lo, key_bias, B, C, L, cpad, eps, st);
  if (e != hipSuccess) return dv_fail(DV_ERR_HIP, "dv_op_prompt_pre: launch failed: %s", hipGetErrorString(e));
  HIPCHK(hipStreamSynchronize(st));
  return DV_OK;
}

// ----------------------------------------------------------------------------- conditioning entry points
// The fp32 kernels of the conditioning path (kernels_misc.hip) through the launchers the cond and step schedules call.

extern "C" int dv_op_timestep_embedding(const float* t, float* out, int32_t B, int32_t dim, void* stream) {
  if (!t || !out) return dv_fail(DV_ERR_INVALID, "dv_op_timestep_embedding: null pointer");
  if (B < 1 || dim < 2 || dim % 2 != 0 || (int64_t)B * (dim / 2) > INT32_MAX - 256)
    return dv_fail(DV_ERR_INVALID, "dv_op_timestep_embedding: B = %d >= 1 rows of an even dim = %d >= 2, B * dim / 2 < 2^31 - 256, are required", B, dim);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = launch_timestep_sincos(t, out, B, dim, st);
  if (e != hipSuccess) return dv_fail(DV_ERR_HIP, "dv_op_timestep_embedding: launch failed: %s", hipGetErrorString(e));
  HIPCHK(hipStreamSynchronize(st));
  return DV_OK;
}

extern "C" int dv_op_small_linear(const float* in, int32_t ldin, const float* w, const float* bias, const float* add, float* out, int32_t ldo,
                                  int32_t M, int32_t K, int32_t N, int32_t silu_in, int32_t silu_out, int32_t route, int32_t add_rows,
                                  void* stream) {
  if (!in || !w || !out) return dv_fail(DV_ERR_INVALID, "dv_op_small_linear: null pointer");
  if (route != 0 && route != 1) return dv_fail(DV_ERR_INVALID, "dv_op_small_linear: route %d is neither 0 (k_small_linear) nor 1 (k_small_linear_t)", route);
  if ((silu_in != 0 && silu_in != 1) || (silu_out != 0 && silu_out != 1)) return dv_fail(DV_ERR_INVALID, "dv_op_small_linear: silu_in and silu_out are 0 or 1");
  if (M < 1 || M > 65536 || K < 1 || K > 16384 || N < 1 || N > (1 << 20))
    return dv_fail(DV_ERR_INVALID, "dv_op_small_linear: 1 <= M = %d <= 65536, 1 <= K = %d <= 16384, 1 <= N = %d <= 2^20 are required", M, K, N);
  if (ldin < K || ldo < N) return dv_fail(DV_ERR_INVALID, "dv_op_small_linear: ldin = %d >= K = %d and ldo = %d >= N = %d are required", ldin, K, ldo, N);
  if (add_rows < 0 || (add_rows > 0 && (route != 1 || !add)))
    return dv_fail(DV_ERR_INVALID, "dv_op_small_linear: add_rows = %d needs route 1 and an add tensor", add_rows);
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = route == 0 ? launch_small_linear(in, ldin, w, bias, add, out, ldo, M, K, N, silu_in, silu_out, st)
                                  : launch_small_linear_t(in, ldin, w, bias, add, out, ldo, M, K, N, silu_in, silu_out, st, add_rows);
  if (e == hipErrorInvalidValue)   // the launchers' own refusals: nothing was launched
    return route == 0 ? dv_fail(DV_ERR_INVALID, "dv_op_small_linear: M x K = %d x %d floats exceed the 64 KiB of LDS k_small_linear stages its rows in", M, K)
                      : dv_fail(DV_ERR_INVALID, "dv_op_small_linear: K = %d exceeds the 512 input columns k_small_linear_t's 64 KiB of LDS hold", K);
  if (e != hipSuccess) return dv_fail(DV_ERR_HIP, "dv_op_small_linear: launch failed: %s", hipGetErrorString(e));
  HIPCHK(hipStreamSynchronize(st));
  return DV_OK;
}

extern "C" int dv_op_pool_attention(float* seq, const float* pos, const float* q, const float* kv, float* out, int32_t B, int32_t L, int32_t D,
                                    int32_t heads, int32_t stage, void* stream) {
  if (stage != 0 && stage != 1) return dv_fail(DV_ERR_INVALID, "dv_op_pool_attention: stage %d is neither 0 (k_mean_token) nor 1 (k_pool_attn)", stage);
  if (B < 1 || B > 65535 || L < 1 || L > (1 << 20) || D < 1 || D > 8192)
    return dv_fail(DV_ERR_INVALID, "dv_op_pool_attention: 1 <= B = %d <= 65535, 1 <= L = %d <= 2^20, 1 <= D = %d <= 8192 are required", B, L, D);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e;
  if (stage == 0) {
    if (!seq || !pos || q || kv || out) return dv_fail(DV_ERR_INVALID, "dv_op_pool_attention: stage 0 takes seq and pos only");
    e = launch_mean_token(seq, pos, B, L, D, st);
  } else {
    if (!q || !kv || !out || seq || pos) return dv_fail(DV_ERR_INVALID, "dv_op_pool_attention: stage 1 takes q, kv and out only");
    if (heads < 1 || heads > 65535 || D % heads != 0) return dv_fail(DV_ERR_INVALID, "dv_op_pool_attention: D = %d is not a multiple of heads = %d >= 1", D, heads);
    e = launch_pool_attn(q, kv, out, B, L + 1, D, heads, st);
    if (e == hipErrorInvalidValue)   // the launcher's own refusal: nothing was launched
      return dv_fail(DV_ERR_INVALID, "dv_op_pool_attention: D / heads = %d exceeds the 8 channels per head k_pool_attn accumulates", D / heads);
  }
  if (e != hipSuccess) return dv_fail(DV_ERR_HIP, "dv_op_pool_attention: launch failed: %s", hipGetErrorString(e));
  HIPCHK(hipStreamSynchronize(st));
  return DV_OK;
}

// Producer GEMM (+ residual) with the raw planes and the row partials of ln_produce, then the consumer GEMM as ln_consume sets it
// up: gamma folded into the packed weights, u and the beta-folded bias by the packing launchers Builder::pack runs.
extern "C" int dv_op_linear_ln(const float* x, const float* w1, const float* b1, const float* res, const float* gamma, const float* beta,
                               const float* w2, const float* b2, int32_t M, int32_t K, int32_t C, int32_t N, int32_t fused, float* y1,
                               float* rowstat, float* y2, void* stream) {
  if (!x || !w1 || !gamma || !beta || !w2 || !y1 || !y2 || M <= 0 || N <= 0 || (fused != 0 && fused != 1) || (fused && !rowstat))
    return dv_fail(DV_ERR_INVALID, "dv_op_linear_ln: bad argument");
  if (K <= 0 || K % 32 != 0 || 2 * (size_t)K + 256 > DV_ZERO_PAGE_BYTES) return dv_fail(DV_ERR_INVALID, "dv_op_linear_ln: K = %d must be a multiple of 32 within one source tensor's width", K);
  if (C <= 0 || C % 32 != 0 || C > 512) return dv_fail(DV_ERR_INVALID, "dv_op_linear_ln: C = %d must be a multiple of 32, <= 512 (the consumer holds 16 partials per row)", C);
  OpScratch sc("dv_op_linear_ln", stream);
  if (int rc = sc.start()) return rc;
  const Planes a = sc.split(x, (size_t)M * K);
  const PackedW3 pw1 = sc.weights(C, K), pw2 = sc.weights(N, C, true);
  sc.pack(pw1, w1, 0, K, 1, K);
  sc.pack(pw2, w2, 0, C, 1, C, 0, gamma);   // (both routes: k_ln_apply has no affine either)
  float* u = sc.get<float>((size_t)pw2.N_pad * 4, OpScratch::ZEROED);
  sc.op("u fold ", [=](hipStream_t s) { return launch_fold_bias(w2, nullptr, gamma, u, N, C, 0, 0, s); });
  sc.fold_bias(pw2, w2, b2, beta, 0);
  const Planes p = sc.planes((size_t)M * C);   // the producer's raw output, the consumer's operand
  GemmParams g = row_gemm_params(1, M, C, nullptr);
  g.seg[0] = seg1(a.hi, a.lo, K, 1, 0);
  g.epi = res ? EPI_RESIDUAL : EPI_STORE; g.res = res; g.out = y1;
  if (fused) { g.out_hi = p.hi; g.out_lo = p.lo; g.rowstat_out = rowstat; }
  sc.gemm(g, pw1, b1, DV_PREC_BF16X3, "producer ");
  if (!fused) sc.op("k_ln_apply ", [=](hipStream_t s) { return launch_ln_apply(y1, p.hi, p.lo, M, C, 1e-5f, s); });
  GemmParams c = row_gemm_params(1, M, N, nullptr);
  c.seg[0] = seg1(p.hi, p.lo, C, 1, 0);
  c.out = y2;
  if (fused) { c.ln_stat = rowstat; c.ln_nblk = C / 32; c.ln_u = u; c.ln_eps = 1e-5f; }
  sc.gemm(c, pw2, nullptr, DV_PREC_BF16X3, "consumer ");
  return sc.run();
}

extern "C" int dv_op_linear_gn(const float* x, const float* w, const float* b, const float* gamma, const float* beta, int32_t B, int32_t T,
                               int32_t Tp, int32_t K, int32_t C, int32_t G, float eps, int32_t route, float* y, float* stats,
                               uint16_t* y_norm_hi, uint16_t* y_norm_lo, void* stream) {
  if (!x || !w || !gamma || !beta || !y || !y_norm_hi || !y_norm_lo || B <= 0 || T <= 0 || C <= 0 || G <= 0 || !(eps >= 0.f) || !std::isfinite(eps))
    return dv_fail(DV_ERR_INVALID, "dv_op_linear_gn: bad argument");
  if (route != DV_GN_STAT16 && route != DV_GN_SLAB && route != DV_GN_KSTAT16) return dv_fail(DV_ERR_INVALID, "dv_op_linear_gn: route %d is not one of DV_GN_*", route);
  if (K <= 0 || K % 32 != 0 || 2 * (size_t)K + 256 > DV_ZERO_PAGE_BYTES) return dv_fail(DV_ERR_INVALID, "dv_op_linear_gn: K = %d must be a multiple of 32 within one source tensor's width", K);
  if (Tp % 32 != 0 || T > Tp || T <= Tp - 32) return dv_fail(DV_ERR_INVALID, "dv_op_linear_gn: Tp = %d must be a multiple of 32 with Tp - 32 < T = %d <= Tp", Tp, T);
  if ((int64_t)B * Tp > INT32_MAX / 2048) return dv_fail(DV_ERR_INVALID, "dv_op_linear_gn: B * Tp = %lld rows are too many", (long long)B * Tp);
  if (C % G != 0 || G > 64 || C / G > 512) return dv_fail(DV_ERR_INVALID, "dv_op_linear_gn: C = %d, G = %d: at most 64 groups of at most 512 channels", C, G);
  if (route == DV_GN_SLAB ? (C / G) % 4 != 0 : (C / G) % 16 != 0)
    return dv_fail(DV_ERR_INVALID, "dv_op_linear_gn: %d channels per group: block statistics need whole 16-channel blocks, the column slab multiples of 4", C / G);
  // the column slab's consumer and the standalone k_stat16 have no padded-row form (launch_gn_apply, launch_stat16)
  if (route != DV_GN_STAT16 && T != Tp) return dv_fail(DV_ERR_INVALID, "dv_op_linear_gn: this route has no padded-row form: T = %d must equal Tp = %d", T, Tp);
  OpScratch sc("dv_op_linear_gn", stream);
  if (int rc = sc.start()) return rc;
  const int M = B * Tp;
  const size_t nstat = route == DV_GN_SLAB ? (size_t)(M / 32) * C * 2 : (size_t)(M / 32) * (C / 16) * 2;
  const Planes a = sc.split(x, (size_t)M * K);
  const PackedW3 pw = sc.weights(C, K);
  sc.pack(pw, w, 0, K, 1, K);
  float* sbuf = stats ? stats : sc.get<float>(nstat * 4);
  GemmParams g = row_gemm_params(B, Tp, C, nullptr);
  g.seg[0] = seg1(a.hi, a.lo, K, 1, 0);
  g.Tv_in = g.Tv_out = g.T_virt = T;
  g.out = y;
  if (route == DV_GN_STAT16) g.stats16 = sbuf;
  if (route == DV_GN_SLAB) g.stats = sbuf;
  sc.gemm(g, pw, b, DV_PREC_BF16X3);
  if (route == DV_GN_KSTAT16) sc.op("k_stat16 ", [=](hipStream_t s) { return launch_stat16(y, sbuf, M, C, s); });
  GnApplyParams gp{};
  gp.a0 = y; gp.c0 = C;
  if (route == DV_GN_SLAB) gp.slab0 = sbuf; else gp.st16_0 = sbuf;
  gp.gamma = gamma; gp.beta = beta; gp.eps = eps; gp.groups = G;
  gp.out_hi = y_norm_hi; gp.out_lo = y_norm_lo; gp.B = B; gp.T = Tp; gp.Tv = T;
  char stage[96];   // (k_gn_apply refuses what its route cannot run: the failure names the shape)
  snprintf(stage, sizeof(stage), "k_gn_apply of C = %d, G = %d, T = %d, Tp = %d on this route: ", C, G, T, Tp);
  sc.op(stage, [=](hipStream_t s) { return launch_gn_apply(gp, s); });
  return sc.run();
}
