"""k_gemm through dv_op_gemm: the case list, the host emulation of its arithmetic, the bounds and the assertions (CPU side; the GPU
runs are tests/test_gpu_gemm_ops.py, what the bounds can and cannot see is tests/test_gemm_reference.py + tools/gemm_reference.py).

The kernel multiplies operands that were split into bf16 planes (hi = bf16_rne(v), lo = bf16_rne(v - hi)) on MFMAs whose products
are exact and whose sums are float32:

  emulation   the fp64 sum of exactly the plane products the kernel forms - bf16x3: hi.hi + hi.lo + lo.hi (P = 3 products per
              k), bf16: hi.hi (P = 1) - with bias, residual, ReLU, row mask and GEGLU applied in fp64 afterwards
  reference   the plain fp64 result on the fp32 inputs
  cpu32       a CPU float32 accumulation of the same products in k order, 16 products per step (one MFMA k-step), the epilogue in
              float32: reference-side arithmetic, the yardstick of the per-row criterion

Criteria (check()):
  element   |y - emu| <= 2 P K 2^-24 sum_k |x_k||w_k| + 2^-23 |emu|.  P K 2^-24 sum|x||w| bounds ANY float32 summation order of the
            P K exact products (gamma_n with n = P K, first order); doubled because the MFMA's internal accumulation rounding is not
            documented; 2^-23 |emu| is one ulp for the epilogue's additions.  GEGLU propagates the two pre-activations' bounds
            through value * gelu(gate) (|gelu'| <= 1.13) and adds gelu_erf's own error: Abramowitz-Stegun 7.1.26, |erf error| <=
            1.5e-7, plus at most eight float32 roundings of O(1) terms in its evaluation: 0.5 |g| (1.5e-7 + 8 x 2^-24) < 4e-7 |g|.
            Derived, not measured.  Cases with K > 320 skip it (the split-K cases: per-row and tile agreement only).
  row       frame_errors(y, emu).worst <= 4 x frame_errors(cpu32, emu).worst: the factor allows for the kernel's different cut of
            the sum into k-groups and slices
  ref       bf16x3: whole-tensor rel-L2 against the reference < 1e-4 (the project's bound).  bf16: <= 2 x the emulation's own
            distance from the reference + ||element bound|| / ||ref|| - the second term is what the element criterion already
            allows on top (triangle inequality) and is all there is where the operands are exact in bf16 (distance 0)
  agreement every tile that can run a shape agrees with the heuristic's tile inside the sum of both element bounds (= 2 x)
"""
import numpy as np
import torch

from diff_vits_amd import synth
from parity_metrics import frame_errors

F32, F64 = np.float32, np.float64
SEED = 4242

# ---- the menu kernels_gemm.hip builds (Tiles<32>, Tiles<64>): name -> (BM, BN, k-groups at BK = 32, at BK = 64 or None, GEGLU) ----
# T0 / T0S are compiled 32 deep only; T2 at BK = 32 is the same template instance as T2S (one k-group) but a menu entry of its own.
TILE_ID = {"T0": 1, "T1": 2, "T2": 3, "T2S": 4, "T2G": 5, "T3": 6, "T4": 7, "T4G": 8, "T0S": 9}
BK64 = 0x100
TILES = {
    "T0": (128, 128, 2, None, True), "T0S": (128, 128, 1, None, True), "T1": (128, 64, 1, 2, True), "T2": (64, 64, 1, 2, False),
    "T2S": (64, 64, 1, 1, False), "T2G": (64, 64, 1, 1, True), "T3": (64, 32, 1, 2, False), "T4": (32, 32, 1, 2, False),
    "T4G": (32, 64, 1, 1, True),
}
STORE, RESIDUAL, GEGLU = 0, 1, 2
SPLITK_FUSED = 0x100


def variant_id(bm, bn, bk, kg):
    return bm | bn << 8 | bk << 16 | kg << 24


def menu():
    """{(variant id, tile id, NSPLIT)} of everything the library builds: 9 tiles at BK = 32, 7 at BK = 64, two operand modes."""
    out = set()
    for name, (bm, bn, kg32, kg64, _) in TILES.items():
        for ns in (3, 1):
            out.add((variant_id(bm, bn, 32, kg32), TILE_ID[name], ns))
            if kg64 is not None:
                out.add((variant_id(bm, bn, 64, kg64), TILE_ID[name], ns))
    return out


def tiles_for(case):
    """[(label, tile argument)] of every forced tile that can run the case (dv_op_gemm's rules), the heuristic first."""
    c0, c1 = (case["K0"], case["K"] - case["K0"]) if case["K0"] else (case["K"], 0)
    out = [("auto", 0)]
    for name, (_, _, _, kg64, geglu) in TILES.items():
        if case["epi"] == GEGLU and not geglu:
            continue
        out.append((name, TILE_ID[name]))
        if kg64 is not None and c0 % 64 == 0 and c1 % 64 == 0:
            out.append((name + "x64", TILE_ID[name] | BK64))
    return out


# ---- cases ----
def _case(name, M, N, K, K0=0, epi=STORE, relu=0, mask=False, ldo=None, ldres=0, splitk=0, values="unit", bias=True):
    n_out = N // 2 if epi == GEGLU else N
    return dict(name=name, M=M, N=N, K=K, K0=K0, epi=epi, relu=relu, mask=mask, ldo=ldo or n_out, ldres=ldres, splitk=splitk,
                values=values, bias=bias)


# M in {1, BM - 1, BM + 1, 2 BM + 3} and N in {8, 17, BN + 1, 2 BN} for BM, BN in {32, 64, 128}; K in {32, 64, 96, 192, 320}: one
# k-tile, an odd k-tile count over two k-groups (192 at BK = 64), BK = 32 forced where 64 is allowed.  Every runnable tile runs every
# shape, so each (tile, BK) sees at least three combinations that straddle ITS tile.
SHAPES = [
    (1, 8, 32), (31, 33, 64), (33, 17, 96), (67, 64, 192), (33, 65, 320), (67, 128, 64),        # BM = 32 (T4, T4G)
    (63, 8, 64), (65, 65, 192), (131, 128, 320), (63, 33, 96), (131, 64, 32),                    # BM = 64 (T2, T2S, T2G, T3)
    (127, 17, 320), (129, 129, 96), (259, 256, 64), (129, 65, 192), (259, 128, 32), (1, 256, 192),   # BM = 128 (T0, T0S, T1)
]
CASES = [_case("plain.%dx%dx%d" % s, *s) for s in SHAPES]
CASES += [
    # no bias (the zero page as the bias source), output pitch beyond N
    _case("nobias.65x33x64", 65, 33, 64, bias=False, ldo=40),
    # residual with ldres != N: 16-byte loads (pitches % 4 == 0), the half-fragment epilogue (N a tile multiple), scalar loads
    _case("res.131x128x320", 131, 128, 320, epi=RESIDUAL, ldres=136),
    _case("res.63x33x96", 63, 33, 96, epi=RESIDUAL, ldres=37, ldo=35),
    _case("res.65x72x192", 65, 72, 192, epi=RESIDUAL, ldres=76, ldo=72),
    # ReLU, then the row mask, with rows that are zero
    _case("relumask.67x64x192", 67, 64, 192, relu=1, mask=True),
    _case("relumask.33x17x96", 33, 17, 96, relu=1, mask=True, epi=RESIDUAL, ldres=20),
    # two sources in one k-segment (K0 | K - K0): (64, 64) runs BK = 64 too, (32, 96) only BK = 32
    _case("k0.64+64", 67, 65, 128, K0=64),
    _case("k0.32+96", 67, 65, 128, K0=32),
    _case("k0.64+128.res", 129, 64, 192, K0=64, epi=RESIDUAL, ldres=64),
    # GEGLU on every tile with a 64-column block per wave; pitches: odd (scalar stores), % 4 (8-byte plane stores), aligned
    _case("geglu.67x128x64.odd", 67, 128, 64, epi=GEGLU, ldo=67),
    _case("geglu.33x192x96.p4", 33, 192, 96, epi=GEGLU, ldo=100),
    _case("geglu.129x256x192.al", 129, 256, 192, epi=GEGLU),
    # value edges on a mid-sized shape
    _case("offset30.65x65x192", 65, 65, 192, values="offset30"),
    _case("exact.65x65x192", 65, 65, 192, values="exact"),
    # one K = 1536 case per split-K form (per-row and agreement criteria only); the fused pair with a ragged last tile
    _case("splitk2.100x72x1536", 100, 72, 1536, splitk=2),
    _case("splitk3.100x72x1536", 100, 72, 1536, splitk=3, epi=RESIDUAL, ldres=72),
    _case("splitkf.130x100x1536", 130, 100, 1536, splitk=2 | SPLITK_FUSED, relu=1, mask=True),
]
CASE_NAMES = [c["name"] for c in CASES]
ELEMENT_MAX_K = 320


def case(name):
    return CASES[CASE_NAMES.index(name)]


def inputs(c):
    """x [M, K], w [N, K], bias [N] or None, res [M, ldres] or None, rowmask [M] or None (float32, deterministic)."""
    M, N, K = c["M"], c["N"], c["K"]
    tag = c["name"]
    x = synth.normal(SEED, tag + ".x", (M, K)).astype(F32)
    w = (synth.normal(SEED, tag + ".w", (N, K)) / np.sqrt(K)).astype(F32)
    if c["values"] == "offset30":           # a common offset of 30 sigma: the lo planes carry real weight
        x = (x + F32(30.0)).astype(F32)
        w = (w + F32(30.0 / np.sqrt(K))).astype(F32)
    if c["values"] == "exact":              # exactly representable in bf16: lo planes are zero
        x, w = bf16_rne(x).astype(F32), bf16_rne(w).astype(F32)
    b = (0.1 * synth.normal(SEED, tag + ".b", (N,))).astype(F32) if c["bias"] else None
    res = synth.normal(SEED, tag + ".r", (M, c["ldres"])).astype(F32) if c["epi"] == RESIDUAL else None
    mask = None
    if c["mask"]:
        mask = np.ones(M, dtype=F32)
        mask[[0, M - 1]] = 0
        mask[5:9] = 0
        mask[M // 2] = 0.5
    return x, w, b, res, mask


# ---- bf16 planes ----
def bf16_rne(v):
    """float32 -> the nearest bf16 (ties to even), as float64."""
    t = torch.from_numpy(np.ascontiguousarray(v, dtype=F32))
    return t.to(torch.bfloat16).double().numpy()


def bf16_trunc(v):
    a = np.ascontiguousarray(v, dtype=F32).view(np.uint32) & np.uint32(0xffff0000)
    return a.view(F32).astype(F64)


def split(v, trunc=False):
    """(hi, lo) planes of float32 v as float64: hi = bf16(v), lo = bf16(v - hi) (v - hi is exact in float32)."""
    rnd = bf16_trunc if trunc else bf16_rne
    hi = rnd(v)
    lo = rnd((np.asarray(v, dtype=F64) - hi).astype(F32))
    return hi, lo


def terms(x, w, nsplit, fault=None):
    """[(A [M, K], B [N, K])] plane pairs whose products the kernel sums, in the order it issues them per k-step."""
    xh, xl = split(x, fault == "trunc")
    wh, wl = split(w, fault == "trunc")
    if nsplit == 1:
        return [(xh, wh)]
    t = [(xl, wh), (xh, wl), (xh, wh)]       # w_hi x_lo, w_lo x_hi, w_hi x_hi
    return t[1:] if fault == "drop_lohi" else t


# ---- faults that re-route the k range (planted by tools/gemm_reference.py) ----
K_FAULTS = ("drop_last_ktile", "dup_ktile", "drop_kgroup_half", "src1_offset")


def _k_columns(c, bk, fault):
    """(columns of x, columns of w) the faulted kernel would multiply pairwise, in k order."""
    K, K0 = c["K"], c["K0"]
    kx = np.arange(K)
    kw = np.arange(K)
    nkt = K // bk
    if fault == "drop_last_ktile":
        kx, kw = kx[:K - bk], kw[:K - bk]
    elif fault == "dup_ktile":              # the middle k-tile added twice
        t = nkt // 2
        kx = np.concatenate([kx, kx[t * bk:(t + 1) * bk]]); kw = kx.copy()
    elif fault == "drop_kgroup_half":       # odd k-tile count: the second k-group's 32 columns of the last 64-deep tile
        if bk == 64 and nkt % 2 == 1:
            kx, kw = kx[:K - 32], kw[:K - 32]
    elif fault == "src1_offset":            # source 1 read from source 0's column offset: x column K0 + j comes from column j
        if K0:
            kx = np.concatenate([np.arange(K0), np.arange(K - K0) % K0])
    return kx, kw


def accumulate(c, x, w, nsplit, f32=False, fault=None, bk=64):
    """The [M, N] pre-epilogue sums: fp64 (the emulation), or float32 in k order, 16 products per step (cpu32)."""
    kx, kw = _k_columns(c, bk, fault) if fault in K_FAULTS else (np.arange(c["K"]), np.arange(c["K"]))
    tt = [(a[:, kx], b[:, kw]) for a, b in terms(x, w, nsplit, fault)]
    if not f32:
        return sum(a @ b.T for a, b in tt)
    acc = np.zeros((x.shape[0], w.shape[0]), dtype=F32)
    tt = [(a.astype(F32), b.astype(F32)) for a, b in tt]
    for s in range(0, len(kx), 16):
        for a, b in tt:
            part = np.zeros_like(acc)
            for k in range(s, min(s + 16, len(kx))):
                part += a[:, k, None] * b[None, :, k]         # exact products (8 x 8 significand bits), float32 additions
            acc += part
    return acc


def gelu(v):
    return 0.5 * v * (1.0 + torch.erf(torch.from_numpy(np.asarray(v, dtype=F64)) / np.sqrt(2.0)).numpy())


def epilogue(c, acc, b, res, mask, fault=None):
    """bias, residual, ReLU, row mask, GEGLU on the sums `acc`, in acc's own precision (fp64: the emulation; float32: cpu32)."""
    dt = acc.dtype
    N = c["N"]
    if fault == "mask_before_bias" and mask is not None:
        acc = acc * mask[:, None].astype(dt)
    v = acc + (b.astype(dt)[None, :] if b is not None else dt.type(0))
    if c["epi"] == GEGLU:
        a, g = v[:, :N // 2], v[:, N // 2:]
        if fault == "geglu_swap":
            a, g = g, a
        return (a * gelu(g).astype(dt)).astype(dt)
    if c["epi"] == RESIDUAL:
        v = v + res[:, :N].astype(dt)
    if c["relu"]:
        v = np.maximum(v, dt.type(0))
    if mask is not None and fault != "mask_before_bias":
        v = v * mask[:, None].astype(dt)
    return v


def element_bound(c, x, w, b, res, mask, nsplit, emu):
    """The element criterion's right-hand side (module docstring)."""
    K, N = c["K"], c["N"]
    mag = np.abs(x.astype(F64)) @ np.abs(w.astype(F64)).T
    acc_b = 2.0 * nsplit * K * 2.0 ** -24 * mag
    if c["epi"] != GEGLU:
        if mask is not None:
            acc_b = acc_b * np.abs(mask[:, None].astype(F64))
        return acc_b + 2.0 ** -23 * np.abs(emu)
    pre = accumulate(c, x, w, nsplit) + (b.astype(F64)[None, :] if b is not None else 0.0)
    a, g = pre[:, :N // 2], pre[:, N // 2:]
    ba = acc_b[:, :N // 2] + 2.0 ** -23 * np.abs(a)
    bg = acc_b[:, N // 2:] + 2.0 ** -23 * np.abs(g)
    dg = 1.13 * bg + 4e-7 * np.abs(g) + 2.0 ** -23 * np.abs(gelu(g))
    return ba * np.abs(gelu(g)) + np.abs(a) * dg + ba * dg + 2.0 ** -23 * np.abs(emu)


class Expected:
    """Everything of a (case, NSPLIT) that does not depend on the tile: computed once, shared by every tile's check."""
    _cache = {}

    def __init__(self, c, nsplit):
        x, w, b, res, mask = inputs(c)
        self.case, self.nsplit = c, nsplit
        self.emu = epilogue(c, accumulate(c, x, w, nsplit), b, res, mask)
        one = dict(c, K0=0)
        self.ref = epilogue(c, x.astype(F64) @ w.astype(F64).T, b, res, mask)
        self.cpu32 = epilogue(c, accumulate(one, x, w, nsplit, f32=True), b, res, mask).astype(F64)
        self.bound = element_bound(c, x, w, b, res, mask, nsplit, self.emu)
        self.row_cpu = frame_errors(self.cpu32[None], self.emu[None])["worst"]
        nref = max(np.linalg.norm(self.ref), 1e-300)
        self.emu_ref = float(np.linalg.norm(self.emu - self.ref) / nref)
        self.ref_bound = 1e-4 if nsplit == 3 else 2.0 * self.emu_ref + float(np.linalg.norm(self.bound) / nref)

    @classmethod
    def of(cls, c, nsplit):
        key = (c["name"], nsplit)
        if key not in cls._cache:
            cls._cache[key] = cls(c, nsplit)
        return cls._cache[key]


def judge(exp, y):
    """{criterion: measured / allowed} of a result y [M, n_out] (fp64 or float32) against exp; <= 1 passes."""
    c = exp.case
    y = np.asarray(y, dtype=F64)
    out = {}
    if c["K"] <= ELEMENT_MAX_K:
        d = np.abs(y - exp.emu)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(d > 0, d / exp.bound, 0.0)
        out["element"] = float(r.max())
    row = frame_errors(y[None], exp.emu[None])["worst"]
    out["row"] = float(row / exp.row_cpu) / 4.0 if exp.row_cpu > 0 else (0.0 if row == 0 else np.inf)
    if c["K"] <= ELEMENT_MAX_K:
        err = float(np.linalg.norm(y - exp.ref) / max(np.linalg.norm(exp.ref), 1e-300))
        out["ref"] = err / exp.ref_bound
    return out


def check(tag, exp, y, figs=None):
    """Asserts every criterion of judge(); prints the figures first.  Returns them."""
    assert np.isfinite(y).all(), tag + ": non-finite result"
    j = judge(exp, y)
    row = frame_errors(np.asarray(y, dtype=F64)[None], exp.emu[None])["worst"]
    print("gemm_ops %-44s element/bound %-9s row %.3e cpu32 row %.3e (x%.2f) ref/bound %s" % (
        tag, "%.3f" % j["element"] if "element" in j else "-", row, exp.row_cpu, 4.0 * j["row"],
        "%.3f" % j["ref"] if "ref" in j else "-"))
    if figs is not None:
        figs[tag] = j
    for k, v in j.items():
        assert v <= 1.0, "%s: %s criterion at %.3f of its bound" % (tag, k, v)
    return j


def check_agreement(tag, exp, y, y_auto):
    """A forced tile against the heuristic's tile on the same shape: inside the sum of both element bounds."""
    d = np.abs(np.asarray(y, dtype=F64) - np.asarray(y_auto, dtype=F64))
    r = float((d / np.maximum(2.0 * exp.bound, 1e-300)).max())
    assert r <= 1.0, "%s: differs from the heuristic's tile by %.3f of the two element bounds" % (tag, r)
    return r


def planes_of(y):
    """(hi, lo) uint16 bit patterns of the split of float32 y, round to nearest even (v_cvt_pk_bf16_f32)."""
    t = torch.from_numpy(np.ascontiguousarray(y, dtype=F32))
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    return hi.view(torch.int16).numpy().view(np.uint16), lo.view(torch.int16).numpy().view(np.uint16)


# (fault, NSPLIT) -> (case, BK, criterion) where tools/gemm_reference.py first sees each planted fault; kept by tests/test_gemm_reference.py
FIRST_SEEN = {
    ('drop_lohi', 3): ('plain.1x8x32', 32, 'row'),
    ('trunc', 3): ('plain.1x8x32', 32, 'row'),
    ('trunc', 1): ('plain.1x8x32', 32, 'row'),
    ('drop_last_ktile', 3): ('plain.1x8x32', 32, 'row'),
    ('drop_last_ktile', 1): ('plain.1x8x32', 32, 'row'),
    ('dup_ktile', 3): ('plain.1x8x32', 32, 'row'),
    ('dup_ktile', 1): ('plain.1x8x32', 32, 'row'),
    ('drop_kgroup_half', 3): ('plain.31x33x64', 64, 'row'),
    ('drop_kgroup_half', 1): ('plain.31x33x64', 64, 'row'),
    ('src1_offset', 3): ('k0.64+64', 32, 'row'),
    ('src1_offset', 1): ('k0.64+64', 32, 'row'),
    ('mask_before_bias', 3): ('relumask.67x64x192', 32, 'element'),
    ('mask_before_bias', 1): ('relumask.67x64x192', 32, 'element'),
    ('geglu_swap', 3): ('geglu.67x128x64.odd', 32, 'row'),
    ('geglu_swap', 1): ('geglu.67x128x64.odd', 32, 'row'),
}
