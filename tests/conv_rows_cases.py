"""k_gemm's convolution operand path through dv_op_conv_rows: the case list, the fp64 restatement of the row gather (gemm_tile.h
prep_a / advance / utt_of), the emulation, the bounds and the assertions (CPU side; the GPU runs are tests/test_gpu_conv_rows.py,
what the criteria can and cannot see is tests/test_conv_rows_reference.py).

The gather adds no arithmetic: a launch is the GEMM  y[(b, t), n] = sum_k X[(b, t), k] W[n, k] + bias[n]  on the rows
  X[(b, t), j (c0 + c1) + c] = [x0 | x1][b, src(t stride + j - pad), c]   (0 where t stride + j - pad is outside [0, T_virt))
  X[(b, t), taps (c0 + c1) + c] = x_sc[b, t, c]                           (the second k-segment: stride 1, no upsampling)
  src(ts) = ts | ts >> 1 (x2) | min(floor((float)ts * ((float)T / (float)U)), T - 1) (to U frames: ATen's float rule)
so gemm_cases.py's emulation (the fp64 sum of the plane products), its element bound with K = taps (c0 + c1) + c_sc, its cpu32
route and check() apply unchanged to the rows that exist.  On top of them, per case:
  padding   output rows [Tv_out, Tp_out) of every utterance are exactly zero
  frames    frame_errors(...).worst on every frame <= 4 x the cpu32 route's (check()'s row criterion IS per frame here: one row is
            one frame); the first frame, the last frame and the frames at tile seams are printed apart
  stats16   the words are (sum, M2 = squared deviations about the block's own mean) of the valid rows of a 32 x 16 block, n = 16 x
            rows values v.  Against fp64 on the emulation: |sum - S| <= u + E with u = 32 x 2^-24 sum|v| (any float32 order of n <= 512
            additions, first order, as the element bound counts them) and E = the block's element bounds summed.  The second word
            is compared as the sum of squares Q = M2 + sum^2 / n (formed in fp64 from the two words): M2 about a mean that is off by
            d = dS / n is M2_true + n d^2, so Q is off by 2 |S| dS / n + 2 dS^2 / n with dS <= u, plus 32 x 2^-24 sum v^2 for the
            float32 sum of the squared deviations, plus the element bounds carried through v^2: sum (2 |v| e + e^2).
            (dv_op_conv_rows gives stats16 only with Tp_out = Tv_out rounded up to 32, as launch_gemm demands: no block lies wholly
            in padding.)
Input rows [T, Tp_in) hold finite garbage of 3e4 sigma and 32 rows of NaN lie behind the last utterance (the entry puts them behind
every operand plane); the emulation sees the same rows, so a planted fault that reads them shows what the kernel would show."""
import numpy as np
import torch
import torch.nn.functional as F

import gemm_cases as gc
from diff_vits_amd import synth
from parity_metrics import frame_errors

F32, F64 = np.float32, np.float64
SEED = 5151
B = 3
UP_NONE, UP_X2, UP_SIZE = 0, 1, 2
GUARD = 32                      # rows of NaN behind the last utterance (dv_op_conv_rows: CONV_ROWS_GUARD)
# (T, U) where ATen's float rule and the exact rational t * T // U pick different source frames
FLOAT_RULE_PAIRS = [(14, 46), (26, 44), (39, 66), (30, 58), (21, 69)]


def rup(v, m):
    return (v + m - 1) // m * m


def _case(name, T, c0, Cout, Tp_in=None, c1=0, c_sc=0, taps=3, stride=1, up=UP_NONE, up_T=0, Tp_out=None, values="unit", bias=True,
          all_tiles=False):
    pad = (taps - 1) // 2
    T_virt = 2 * T if up == UP_X2 else (up_T if up == UP_SIZE else T)
    Tv_out = (T_virt + 2 * pad - taps) // stride + 1
    Tp_out = rup(Tv_out, 32) if Tp_out is None else Tp_out
    Tp_in = rup(T, 32) if Tp_in is None else Tp_in
    stats = Cout % 16 == 0 and Tp_out == rup(Tv_out, 32)
    return dict(name=name, B=B, T=T, Tp_in=Tp_in, c0=c0, c1=c1, c_sc=c_sc, Cout=Cout, taps=taps, pad=pad, stride=stride, up=up, up_T=up_T,
                T_virt=T_virt, Tv_out=Tv_out, Tp_out=Tp_out, K=taps * (c0 + c1) + c_sc, values=values, bias=bias, stats=stats,
                all_tiles=all_tiles)


CASES = [
    # ---- stride 2, three taps (Downsample2D): odd T puts the last output's right tap on T_virt, even T does not ----
    _case("s2.T1", 1, 32, 16, stride=2),
    _case("s2.T2", 2, 32, 16, Tp_in=2, stride=2),
    _case("s2.T3", 3, 64, 16, stride=2),
    _case("s2.T31", 31, 64, 80, Tp_in=31, Tp_out=16, stride=2),
    _case("s2.T32", 32, 96, 144, Tp_in=64, stride=2),
    _case("s2.T33.64|32", 33, 64, 80, c1=32, all_tiles=True, stride=2),
    _case("s2.T63.32|64", 63, 32, 16, c1=64, stride=2),
    _case("s2.T65", 65, 64, 80, all_tiles=True, stride=2),
    _case("s2.T75", 75, 96, 144, stride=2),
    # ---- nearest upsampling to a size (the size-forced Upsample2D), the float-rule pairs among them ----
    _case("up.19-37", 19, 32, 16, up=UP_SIZE, up_T=37),
    _case("up.38-75", 38, 64, 80, up=UP_SIZE, up_T=75, all_tiles=True),
    _case("up.5-9", 5, 32, 16, up=UP_SIZE, up_T=9, Tp_in=5, Tp_out=9),
] + [
    _case("up.%d-%d" % p, p[0], 32, 16, up=UP_SIZE, up_T=p[1]) for p in FLOAT_RULE_PAIRS
] + [
    # ---- x2 on k_gemm at a channel count k_conv3u refuses ----
    _case("x2.20-40.C96", 20, 96, 80, up=UP_X2),
    # ---- stride 1, three taps: the unpadded row space (pitch T), T rounded up to 32, one more block of padding ----
    _case("s1.T1.p1", 1, 32, 16, Tp_in=1, Tp_out=1),
    _case("s1.T1.p32", 1, 32, 16),
    _case("s1.T1.p64", 1, 32, 16, Tp_in=64),
    _case("s1.T31.p31", 31, 32, 16, Tp_in=31, Tp_out=31),
    _case("s1.T31.p32.32|64", 31, 32, 80, c1=64),
    _case("s1.T31.p64", 31, 64, 16, Tp_in=64),
    _case("s1.T33.p33", 33, 32, 16, Tp_in=33, Tp_out=33),
    _case("s1.T33.p64.64|32", 33, 64, 144, c1=32),
    _case("s1.T33.p96", 33, 96, 16, Tp_in=96),
    _case("s1.T65.p65", 65, 32, 80, Tp_in=65, Tp_out=65),
    _case("s1.T65.p96.sc32", 65, 64, 80, c_sc=32),
    _case("s1.T65.p128", 65, 32, 16, Tp_in=128),
    # ---- two sources at widths that run 64-deep k-tiles too (K <= 320: one tap), the second k-segment, Cout = 17, no bias ----
    _case("s1.T65.64|64.k1", 65, 64, 80, c1=64, taps=1, all_tiles=True),
    _case("s1.T33.C96.sc32", 33, 96, 144, c_sc=32),
    _case("s1.T33.N17", 33, 32, 17, Tp_out=37),
    _case("s2.T33.nobias", 33, 32, 16, bias=False, stride=2),
    # ---- value edges on a stride-2 shape; one frame 1e3 x louder than its neighbours in the unpadded row space ----
    _case("s2.T33.offset30", 33, 64, 80, values="offset30", stride=2),
    _case("s2.T33.exact", 33, 64, 80, values="exact", stride=2),
    _case("s1.T31.p31.loud", 31, 32, 16, Tp_in=31, Tp_out=31, values="loud"),
    _case("s2.T32.p32.loud", 32, 32, 16, values="loud", stride=2),
]
CASE_NAMES = [c["name"] for c in CASES]
assert len(set(CASE_NAMES)) == len(CASES) and all(c["K"] <= gc.ELEMENT_MAX_K for c in CASES)
# Not in the list: conv_in's Cin = 80 packed to 96.  dv_op_conv_rows takes sources whose widths are k-tile multiples and packs the
# weights at that width; the forward's zero-padded weight columns come from its own input packer, which this entry does not run.


def case(name):
    return CASES[CASE_NAMES.index(name)]


def mode_of(c):
    """The profile's mode labels of a case (a case can carry several)."""
    m = []
    if c["stride"] == 2:
        m.append("stride2")
    if c["up"] == UP_SIZE:
        m.append("size")
    if c["up"] == UP_X2:
        m.append("x2")
    if c["c1"]:
        m.append("two-source")
    if c["c_sc"]:
        m.append("segment2")
    return m or ["stride1"]


def tiles_for(c, candidates=()):
    """[(label, tile argument)]: the heuristic, the forced tiles the tuner would try on this launch (`candidates`: DV_GT_* values from
    dv_op_conv_rows_variant), and - all_tiles - every menu entry that can run the widths (dv_op_gemm's rules)."""
    widths = [w for w in (c["c0"], c["c1"], c["c_sc"]) if w]
    out = [("auto", 0)]
    names = {v: k for k, v in gc.TILE_ID.items()}
    for t in candidates:
        out.append((names[t & 0xff] + ("x64" if t & gc.BK64 else ""), t))
    if c["all_tiles"]:
        for name, (_, _, _, kg64, _) in gc.TILES.items():
            out.append((name, gc.TILE_ID[name]))
            if kg64 is not None and all(w % 64 == 0 for w in widths):
                out.append((name + "x64", gc.TILE_ID[name] | gc.BK64))
    seen, uniq = set(), []
    for label, t in out:
        if t not in seen:
            seen.add(t)
            uniq.append((label, t))
    return uniq


# ---- inputs ----
def inputs(c):
    """x0 [B, Tp_in, c0], x1 or None, w [Cout, c0 + c1, taps], bias or None, x_sc or None, w_sc [Cout, c_sc, 1] or None (float32)."""
    tag, T, Tp = c["name"], c["T"], c["Tp_in"]
    rng = np.random.default_rng(7)
    cin = c["c0"] + c["c1"]

    def src(name, C):
        a = np.empty((B, Tp, C), dtype=F32)
        a[:, :T] = synth.normal(SEED, tag + name, (B, T, C)).astype(F32)
        if c["values"] == "offset30":
            a[:, :T] += F32(30.0)
        if c["values"] == "exact":
            a[:, :T] = gc.bf16_rne(a[:, :T]).astype(F32)
        if c["values"] == "loud":               # the last frame of utterance 0 and the first of utterance 2: neighbours of utterance 1
            a[0, T - 1] *= F32(1e3)
            a[2, 0] *= F32(1e3)
        a[:, T:] = (3.0e4 * rng.standard_normal((B, Tp - T, C))).astype(F32)
        return a

    def wt(name, C, taps):
        w = (synth.normal(SEED, tag + name, (c["Cout"], C, taps)) / np.sqrt(C * taps)).astype(F32)
        if c["values"] == "offset30":
            w = (w + F32(30.0 / np.sqrt(C * taps))).astype(F32)
        if c["values"] == "exact":
            w = gc.bf16_rne(w).astype(F32)
        return w

    x0 = src(".x0", c["c0"])
    x1 = src(".x1", c["c1"]) if c["c1"] else None
    w = wt(".w", cin, c["taps"])
    b = (0.1 * synth.normal(SEED, tag + ".b", (c["Cout"],))).astype(F32) if c["bias"] else None
    xs = src(".xs", c["c_sc"]) if c["c_sc"] else None
    ws = wt(".ws", c["c_sc"], 1) if c["c_sc"] else None
    return x0, x1, w, b, xs, ws


# ---- the gather, restated ----
FAULTS = ("taps_reversed", "pad_plus_one", "s2_last_right_reads_T", "left_tap_prev_utt", "nearest_rational", "no_clamp", "a0_a1_swapped",
          "seg2_strided", "out_pad_not_zeroed", "utt_off_by_one", "Tp_in_bounds")


def nearest_index(ts, T, U, fault=None):
    """Source frame of virtual frame ts of a nearest upsampling T -> U: ATen's float rule, in float32 as the kernel computes it."""
    ts = np.asarray(ts, dtype=np.int64)
    if fault == "nearest_rational":
        return np.minimum(ts * T // U, T - 1)
    scale = F32(T) / F32(U)
    st = np.floor(ts.astype(F32) * scale).astype(np.int64)
    return st if fault == "no_clamp" else np.minimum(st, T - 1)


def rows_of(c, x0, x1, xs, fault=None):
    """X [B, Tp_out, K] float32: the operand rows of every output row (zeros for rows that do not exist - unless a fault reads them)."""
    T, Tp, taps, pad, stride = c["T"], c["Tp_in"], c["taps"], c["pad"], c["stride"]
    cat = x0 if x1 is None else np.concatenate([x1, x0] if fault == "a0_a1_swapped" else [x0, x1], -1)
    cin = cat.shape[-1]

    def flat(a):                                # [B * Tp_in + GUARD rows, C]: what lies behind an utterance is the next one, then NaN
        return np.concatenate([a.reshape(B * Tp, -1), np.full((GUARD, a.shape[-1]), np.nan, dtype=F32)], 0)

    fcat = flat(cat)
    X = np.zeros((B, c["Tp_out"], c["K"]), dtype=F32)
    t = np.arange(c["Tv_out"])
    if fault == "pad_plus_one":
        pad = pad + 1
    bound = Tp * (c["T_virt"] // T) if (fault == "Tp_in_bounds" and c["up"] != UP_SIZE) else c["T_virt"]
    for b in range(B):
        for j in range(taps):
            ts = t * stride + (taps - 1 - j if fault == "taps_reversed" else j) - pad
            ok = (ts >= 0) & (ts < bound)
            if fault == "s2_last_right_reads_T" and stride == 2:
                ok = ok | (ts == c["T_virt"])
            if fault == "left_tap_prev_utt" and b > 0:
                ok = ok | (ts == -1)
            st = ts >> 1 if c["up"] == UP_X2 else (nearest_index(np.maximum(ts, 0), T, c["up_T"], fault) if c["up"] == UP_SIZE else ts)
            st = np.where(ts < 0, ts, st)
            row = np.clip(b * Tp + st, 0, fcat.shape[0] - 1)
            X[b, :c["Tv_out"], j * cin:(j + 1) * cin] = np.where(ok[:, None], fcat[row], F32(0))
        if xs is not None:
            ts = t * (2 if fault == "seg2_strided" else 1)
            fx = flat(xs)
            X[b, :c["Tv_out"], taps * cin:] = np.where((ts < c["T_virt"])[:, None], fx[np.clip(b * Tp + ts, 0, fx.shape[0] - 1)], F32(0))
    return X


def weight_rows(c, w, ws):
    """W [Cout, K] in the kernel's k order: tap-major, [x0 | x1] channels inside a tap, the second segment behind."""
    W = np.transpose(w, (0, 2, 1)).reshape(c["Cout"], -1)
    return W if ws is None else np.concatenate([W, ws[:, :, 0]], 1)


def _gemm_case(c, M):
    return dict(name=c["name"], M=M, N=c["Cout"], K=c["K"], K0=0, epi=gc.STORE, relu=0, mask=False, splitk=0)


def result(c, nsplit, fault=None, f32=False):
    """The full output [B, Tp_out, Cout] of the emulation (fp64 sum of the plane products; f32: the cpu32 route), with a planted
    fault; padding rows are zero (a fault may fill them)."""
    x0, x1, w, b, xs, ws = inputs(c)
    X = rows_of(c, x0, x1, xs, fault)
    W = weight_rows(c, w, ws)
    g = _gemm_case(c, X.shape[0] * X.shape[1])
    y = gc.epilogue(g, gc.accumulate(g, X.reshape(-1, c["K"]), W, nsplit, f32=f32), b, None, None).astype(F64)
    y = y.reshape(B, c["Tp_out"], c["Cout"])
    if fault == "utt_off_by_one":               # row m = b T_out counted to utterance b - 1 as frame T_out: a row that does not exist
        y[1:, 0] = 0.0
    if fault != "out_pad_not_zeroed":
        y[:, c["Tv_out"]:] = 0.0
    return y


def reference(c):
    """fp64 on the fp32 inputs through torch's own operators: F.interpolate(mode="nearest") on the frames that exist (float32: ATen's
    float rule), F.conv1d, plus the 1x1 segment -> [B, Tv_out, Cout]."""
    x0, x1, w, b, xs, ws = inputs(c)
    T = c["T"]
    x = torch.from_numpy(x0[:, :T] if x1 is None else np.concatenate([x0[:, :T], x1[:, :T]], -1)).permute(0, 2, 1)
    if c["up"] == UP_X2:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    if c["up"] == UP_SIZE:
        x = F.interpolate(x, size=c["up_T"], mode="nearest")
    y = F.conv1d(x.double(), torch.from_numpy(w).double(), None if b is None else torch.from_numpy(b).double(), stride=c["stride"],
                 padding=c["pad"])
    if xs is not None:
        y = y + F.conv1d(torch.from_numpy(xs[:, :T]).double().permute(0, 2, 1), torch.from_numpy(ws).double())
    return y.permute(0, 2, 1).contiguous().numpy()


def restatement(c):
    """The same in fp64 through rows_of(): X W^T + bias on the rows that exist -> [B, Tv_out, Cout]."""
    x0, x1, w, b, xs, ws = inputs(c)
    X = rows_of(c, x0, x1, xs)[:, :c["Tv_out"]].astype(F64)
    y = X @ weight_rows(c, w, ws).astype(F64).T
    return y + (b.astype(F64) if b is not None else 0.0)


class Expected:
    """Everything of a (case, NSPLIT) that does not depend on the tile; has what gemm_cases.judge() / check() read."""
    _cache = {}

    def __init__(self, c, nsplit):
        x0, x1, w, b, xs, ws = inputs(c)
        Tv = c["Tv_out"]
        X = rows_of(c, x0, x1, xs)[:, :Tv].reshape(-1, c["K"])
        W = weight_rows(c, w, ws)
        self.conv, self.nsplit = c, nsplit
        self.case = g = _gemm_case(c, X.shape[0])
        self.emu = gc.epilogue(g, gc.accumulate(g, X, W, nsplit), b, None, None)
        self.ref = gc.epilogue(g, X.astype(F64) @ W.astype(F64).T, b, None, None)
        self.cpu32 = gc.epilogue(g, gc.accumulate(g, X, W, nsplit, f32=True), b, None, None).astype(F64)
        self.bound = gc.element_bound(g, X, W, b, None, None, nsplit, self.emu)
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


def block_words(c, y):
    """stats16 as the kernel lays it out, from a full output y [B, Tp_out, Cout]: [B * Tp_out / 32, Cout / 16, 2] float32 (sum, M2)."""
    Tv, Tp, N = c["Tv_out"], c["Tp_out"], c["Cout"]
    v = np.asarray(y, dtype=F64).reshape(B, Tp // 32, 32, N // 16, 16)
    ok = (np.arange(Tp).reshape(Tp // 32, 32) < Tv)[None, :, :, None, None]
    n = 16.0 * ok.sum(2, keepdims=True)
    s = np.where(ok, v, 0.0).sum((2, 4))
    mean = s[:, :, None, :, None] / n
    m2 = np.where(ok, (v - mean) ** 2, 0.0).sum((2, 4))
    return np.stack([s, m2], -1).reshape(B * Tp // 32, N // 16, 2).astype(F32)


def judge_stats(exp, words):
    """{"stats sum", "stats sumsq"}: measured / allowed of stats16 words [B * Tp_out / 32, Cout / 16, 2] (module docstring)."""
    c = exp.conv
    Tv, Tp, N = c["Tv_out"], c["Tp_out"], c["Cout"]

    def blocks(a):                              # [B, Tv, N] -> [B, Tp / 32, N / 16] sums over the rows that exist
        full = np.zeros((B, Tp, N))
        full[:, :Tv] = a.reshape(B, Tv, N)
        return full.reshape(B, Tp // 32, 32, N // 16, 16).sum((2, 4))

    n = 16.0 * np.minimum(32, Tv - 32 * np.arange(Tp // 32))[None, :, None]
    v, e = exp.emu, exp.bound
    S, Q = blocks(v), blocks(v * v)
    u = 32 * 2.0 ** -24 * blocks(np.abs(v))
    w = np.asarray(words, dtype=F64).reshape(B, Tp // 32, N // 16, 2)
    ds = u + blocks(e)
    dq = 2.0 * np.abs(S) * ds / n + 2.0 * ds * ds / n + 32 * 2.0 ** -24 * Q + blocks(2.0 * np.abs(v) * e + e * e)
    got_q = w[..., 1] + w[..., 0] ** 2 / n
    with np.errstate(invalid="ignore", divide="ignore"):
        rs = np.where(w[..., 0] == S, 0.0, np.abs(w[..., 0] - S) / ds)
        rq = np.where(got_q == Q, 0.0, np.abs(got_q - Q) / dq)
    return {"stats sum": float(np.nan_to_num(rs, nan=np.inf).max()), "stats sumsq": float(np.nan_to_num(rq, nan=np.inf).max())}


def seams(c, bm):
    """Frames (b, t) of [B, Tv_out] at the first / last row of a bm-row tile of the launch's row space (row m = b Tp_out + t)."""
    m = np.arange(B)[:, None] * c["Tp_out"] + np.arange(c["Tv_out"])[None, :]
    return (m % bm == 0) | (m % bm == bm - 1)


class Miss(AssertionError):
    pass


def check(tag, exp, y_full, words=None, bm=64, figs=None):
    """Every criterion of one result y_full [B, Tp_out, Cout] (and its stats16 words): raises Miss (an AssertionError) naming the
    criterion.  Returns {criterion: measured / allowed}."""
    c = exp.conv
    Tv = c["Tv_out"]
    y_full = np.asarray(y_full, dtype=F64)
    if not (y_full[:, Tv:] == 0).all():
        raise Miss("%s: padding criterion: output rows [Tv_out, Tp_out) are not exactly zero" % tag)
    y = y_full[:, :Tv]
    if not np.isfinite(y).all():
        raise Miss("%s: finite criterion: NaN or Inf in the frames that exist" % tag)
    fe = frame_errors(y, exp.emu.reshape(y.shape))
    per, sm = fe["per_frame"], seams(c, bm)
    sm[:, [0, Tv - 1]] = False
    inner = ~sm
    inner[:, [0, Tv - 1]] = False
    print("conv_rows %-40s frames: first %.2e last %.2e seams(%d) %.2e other %.2e worst %.2e at %s" % (
        tag, per[:, 0].max(), per[:, Tv - 1].max(), bm, per[sm].max() if sm.any() else 0.0, per[inner].max() if inner.any() else 0.0,
        fe["worst"], fe["at"]))
    try:
        j = gc.check(tag, exp, y.reshape(-1, c["Cout"]))
    except AssertionError as e:
        raise Miss(str(e))
    # (frames: per-frame worst against 4 x the cpu32 route's, over [B, Tv_out] frames - check()'s row criterion on the same rows)
    j["frames"] = j["row"]
    if words is not None:
        j.update(judge_stats(exp, words))
        print("conv_rows %-40s stats16 / bound: sum %.3f sum of squares %.3f" % (tag, j["stats sum"], j["stats sumsq"]))
        for k in ("stats sum", "stats sumsq"):
            if not j[k] <= 1.0:
                raise Miss("%s: %s criterion at %.3f of its bound" % (tag, k, j[k]))
    if figs is not None:
        figs[tag] = j
    return j
