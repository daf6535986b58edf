"""Value-edge cases, float32 emulations and the assertions of the normalisation ops (tests/test_gpu_norm_ops.py runs them on what the
GPU returned, tests/test_norm_reference.py and tools/norm_reference.py on emulations of the correct arithmetic and of planted
faults).  Plain helper module: no fixtures, no hooks.

Every comparison is against fp64 of the kernel's own fp32 INPUT to the normalisation (the y1 / y the producer GEMM returned), so the
split-bf16 contraction error never enters a statistics bound.

Bounds
  mean   |mean - mean64| <= (depth / 2 + 1) units, unit = sum over the kernel's blocks of ulp32(sum |x| of the block) / n: `depth` fp32
         additions on the longest path of the kernel's sum, half an ulp of a partial sum (<= sum |x|) each, + 1 for the division and the
         rounding of the word itself.  For same-signed data (the offset edges) the unit is the ulp of the mean.  DEPTH names the count
         per kernel as read from its code.
  rstd   1e-5 relative (tests/test_gpu_ops.py test_group_stats_value_edges).
  words  sum: the mean's bound on the block.  Squared deviations about the block's own mean, against fp64 of the same block:
         (depth + 4) 2^-24 relative (one rounding each for v - mb and its square, `depth` additions) + n (mean bound)^2 absolute (what
         the fp32 block mean's own error moves the sum of squares by).
  rows   every row within 2 x the worst row of the float32 emulation against fp64 on the same inputs (+ 2^-16 where the result leaves as
         two bf16 planes, tests/test_gpu_ops.py test_attention_frag's rule); row errors relative to max(row norm, 0.1 rms row norm),
         at most 1 % of the rows on that floor.  Constant rows (every normalised row is beta: no norm to divide by) absolutely.
         The emulation is of the documented arithmetic, which for a split-bf16 contraction means its three products (hi hi + hi lo +
         lo hi; lo lo is never formed - at a 300 sigma offset that term, not the statistic, is most of y2's error) and float32 sums.
         The row kernels at M = 1 and 5 are judged by the emulation's worst row over all M of the same C (check_rows pop_worst).
FIRST_SEEN: where each planted fault first exceeds its bound 5 x (tools/norm_reference.py).
"""
import numpy as np
import torch

from parity_metrics import FLOOR_FRACTION, MAX_FLOORED, _planes, ln_linear

SEED = 4242
F32, F64 = np.float32, np.float64
EDGES = ("unit", "offset30", "offset300", "constant", "outlier", "small-sigma")
GAMMAS = ("plain", "signs")
RSTD_REL = 1e-5
PLANES_REL = 2.0 ** -16
# fp32 additions on the longest path of each kernel's sum (k_ln_rows / k_ln_apply / k_ln_affine: a float4 pairwise = 2, 8 slots, 6
# butterfly steps; k_prompt_pre: 8 slots + 6; rowstat_out: 16 in-lane + 1 pair exchange; stats16 and k_stat16: 8 in-lane + 6 wave
# steps; the column slab: 5 butterfly steps + the shift's re-addition and its product)
DEPTH = {"ln_rows": 16, "prompt_pre": 14, "rowstat": 17, "stat16": 14, "slab": 7}
OFFSET_GRID = (30, 100, 300, 1000)
# (route, planted fault) -> the first point at which the route's assertions see it at >= 5 x the bound (tools/norm_reference.py,
# profiles/norm_reference.txt: offsets in grid order, then the other value edges).  Every point is a case of tests/test_gpu_norm_ops.py.
# No fault of the list stays out of reach.
FIRST_SEEN = {
    ("ln_rows", "var_e2"): "offset30", ("ln_rows", "no_eps"): "unit",
    ("prompt_pre", "var_e2"): "offset30", ("prompt_pre", "no_eps"): "small-sigma", ("prompt_pre", "mean_cpad"): "offset30",
    ("linear_ln", "var_e2"): "offset1000", ("linear_ln", "no_dm2"): "offset30", ("linear_ln", "no_eps"): "unit",
    ("gn_stat16", "var_e2"): "offset100", ("gn_stat16", "no_eps"): "small-sigma", ("gn_stat16", "pad32"): "offset30",
    ("gn_slab", "slab_fp32"): "offset100", ("gn_slab", "no_eps"): "small-sigma",
}


def _normal(name, shape):
    from diff_vits_amd import synth
    return synth.normal(SEED, name, shape)


def _dyadic(a, frac_bits=4, lim=7.9375):
    """Multiples of 2^-frac_bits within +-lim: at most 8 significant bits."""
    return (np.clip(np.round(a.astype(F64) * 2 ** frac_bits) / 2 ** frac_bits, -lim, lim)).astype(F32)


def affine(C, gamma="plain", dyadic=False, name="g"):
    """gamma, beta [C]: 1 + 0.1 n / 0.1 n, or ("signs") sign-alternating with one zero; dyadic: multiples of 1 / 16."""
    g = 1.0 + 0.1 * _normal(name + ".gamma", (C,)).astype(F64)
    b = 0.1 * _normal(name + ".beta", (C,)).astype(F64)
    if dyadic:
        g, b = _dyadic(g).astype(F64), _dyadic(b).astype(F64)
    if gamma == "signs":
        g = g * np.where(np.arange(C) % 2 == 0, 1.0, -1.0)
        g[C // 3] = 0.0
    return g.astype(F32), b.astype(F32)


def edge_values(edge, shape, name="x", dyadic=False, offset=None):
    """[..., n] float32: every slice along the last axis is one normalisation domain (a row) at the value edge `edge`.
    dyadic: unit draws are multiples of 1 / 16 up to 8 bits, offsets integers, the small sigma 2^-10 - exact in two bf16 planes."""
    z = _normal(name, shape)
    if dyadic:
        z = _dyadic(z)
    if edge == "unit":
        return z
    if edge.startswith("offset"):
        return (z.astype(F64) + float(offset if offset is not None else edge[6:])).astype(F32)
    if edge == "constant":
        return np.full(shape, 1.5, dtype=F32)
    if edge == "outlier":
        x = (z.astype(F64) + 0.75).astype(F32)
        flat = x.reshape(-1, shape[-1])
        flat[np.arange(flat.shape[0]), (np.arange(flat.shape[0]) * 7 + 3) % shape[-1]] = F32(1.0e4)
        return x
    if edge == "small-sigma":
        return (z.astype(F64) * (2.0 ** -10 if dyadic else 1e-3) + 0.5).astype(F32)
    raise KeyError(edge)


def group_values(edge, B, T, Tp, C, G, name="x", dyadic=False, offset=None):
    """[B, Tp, C] float32 whose (utterance, group) domains sit at `edge`; rows [T, Tp) hold finite junk.  "two-offsets": utterance 0
    at 30, utterance 1 at 300.  The outlier edge has ONE 1e4 value per (utterance, group)."""
    cg = C // G
    if edge == "two-offsets":
        x = np.concatenate([group_values("offset30", 1, T, Tp, C, G, name + ".0", dyadic),
                            group_values("offset300", 1, T, Tp, C, G, name + ".1", dyadic)], 0)
        return x
    if edge == "outlier":
        x = (edge_values("unit", (B, Tp, C), name, dyadic).astype(F64) + 0.75).astype(F32)
        for b in range(B):
            for g in range(G):
                x[b, (5 * g + 3 * b + 1) % T, g * cg + (3 * g + b) % cg] = F32(1.0e4)
    else:
        x = edge_values(edge, (B, Tp, C), name, dyadic, offset)
    x[:, T:, :] = F32(7.0)
    return x


# ---------------------------------------------------------------------------------------------------- fp64 references
def ln64(x, gamma=None, beta=None, eps=1e-5):
    """-> mean [M], rstd [M], y [M, C] in fp64 (gamma / beta None: no affine)."""
    x = np.asarray(x, dtype=F64)
    m = x.mean(-1)
    r = 1.0 / np.sqrt(x.var(-1) + eps)
    y = (x - m[..., None]) * r[..., None]
    if gamma is not None:
        y = y * np.asarray(gamma, F64) + np.asarray(beta, F64)
    return m, r, y


def gn64(y, T, G, gamma, beta, eps):
    """y [B, Tp, C] -> mean, rstd [B, G], normalised [B, Tp, C] in fp64 over the first T frames (the others: the same affine)."""
    y = np.asarray(y, dtype=F64)
    B, Tp, C = y.shape
    v = y[:, :T].reshape(B, T, G, C // G)
    m, r = v.mean((1, 3)), 1.0 / np.sqrt(v.var((1, 3)) + eps)
    a = np.repeat(r, C // G, 1) * np.asarray(gamma, F64)[None, :]
    sh = np.asarray(beta, F64)[None, :] - np.repeat(m, C // G, 1) * a
    return m, r, y * a[:, None, :] + sh[:, None, :]


# ---------------------------------------------------------------------------------------------------- float32 emulations
FAULTS = ("var_e2", "slab_fp32", "no_dm2", "no_eps", "mean_cpad", "pad32")


REVERSED = False   # the float32 sums of the emulations take their terms in reverse order: a second, independent rounding pattern of
                   # the same arithmetic at the same (pairwise) depth, which is also the depth class of the kernels' lane / wave trees.
                   # (A strictly left-to-right sum of 512 terms is no model of them: at an offset its mean error is 5 x the pairwise one.)


def _sum(a, axes=1):
    """float32 sum over the last `axes` axes."""
    a = np.asarray(a, dtype=F32)
    a = a.reshape(a.shape[:a.ndim - axes] + (-1,))
    return np.ascontiguousarray(a[..., ::-1]).sum(-1, dtype=F32) if REVERSED else a.sum(-1, dtype=F32)


def ln_emulate(x, gamma=None, beta=None, rowmask=None, eps=1e-5, fault=None, cpad=None, fma=False):
    """The row kernels in float32 (two passes: mean, centred variance; then (x - mean) * rstd [* gamma + beta] [* mask]).
    Faults: "var_e2" variance as E[x^2] - mean^2, "no_eps", "mean_cpad" the sums divided by cpad instead of C."""
    x = np.asarray(x, dtype=F32)
    C = x.shape[-1]
    n = F32(cpad if fault == "mean_cpad" else C)
    mu = _sum(x) / n
    if fault == "var_e2":
        var = np.maximum(_sum(x * x) / n - mu * mu, F32(0))
    else:
        d = x - mu[..., None]
        var = _sum(d * d) / n
    rs = F32(1) / np.sqrt(var + F32(0 if fault == "no_eps" else eps), dtype=F32)
    y = (x - mu[..., None]) * rs[..., None]
    if gamma is not None:
        g, b = np.asarray(gamma, F32), np.asarray(beta, F32)
        y = (y.astype(F64) * g + b).astype(F32) if fma else y * g + b
    if rowmask is not None:
        y = y * np.asarray(rowmask, F32)[..., None]
    return mu, rs, y.astype(F32)


def rowstat_emulate(y1):
    """[M, C] -> [M, C / 32, 2]: per 32-column block (sum, squared deviations from the block's own mean) in float32."""
    v = np.asarray(y1, dtype=F32).reshape(y1.shape[0], -1, 32)
    a = _sum(v)
    d = v - (a * F32(1 / 32.0))[..., None]
    return np.stack([a, _sum(d * d)], -1)


def rowstat_combine(rs, eps=1e-5, fault=None, y1=None):
    """The consumer's combination in float32 -> mean, rstd [M].  Faults: "no_dm2" the 32 dm^2 term dropped, "no_eps", "var_e2"
    (needs y1: the row's E[x^2] - mean^2 in float32)."""
    rs = np.asarray(rs, dtype=F32)
    nb = rs.shape[1]
    inv_c = F32(1.0) / F32(nb * 32)
    mean = _sum(rs[..., 0]) * inv_c
    dm = rs[..., 0] * F32(1 / 32.0) - mean[:, None]
    m2 = _sum(rs[..., 1] + (F32(0) if fault == "no_dm2" else F32(32) * dm * dm))
    var = m2 * inv_c
    if fault == "var_e2":
        x = np.asarray(y1, dtype=F32)
        var = np.maximum(_sum(x * x) * inv_c - mean * mean, F32(0))
    return mean, F32(1) / np.sqrt(var + F32(0 if fault == "no_eps" else eps), dtype=F32)


def _blocks(y, cols):
    """[B, Tp, C] -> [B, Tp / 32, C / cols, 32, cols]"""
    B, Tp, C = y.shape
    return np.asarray(y).reshape(B, Tp // 32, 32, C // cols, cols).transpose(0, 1, 3, 2, 4)


def _counts(T, Tp):
    return np.minimum(32, T - 32 * np.arange(Tp // 32)).astype(F64)


def block_words_emulate(y, T, cols, fault=None):
    """The producer's block statistics in float32: y [B, Tp, C] (rows [T, Tp) zero) -> [B, Tp / 32, C / cols, 2].  cols = 16: the
    32x16 blocks; cols = 1: the column slab.  (sum, squared deviations from the block's own mean over the rows that exist).
    Faults: "pad32" a partial block's mean and deviations taken over 32 rows; "slab_fp32" (sum, float32 sum of squares)."""
    B, Tp, C = y.shape
    v = _blocks(np.asarray(y, dtype=F32), cols)
    cnt = _counts(T, Tp)
    ok = (np.arange(32)[None, :] < cnt[:, None])[None, :, None, :, None]
    a = _sum(v, 2)
    if fault == "slab_fp32":
        return np.stack([a, _sum(v * v, 2)], -1)
    n = (np.full_like(cnt, 32.0) if fault == "pad32" else cnt) * cols
    mb = a / n.astype(F32)[None, :, None]
    d = np.where(ok | (fault == "pad32"), v - mb[..., None, None], F32(0)).astype(F32)
    return np.stack([a, _sum(d * d, 2)], -1)


def block_words_combine(words, T, Tp, G, cols, eps, fault=None):
    """k_gn_apply's reduction (fp64 on the fp32 words) -> mean, rstd [B, G] (rstd rounded to float32, as the kernel holds it).
    Faults: "pad32" every block counted as 32 rows; "slab_fp32" the words are (sum, sum of squares); "no_eps"; "var_e2" the sums of
    squares rounded to float32 before E[x^2] - mean^2."""
    w = np.asarray(words, dtype=F64)
    B, RB, NB, _ = w.shape
    cnt = (np.full(RB, 32.0) if fault == "pad32" else _counts(T, Tp))
    q = w[..., 1] if fault == "slab_fp32" else w[..., 1] + w[..., 0] ** 2 / (cols * cnt)[None, :, None]
    if fault == "var_e2":
        q = q.astype(F32).astype(F64)
    s1 = w[..., 0].reshape(B, RB, G, NB // G).sum((1, 3))
    q = q.reshape(B, RB, G, NB // G).sum((1, 3))
    if fault == "var_e2":
        q = q.astype(F32).astype(F64)
    n = (NB // G) * cols * cnt.sum()
    mean = s1 / n
    var = np.maximum(q / n - mean * mean, 0.0)
    return mean, (1.0 / np.sqrt(var + (0.0 if fault == "no_eps" else eps))).astype(F32).astype(F64)


def gn_apply_emulate(y, mean, rstd, gamma, beta):
    """k_gn_apply's affine in float32: a = rstd gamma, shift = beta - float(mean) a, out = fma(y, a, shift) -> [B, Tp, C]."""
    B, Tp, C = y.shape
    cg = C // mean.shape[1]
    a = np.repeat(np.asarray(rstd, F32), cg, 1) * np.asarray(gamma, F32)[None, :]
    sh = np.asarray(beta, F32)[None, :] - np.repeat(np.asarray(mean).astype(F32), cg, 1) * a
    return (np.asarray(y, F32).astype(F64) * a[:, None, :] + sh[:, None, :].astype(F64)).astype(F32)


def planes(v):
    """What two bf16 planes hold of a float32 array, as fp64."""
    return _planes(torch.from_numpy(np.ascontiguousarray(v, dtype=F32))).numpy()


def from_planes(hi, lo):
    """uint16 bit patterns of the hi / lo bf16 planes (numpy) -> fp64 value hi + lo."""
    def f(b):
        return (np.asarray(b).astype(np.uint32) << 16).view(F32).astype(F64)
    return f(hi) + (0.0 if lo is None else f(lo))


def linear_ln_emulate(y1, gamma, beta, w2, b2, fused=True, fault=None, eps=1e-5):
    """y2 as the two routes compute it from the fp32 y1: fused - parity_metrics.ln_linear's folded form with the statistics the
    consumer combines from float32 partials, float32 accumulation; unfused - k_ln_apply's planes times the folded weights."""
    t = lambda a: None if a is None else torch.from_numpy(np.asarray(a, dtype=F64))
    if fused:
        st = rowstat_combine(rowstat_emulate(y1), eps, fault, y1)
        return ln_linear(t(y1), t(gamma), t(beta), t(w2), t(b2), emulate=True, eps=eps, stats=st, acc32=True).numpy()
    _, _, n = ln_emulate(y1, eps=eps, fault=fault)
    wf = (np.asarray(w2, F64) * np.asarray(gamma, F64)[None, :]).astype(F32)
    bf = (np.asarray(w2, F64) @ np.asarray(beta, F64) + (0.0 if b2 is None else np.asarray(b2, F64))).astype(F32)
    hi = lambda a: _planes(torch.from_numpy(np.ascontiguousarray(a, dtype=F32)), lo=False).numpy().astype(F32)
    nh, wh = hi(n), hi(wf)
    nl, wl = hi(n - nh), hi(wf - wh)
    return (nh @ wh.T + nh @ wl.T + nl @ wh.T + bf).astype(F64)     # the split-bf16 contraction's three products, float32 sums


def linear_ln64(y1, gamma, beta, w2, b2, eps=1e-5):
    _, _, n = ln64(y1, gamma, beta, eps)
    return n @ np.asarray(w2, F64).T + (0.0 if b2 is None else np.asarray(b2, F64))


# ---------------------------------------------------------------------------------------------------- operands
def permutation(C, name="perm"):
    """A fixed-point-free permutation of C columns that also moves columns across 32-column blocks: w [C, C] with w[n, p[n]] = 1."""
    p = (np.arange(C) * 37 + 45) % C if C % 37 else (np.arange(C) * 41 + 45) % C
    assert len(set(p.tolist())) == C
    w = np.zeros((C, C), dtype=F32)
    w[np.arange(C), p] = 1.0
    return p, w


def producer(C, exact, name="w1"):
    """-> p, w1 [C, C], b1 [C] or None: the permutation alone (exact) or with 2^-6-scale noise and a bias."""
    p, w = permutation(C)
    if exact:
        return p, w, None
    return p, (w + _normal(name, (C, C)) * F32(2.0 ** -6 / np.sqrt(C))).astype(F32), (0.1 * _normal(name + ".b", (C,))).astype(F32)


def consumer(N, C, exact, name="w2"):
    w = _normal(name, (N, C)).astype(F64) / (1.0 if exact else np.sqrt(C))
    b = 0.1 * _normal(name + ".b", (N,))
    if exact:
        return _dyadic(w), _dyadic(b)
    return w.astype(F32), b.astype(F32)


# ---------------------------------------------------------------------------------------------------- assertions
class Miss(AssertionError):
    pass


def mean_units(got, x_blocks):
    """|got - mean64| in the unit of the module docstring.  x_blocks [..., nblk, n_in_block] fp64: the kernel's input per block."""
    xb = np.asarray(x_blocks, dtype=F64)
    n = xb.shape[-1] * xb.shape[-2]
    unit = np.spacing(np.abs(xb).sum(-1).astype(F32)).astype(F64).sum(-1) / n
    return np.abs(np.asarray(got, F64) - xb.mean((-1, -2))) / np.maximum(unit, 1e-300)


def check_stats(what, mean, rstd, x_blocks, eps, depth, figs=None):
    """mean within depth / 2 + 1 units, rstd within 1e-5 relative of fp64 over the same values."""
    xb = np.asarray(x_blocks, dtype=F64)
    flat = xb.reshape(xb.shape[:-2] + (-1,))
    want = 1.0 / np.sqrt(flat.var(-1) + eps)
    em = float(mean_units(mean, xb).max())
    er = float((np.abs(np.asarray(rstd, F64) - want) / want).max())
    if figs is not None:
        figs[what + " mean units"] = em
        figs[what + " rstd rel"] = er
    if em > depth / 2 + 1:
        raise Miss("%s: mean off by %.2f units (bound %.1f)" % (what, em, depth / 2 + 1))
    if not er <= RSTD_REL:
        raise Miss("%s: rstd off by %.3e relative (bound %.0e)" % (what, er, RSTD_REL))


def check_group_stats(what, mean, rstd, y, T, G, cols, eps, depth, figs=None):
    """Group mean / rstd [B, G] (recombined from block words of `cols` columns) against fp64 of y [B, Tp, C]'s first T frames."""
    y = np.asarray(y, dtype=F64)
    B, Tp, C = y.shape
    v = np.abs(y).copy()
    v[:, T:] = 0.0
    unit = np.spacing(_blocks(v, cols).sum((-1, -2)).astype(F32)).astype(F64)            # [B, RB, C / cols]
    unit = unit.reshape(B, Tp // 32, G, -1).sum((1, 3)) / (T * (C // G))
    grp = y[:, :T].reshape(B, T, G, C // G)
    em = float((np.abs(np.asarray(mean, F64) - grp.mean((1, 3))) / np.maximum(unit, 1e-300)).max())
    want = 1.0 / np.sqrt(grp.var((1, 3)) + eps)
    er = float((np.abs(np.asarray(rstd, F64) - want) / want).max())
    if figs is not None:
        figs[what + " mean units"] = em
        figs[what + " rstd rel"] = er
    if em > depth / 2 + 1:
        raise Miss("%s: mean off by %.2f units (bound %.1f)" % (what, em, depth / 2 + 1))
    if not er <= RSTD_REL:
        raise Miss("%s: rstd off by %.3e relative (bound %.0e)" % (what, er, RSTD_REL))


def words_to_group_stats(words, T, Tp, G, cols, eps):
    """Block words [B, Tp / 32, C / cols, 2] -> group mean, rstd [B, G] with the parallel-variance formula, all in fp64."""
    w = np.asarray(words, dtype=F64)
    B, RB, NB, _ = w.shape
    n_b = (cols * _counts(T, Tp)).reshape(1, RB, 1, 1)
    s1 = w[..., 0].reshape(B, RB, G, NB // G)
    n = (NB // G) * cols * float(T)
    mean = s1.sum((1, 3)) / n
    dm = s1 / n_b - mean[:, None, :, None]
    m2 = (w[..., 1].reshape(s1.shape) + n_b * dm * dm).sum((1, 3))
    return mean, 1.0 / np.sqrt(m2 / n + eps)


def check_words(what, words, x_blocks, depth, figs=None, shifted=False):
    """words [..., 2] = (sum, squared deviations about the block's own mean) of x_blocks [..., n] (fp64 values of one block each).
    shifted: the column slab forms both words from sums of values shifted by the block's FIRST value k (gemm_tile.h) and takes
    M2 = sum (v - k)^2 - (sum (v - k))^2 / n: its roundings are relative to those two terms, M2 + n (mean - k)^2 each."""
    xb = np.asarray(x_blocks, dtype=F64)
    w = np.asarray(words, dtype=F64)
    n = xb.shape[-1]
    unit = np.spacing(np.abs(xb).sum(-1).astype(F32)).astype(F64)
    es = np.abs(w[..., 0] - xb.sum(-1)) / np.maximum(unit, 1e-300)
    m2 = ((xb - xb.mean(-1, keepdims=True)) ** 2).sum(-1)
    scale = m2 + 2.0 * n * (xb.mean(-1) - xb[..., 0]) ** 2 if shifted else m2
    tol = (depth + 4) * 2.0 ** -24 * scale + ((depth / 2 + 1) * unit) ** 2 / n
    eq = np.abs(w[..., 1] - m2) / np.maximum(tol, 1e-300)
    if figs is not None:
        figs[what + " sum units"] = float(es.max())
        figs[what + " M2 / tol"] = float(eq.max())
    if es.max() > depth / 2 + 1:
        raise Miss("%s: block sum off by %.2f units (bound %.1f)" % (what, es.max(), depth / 2 + 1))
    if np.any(m2 == 0) and np.any(w[..., 1][m2 == 0] != 0):
        raise Miss("%s: a constant block has non-zero squared deviations" % what)
    if eq[m2 > 0].size and eq[m2 > 0].max() > 1.0:
        raise Miss("%s: squared deviations off by %.2f x their tolerance" % (what, eq[m2 > 0].max()))


def row_errors(got, want):
    """Per-row relative error over the last axis with parity_metrics' floor -> errors (flat), share of floored rows."""
    g = np.asarray(got, dtype=F64).reshape(-1, np.shape(want)[-1])
    w = np.asarray(want, dtype=F64).reshape(g.shape)
    wn = np.sqrt((w * w).sum(-1))
    floor = FLOOR_FRACTION * np.sqrt((wn * wn).mean())
    return np.sqrt(((g - w) ** 2).sum(-1)) / np.maximum(np.maximum(wn, floor), 1e-300), float((wn < floor).mean())


def emu_worst(emulated, want, constant=False):
    """The emulation's worst row against fp64 (constant: its largest absolute error)."""
    e, w = (np.asarray(a, dtype=F64).reshape(-1, np.shape(want)[-1]) for a in (emulated, want))
    return float(np.abs(e - w).max()) if constant else float(row_errors(e, w)[0].max())


def check_rows(what, got, emulated, want, in_planes, constant=False, figs=None, rows=None, pop_worst=0.0):
    """Every row of `got` within 2 x the worst row of `emulated` (+ 2^-16 for planes) of `want`; constant: absolute, against
    2 x the emulation's largest absolute error (+ 2^-16 |want|).  rows: boolean selector of the rows that count.  pop_worst: the
    emulation's worst row over the other row counts of the same case (emu_worst): the worst of ONE or five emulated rows says
    little about the worst row of the arithmetic - a row kernel at M = 1 is judged by the emulation's worst over all M of its C."""
    g, e, w = (np.asarray(a, dtype=F64).reshape(-1, np.shape(want)[-1]) for a in (got, emulated, want))
    if rows is not None:
        sel = np.asarray(rows).reshape(-1)
        g, e, w = g[sel], e[sel], w[sel]
    if constant:
        bound = 2.0 * max(np.abs(e - w).max(), pop_worst) + (PLANES_REL * np.abs(w).max() if in_planes else 0.0)
        err = float(np.abs(g - w).max())
    else:
        ee, floored = row_errors(e, w)
        ge, _ = row_errors(g, w)
        if floored > MAX_FLOORED:
            raise Miss("%s: %.1f %% of the rows sit on the norm floor" % (what, 100 * floored))
        bound = 2.0 * max(float(ee.max()), pop_worst) + (PLANES_REL if in_planes else 0.0)
        err = float(ge.max())
    if figs is not None:
        figs[what + " worst row"] = err
        figs[what + " bound"] = bound
    if not err <= bound:
        raise Miss("%s: worst row %.3e exceeds %.3e" % (what, err, bound))
