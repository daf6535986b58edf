"""Cases and the fp64 restatement for the length regulator of the prior (reference model3.py:840-856; mirror
VITS.infer_from_encoder; native kernels csrc/kernels_regulate.hip).  Shared by tests/test_regulator_cpu.py and
tests/test_gpu_regulator.py; a case and its reference are computed once per process (lru_cache) and never modified.

The restatement is in GATHER form - a prefix sum over the integer durations and, per output frame, the first token whose
inclusive sum lies above the frame - where the reference multiplies a one-hot [B, T', Tx] alignment into m_p / logs_p.  The CPU
test pins the two forms against each other on every case.

Durations: w = exp(logw) * [j < x_len] * length_scale, d = ceil(w).  float32 and float64 agree on ceil(w) unless w is within
rounding of an integer, so every case is drawn with each valid token's fp64 w at least MARGIN = 1e-4 (relative) away from one - a
token that violates it is redrawn, no case is skipped - and `assert_margin` is asserted by every test that uses a case.  The one
place where the float32 range matters is modelled: exp(-200) is 0 in float32 (1.4e-87 in fp64 would ceil to 1), so the
exponential is rounded to float32 before anything else happens to it.

Comparison (`compare`), the one the GPU test applies to the operator and the CPU test to the mirror's torch branch and to the
planted faults: cum and y_len IDENTICAL, the gathered m / logs BIT-EQUAL to the inputs' columns (+0 on frames without a token),
|z - ref| <= 4 * 2^-23 * (|m| + |noise * exp(logs) * noise_scale|) per element: one expf at <= 1 ulp, two products and one sum, each
at half an ulp of a magnitude bounded by that of the two summands."""
import functools

import numpy as np

from diff_vits_amd import synth

SEED = 1234
MARGIN = 1e-4
EPS = 2.0 ** -23
ZERO = -200.0        # a log-duration whose exponential is exactly 0 in float32


def _ragged(Tx):
    return (Tx, Tx - 3, 1)


# name -> B, Tx, C, x_lengths, length_scale, noise_scale and either explicit integer durations [B][Tx] (0: logw = ZERO) or, with
# durations None, random log-durations N(0.5, 0.6^2) (median w 1.65) with logw = ZERO at the (b, j) of `zero_at`.  Each is the
# smallest shape that crosses one boundary of the kernels (256-thread workgroups of four wave64s; LDS search up to Tx = 1024).
CASES = {
    "one":        dict(B=1, Tx=1, C=5, x_lengths=(1,), durations=[[1]]),
    "tx63":       dict(B=1, Tx=63, C=5, x_lengths=(63,)),
    "tx64":       dict(B=1, Tx=64, C=5, x_lengths=(64,), length_scale=1.7),
    "tx65":       dict(B=1, Tx=65, C=5, x_lengths=(65,)),
    "tx255":      dict(B=1, Tx=255, C=5, x_lengths=(255,)),
    "tx256":      dict(B=1, Tx=256, C=5, x_lengths=(256,)),
    "tx257":      dict(B=1, Tx=257, C=5, x_lengths=(257,), length_scale=1.7),
    "tx1024":     dict(B=2, Tx=1024, C=5, x_lengths=(1024, 1000)),                     # the longest row searched in LDS
    "tx1025":     dict(B=2, Tx=1025, C=5, x_lengths=(1025, 1024)),                     # searched in global memory
    "tp255":      dict(B=1, Tx=17, C=5, x_lengths=(17,), durations=[[15] * 17]),
    "tp256":      dict(B=1, Tx=17, C=5, x_lengths=(17,), durations=[[15] * 16 + [16]]),
    "tp257":      dict(B=1, Tx=17, C=5, x_lengths=(17,), durations=[[15] * 16 + [17]]),
    "tp2048c128": dict(B=1, Tx=64, C=128, x_lengths=(64,), durations=[[32] * 64]),
    "longtoken":  dict(B=1, Tx=5, C=5, x_lengths=(5,), durations=[[3, 300, 2, 0, 4]]),     # one token spans two workgroups
    "ragged":     dict(B=3, Tx=65, C=128, x_lengths=_ragged(65), length_scale=1.7),
    "zeros":      dict(B=2, Tx=20, C=5, x_lengths=(20, 17), zero_at=[(0, 0), (0, 1), (0, 7), (0, 19), (1, 5), (1, 6), (1, 16)]),
    "allzero":    dict(B=2, Tx=9, C=5, x_lengths=(9, 6), zero_at=[(1, j) for j in range(9)]),   # y_len = 1, a frame without a token
    "ls0":        dict(B=2, Tx=12, C=5, x_lengths=(12, 4), length_scale=0.0),
    "ns0":        dict(B=2, Tx=33, C=5, x_lengths=(33, 30), length_scale=1.7, noise_scale=0.0),
}


def w_fp64(logw, x_len, length_scale):
    """[B, Tx] float64: the durations before ceil, the exponential rounded to float32 first (module docstring)."""
    logw = np.asarray(logw, dtype=np.float64)
    valid = np.arange(logw.shape[1])[None, :] < np.asarray(x_len)[:, None]
    with np.errstate(over="ignore"):
        e = np.exp(logw).astype(np.float32).astype(np.float64)
    return np.where(valid, e, 0.0) * float(length_scale), valid


def margin_violations(logw, x_len, length_scale):
    w, valid = w_fp64(logw, x_len, length_scale)
    return valid & (np.abs(w - np.rint(w)) < MARGIN * np.abs(w))


def assert_margin(case):
    assert not margin_violations(case["logw"], case["x_len"], case["length_scale"]).any()


def durations_ref(logw, x_len, length_scale):
    """cum [B, Tx] int64 (inclusive prefix sums of ceil(w)) and y_len [B] int64 = max(cum[b, x_len - 1], 1)."""
    w, _ = w_fp64(logw, x_len, length_scale)
    cum = np.cumsum(np.ceil(w).astype(np.int64), axis=1)
    return cum, np.maximum(cum[:, -1], 1)          # tokens behind x_len have w = 0: the last column is cum[b, x_len - 1]


def tokens_ref(cum, x_len, Tp):
    """tok [B, Tp]: the first j < x_len with cum[b, j] > t, or -1 (a frame without a token)."""
    tok = np.full((cum.shape[0], Tp), -1, dtype=np.int64)
    for b, n in enumerate(np.asarray(x_len)):
        j = np.searchsorted(cum[b, :n], np.arange(Tp), side="right")
        tok[b] = np.where(j < n, j, -1)
    return tok


def gather(a, tok):
    """a [B, C, Tx] -> [B, C, Tp] columns tok, +0 where tok = -1 (the alignment row of such a frame is all zeros)."""
    out = np.take_along_axis(a, np.broadcast_to(np.maximum(tok, 0)[:, None, :], (a.shape[0], a.shape[1], tok.shape[1])), axis=2)
    return np.where((tok >= 0)[:, None, :], out, np.zeros((), dtype=a.dtype))


def sample_ref(tok, m_p, logs_p, noise, noise_scale):
    """fp64 z = m + (noise * exp(logs)) * noise_scale on the gathered statistics, and the per-element bound of `compare`."""
    m, logs = gather(np.asarray(m_p, np.float64), tok), gather(np.asarray(logs_p, np.float64), tok)
    term = np.asarray(noise, np.float64) * np.exp(logs) * float(noise_scale)
    return m + term, 4.0 * EPS * (np.abs(m) + np.abs(term))


def regulate_ref(logw, x_len, m_p, logs_p, noise, length_scale, noise_scale):
    """(cum, y_len, z_p) in int64 / int64 / float64; the frame axis is the noise's (max(y_len) in the product)."""
    cum, y_len = durations_ref(logw, x_len, length_scale)
    z, _ = sample_ref(tokens_ref(cum, x_len, noise.shape[2]), m_p, logs_p, noise, noise_scale)
    return cum, y_len, z


def _draw_logw(name, spec, attempt):
    B, Tx, tag = spec["B"], spec["Tx"], "reg.%s.logw.%d" % (name, attempt)
    if spec.get("durations") is None:
        logw = synth.normal(SEED, tag, (B, Tx), std=0.6).astype(np.float64) + 0.5
        for b, j in spec.get("zero_at", ()):
            logw[b, j] = ZERO
        return logw.astype(np.float32)
    d = np.asarray(spec["durations"], dtype=np.float64)
    frac = 0.5 + 0.25 * synth.uniform(SEED, tag, (B, Tx)).astype(np.float64)          # w = d - frac, frac in [0.25, 0.75)
    with np.errstate(divide="ignore", invalid="ignore"):
        logw = np.where(d > 0, np.log(np.maximum(d - frac, 1e-30) / spec.get("length_scale", 1.0)), ZERO)
    return logw.astype(np.float32)


@functools.lru_cache(maxsize=None)
def make_case(name):
    """dict: logw [B, Tx], x_len [B], m_p / logs_p [B, C, Tx], noise [B, C, Tp] (float32 / int64), length_scale, noise_scale, Tp."""
    spec = CASES[name]
    B, Tx, C = spec["B"], spec["Tx"], spec["C"]
    ls, ns = spec.get("length_scale", 1.0), spec.get("noise_scale", 0.667)
    x_len = np.asarray(spec["x_lengths"], dtype=np.int64)
    logw = _draw_logw(name, spec, 0)
    for attempt in range(1, 32):
        bad = margin_violations(logw, x_len, ls)
        if not bad.any():
            break
        logw = np.where(bad, _draw_logw(name, spec, attempt), logw)
    _, y_len = durations_ref(logw, x_len, ls)
    Tp = int(y_len.max())
    case = dict(name=name, B=B, Tx=Tx, C=C, Tp=Tp, x_len=x_len, logw=logw, length_scale=ls, noise_scale=ns,
                m_p=synth.normal(SEED, "reg.%s.m" % name, (B, C, Tx)),
                logs_p=(synth.normal(SEED, "reg.%s.logs" % name, (B, C, Tx), std=0.3).astype(np.float64) - 0.5).astype(np.float32),
                noise=synth.normal(SEED, "reg.%s.noise" % name, (B, C, Tp)))
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def reference(name):
    """dict: cum, y_len, tok, z, bound, m_exp, logs_exp (the float32 inputs' gathered columns) of a case."""
    c = make_case(name)
    cum, y_len = durations_ref(c["logw"], c["x_len"], c["length_scale"])
    tok = tokens_ref(cum, c["x_len"], c["Tp"])
    z, bound = sample_ref(tok, c["m_p"], c["logs_p"], c["noise"], c["noise_scale"])
    ref = dict(cum=cum, y_len=y_len, tok=tok, z=z, bound=bound, m_exp=gather(c["m_p"], tok), logs_exp=gather(c["logs_p"], tok))
    for v in ref.values():
        v.setflags(write=False)
    return ref


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def compare(ref, cum=None, y_len=None, z=None, m_exp=None, logs_exp=None, label=""):
    """The comparison of the module docstring on whichever results are given; prints the figures before it asserts."""
    if cum is not None:
        assert np.array_equal(np.asarray(cum, dtype=np.int64), ref["cum"]), "%s: cum differs" % label
    if y_len is not None:
        assert np.array_equal(np.asarray(y_len, dtype=np.int64), ref["y_len"]), "%s: y_len %s != %s" % (label, y_len, ref["y_len"])
    for got, key in ((m_exp, "m_exp"), (logs_exp, "logs_exp")):
        if got is not None:
            assert got.shape == ref[key].shape and np.array_equal(_bits(got), _bits(ref[key])), "%s: %s is not the gathered input" % (label, key)
    if z is not None:
        z = np.asarray(z, dtype=np.float64)
        assert z.shape == ref["z"].shape, (label, z.shape, ref["z"].shape)
        assert np.isfinite(z).all(), "%s: z has elements that are not finite (not written?)" % label
        err = np.abs(z - ref["z"])
        ratio = float((err / np.maximum(ref["bound"], 1e-300)).max()) if err.max() > 0 else 0.0
        print("%s: max |z - ref| %.3e, worst error / bound %.3f" % (label, float(err.max()), ratio))
        assert (err <= ref["bound"]).all(), "%s: z misses the bound by a factor %.3g" % (label, ratio)
