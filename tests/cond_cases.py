"""The conditioning path's fp32 kernels (csrc/kernels_misc.hip: k_timestep_sincos, k_small_linear, k_small_linear_t<8 / 16> and its
chunked launch, k_mean_token, k_pool_attn): dense fp64 restatements of the three operations, the cases, the per-element bounds and
float32 emulations of each kernel's documented arithmetic with the faults the bounds must catch.  Shared by
tests/test_cond_reference.py (CPU) and tests/test_gpu_cond_ops.py (dv_op_timestep_embedding / dv_op_small_linear /
dv_op_pool_attention).  Plain helper module: no fixtures, no hooks.  Every input comes from `synth`.

The restatements are written from the modules this repository mirrors (unet1d/embeddings.py):
  sinusoid   [cos(t f_j) | sin(t f_j)], f_j = exp(-ln(10000) j / half), half = dim / 2      (flip_sin_to_cos=True, freq_shift=0)
  linear     act_out(act_in(x) w^T + bias) + add,  act = SiLU or nothing                    (TimestepEmbedding's two Linears)
  pooling    token = mean_r x_r + pos;  per head  softmax_s((q dph^-1/4) . (k_s dph^-1/4)) v_s    (AttentionPooling)

Bounds count roundings in units of u = 2^-24 (half an ulp of a float32 in [1, 2)), the way norm_cases.DEPTH does.  All of them are
per element and first order in u; every one is derived below next to its function.  The only measured constant is SILU_C."""
import math

import numpy as np
import torch

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
SEED = 7711
LN1E4 = math.log(10000.0)
LN1E4_F32 = float(F32(LN1E4))                        # the literal of the kernel and of float32 torch (a Python scalar times a float32 tensor)
D_LN = abs(LN1E4_F32 - LN1E4) / LN1E4                # 0.23 u: the constant's own rounding
ULP1 = 2.0 * U                                       # "1 ulp" of a library function relative to its value, counted as two roundings
                                                     # (csrc/kernels_align.hip:8, kernels_wn.hip:28 assume the same of expf)
# SiLU as the kernels compute it, v / (1 + __expf(-v)): the hardware exponential's error cannot be derived here.  Its allowance is
# SILU_C u (1 + |v|) |silu(v)| (the |v| term: the exponent's own rounding moves exp(-v) by |v| u relative).  Measured on the MI355X
# over the 260 053 values these cases put through a SiLU, through both kernels and both positions
# (tests/test_gpu_cond_ops.py test_silu_constant_covers_the_measured_worst): worst 2.251 in all four.  SILU_C = 2 x that (the margin
# covers the other machines of the pool); float32 torch.nn.functional.silu on the CPU shows 2.167 on the same values and 2.281 on the
# CPU's own set (tests/test_cond_reference.py), both below it.  Figures: profiles/cond_ops_parity.txt.
SILU_C = 4.5
SILU_LIP = 1.1                                       # max |silu'| = 1.0998 (at v = 2.3994)


def _normal(name, shape, std=1.0):
    from diff_vits_amd import synth
    return (synth.normal(SEED, name, shape).astype(F64) * std).astype(F32)


def silu64(v):
    v = np.asarray(v, dtype=F64)
    return v / (1.0 + np.exp(-v))


def silu_allow(v, ev=0.0, es=0.0):
    """What a float32 SiLU may be off by at fp64 argument v, when the argument it really sees is within ev of v (so that its value is
    within es = SILU_LIP ev of silu(v))."""
    return SILU_C * U * (1.0 + np.abs(v) + ev) * (np.abs(silu64(v)) + es)


def silu_units(got, v):
    """|got - silu64(v)| in units of u (1 + |v|) |silu(v)| for float32 arguments v (what SILU_C bounds); zeros of silu skipped."""
    v = np.asarray(v, dtype=F64)
    s = silu64(v)
    ok = s != 0
    return np.abs(np.asarray(got, F64) - s)[ok] / (U * (1.0 + np.abs(v[ok])) * np.abs(s[ok]))


# ------------------------------------------------------------------------------------------------------------ sinusoid
TS_VALUES = (0.0, 1.0, 0.5, 19.99, 999.0, 1000.0, 1e-3, 999.999, 1000.0)        # 999.999 sits next to 1000
TS_CASES = [(B, dim) for dim in (128, 32) for B in (1, 5, 257)]                  # 257 x 64 crosses 256-thread blocks, 5 x 16 ends inside one


def ts_times(B):
    """float32 [B]: TS_VALUES in turn (B = 1: 999.999, the largest argument with a fraction)."""
    return np.array([TS_VALUES[(b + (7 if B == 1 else 0)) % len(TS_VALUES)] for b in range(B)], dtype=F32)


def sincos64(t, dim):
    t = np.asarray(t, dtype=F64)
    half = dim // 2
    arg = t[:, None] * np.exp(-LN1E4 * np.arange(half, dtype=F64) / half)[None, :]
    return np.concatenate([np.cos(arg), np.sin(arg)], 1)


def sincos_bound(t, dim):
    """[B, dim].  Roundings on the way to arg = t exp(-L j / half), as relative errors of arg:
         L as a float32 literal  D_LN     the product L j  u     the division by half  u   (j and half are exact integers)
       - these three sit in the exponent x_j = L j / half and move exp by x_j (D_LN + 2 u) -; expf 1 ulp = 2 u; the product
       with t (exact: the input) u.  So rho_j = x_j (D_LN + 2 u) + 3 u and |d arg| <= t exp(-x_j) rho_j.  At j = 0 every step is
       exact (-L 0 = -0, -0 / half = -0, expf(-0) = 1, t 1 = t): rho_0 = 0 - column 0 is cosf(t) and column half sinf(t).
       |d cos|, |d sin| <= |d arg|; cosf / sinf add 1 ulp of the value they return, 2 u (|want| + |d arg|)."""
    t = np.abs(np.asarray(t, dtype=F64))
    half = dim // 2
    x = LN1E4 * np.arange(half, dtype=F64) / half
    rho = np.where(x > 0, x * (D_LN + 2 * U) + 3 * U, 0.0)
    darg = t[:, None] * (np.exp(-x) * rho)[None, :]
    darg = np.concatenate([darg, darg], 1)
    return darg + ULP1 * (np.abs(sincos64(t, dim)) + darg)


def _t32(fn, a):
    """A float32 library function through torch's CPU kernels (1-ulp vector routines)."""
    return fn(torch.from_numpy(np.array(a, dtype=F32))).numpy()


def sincos_emulate(t, dim, fault=None):
    """k_timestep_sincos in float32: e = -L j; e /= half; arg = t expf(e); [cosf | sinf].
    Faults: "swap" [sin | cos] (the flip left out), "half_m1" the divisor half - 1, "ln_bf16" the constant rounded to bf16."""
    half = dim // 2
    L = F32(LN1E4)
    if fault == "ln_bf16":
        L = ((np.array([L]).view(np.uint32) + np.uint32(0x8000)) & np.uint32(0xFFFF0000)).view(F32)[0]
    e = (-L) * np.arange(half, dtype=F32)
    e = e / F32(half - 1 if fault == "half_m1" else half)
    arg = np.asarray(t, dtype=F32)[:, None] * _t32(torch.exp, e)[None, :]
    c, s = _t32(torch.cos, arg), _t32(torch.sin, arg)
    return np.concatenate([s, c] if fault == "swap" else [c, s], 1)


def sincos_torch32(t, dim):
    from diff_vits_amd.unet1d.embeddings import Timesteps
    return Timesteps(dim, True, 0)(torch.from_numpy(np.asarray(t, dtype=F32))).numpy()


# ------------------------------------------------------------------------------------------------------------ small linear
# (M, K, N, wide ldin, wide ldo, flags): a pairwise covering of
#   M 1 7 8 9 16 32 | K 4 63 64 65 512 | N 1 3 4 5 130 4100 (two columns per wave) | ldin K or 3 K + 4 | ldo N or N + 3 |
#   flags - (none), a (add), i (silu_in), o (silu_out), aio (all three)
# every pair of values of two different parameters occurs in a case (test_cond_reference.py checks that); M = 32, K = 512 is
# exactly 64 KiB of staged rows.
ROUTE0 = [
    (1, 4, 1, 1, 1, "aio"), (1, 4, 4, 1, 0, "o"), (1, 63, 4100, 0, 1, "o"), (1, 64, 130, 1, 0, "-"), (1, 65, 5, 1, 0, "i"),
    (1, 512, 3, 1, 0, "a"), (7, 4, 4, 1, 0, "o"), (7, 4, 5, 0, 1, "-"), (7, 63, 1, 0, 1, "a"), (7, 63, 4100, 0, 0, "aio"),
    (7, 64, 3, 1, 0, "i"), (7, 65, 130, 0, 1, "a"), (7, 512, 4, 1, 0, "aio"), (8, 4, 3, 1, 0, "i"), (8, 4, 4100, 0, 0, "a"),
    (8, 63, 5, 1, 0, "aio"), (8, 63, 130, 0, 0, "i"), (8, 64, 4100, 1, 1, "o"), (8, 65, 4, 0, 1, "i"), (8, 512, 1, 1, 1, "-"),
    (9, 4, 130, 1, 1, "o"), (9, 63, 3, 0, 0, "o"), (9, 63, 4, 0, 0, "a"), (9, 64, 1, 0, 1, "aio"), (9, 65, 4100, 1, 0, "-"),
    (9, 512, 5, 0, 1, "i"), (16, 4, 3, 0, 1, "-"), (16, 4, 130, 1, 0, "a"), (16, 63, 1, 1, 0, "i"), (16, 64, 4, 1, 0, "a"),
    (16, 65, 3, 1, 0, "aio"), (16, 65, 5, 0, 0, "o"), (16, 512, 4100, 1, 0, "o"), (32, 4, 3, 1, 1, "i"), (32, 4, 4100, 0, 0, "i"),
    (32, 63, 4, 0, 0, "-"), (32, 64, 5, 1, 1, "a"), (32, 65, 1, 1, 0, "o"), (32, 512, 130, 0, 0, "aio"),
]
# the same for k_small_linear_t:  M 1 8 (MR 8) 9 16 (MR 16) 17 24 50 (chunks of 8, the last one partial) | K 13 128 512 |
#   N 1 63 64 65 200 | ldin | ldo | flags as above and a5: add with add_rows = 5 (M = 50 only: the rows wrap)
ROUTE1 = [
    (1, 13, 63, 0, 0, "o"), (1, 13, 63, 1, 0, "aio"), (1, 13, 200, 1, 1, "a"), (1, 128, 65, 1, 1, "i"), (1, 512, 1, 0, 0, "a"),
    (1, 512, 64, 0, 1, "-"), (8, 13, 1, 0, 1, "-"), (8, 128, 63, 0, 0, "i"), (8, 128, 65, 1, 0, "a"), (8, 128, 200, 1, 0, "o"),
    (8, 512, 64, 1, 1, "aio"), (9, 13, 64, 1, 1, "a"), (9, 13, 65, 0, 1, "-"), (9, 128, 1, 0, 0, "o"), (9, 128, 200, 0, 1, "aio"),
    (9, 512, 63, 0, 0, "i"), (16, 13, 64, 0, 1, "i"), (16, 13, 200, 1, 0, "a"), (16, 128, 1, 1, 0, "-"), (16, 512, 63, 0, 0, "aio"),
    (16, 512, 65, 1, 1, "o"), (17, 13, 64, 1, 1, "i"), (17, 13, 65, 1, 1, "aio"), (17, 13, 200, 1, 0, "-"), (17, 128, 64, 0, 0, "o"),
    (17, 512, 1, 0, 1, "aio"), (17, 512, 63, 0, 0, "a"), (24, 13, 1, 0, 1, "o"), (24, 13, 64, 0, 0, "-"), (24, 128, 63, 1, 1, "aio"),
    (24, 128, 65, 0, 0, "i"), (24, 512, 200, 0, 0, "a"), (50, 13, 1, 1, 1, "i"), (50, 13, 65, 0, 0, "a5"), (50, 13, 65, 1, 0, "a"),
    (50, 13, 65, 1, 0, "o"), (50, 13, 200, 1, 0, "a5"), (50, 128, 1, 0, 1, "a5"), (50, 128, 63, 1, 1, "aio"), (50, 128, 64, 1, 1, "a5"),
    (50, 128, 200, 1, 1, "i"), (50, 512, 63, 1, 0, "-"), (50, 512, 63, 1, 1, "a5"),
]
# the launches the bitwise claims are checked on: the time MLP's second Linear over a sampler's table (add = the pooled-text row of
# utterance r % 5) and the 22 time_emb_proj GEMVs (SiLU on the input)
BITWISE = [(50, 512, 200, 0, 0, "a5"), (50, 512, 200, 1, 1, "i"), (50, 13, 65, 0, 1, "a5o")]
FACTORS = {0: ((1, 7, 8, 9, 16, 32), (4, 63, 64, 65, 512), (1, 3, 4, 5, 130, 4100), (0, 1), (0, 1), ("-", "a", "i", "o", "aio")),
           1: ((1, 8, 9, 16, 17, 24, 50), (13, 128, 512), (1, 63, 64, 65, 200), (0, 1), (0, 1), ("-", "a", "i", "o", "aio", "a5"))}


def lin_name(route, spec):
    return "r%d_M%d_K%d_N%d_%s%s_%s" % ((route,) + tuple(spec[:3]) + ("w" if spec[3] else "t", "w" if spec[4] else "t", spec[5]))


_LIN = {}


def lin_case(route, spec):
    """dict: x [M, K], w [N, K], bias [N], add [rows, N] or None, add_rows, silu_in, silu_out, ldin, ldo (float32, read-only)."""
    key = (route,) + tuple(spec)
    if key not in _LIN:
        M, K, N, wi, wo, flags = spec
        name = lin_name(route, spec)
        c = dict(route=route, M=M, K=K, N=N, ldin=3 * K + 4 if wi else K, ldo=N + 3 if wo else N, name=name,
                 silu_in=int("i" in flags), silu_out=int("o" in flags), add_rows=5 if "a5" in flags else 0)
        c["x"] = _normal(name + ".x", (M, K), 1.5)                      # |v| up to ~6 through an input SiLU
        c["w"] = _normal(name + ".w", (N, K), 1.0 / math.sqrt(K))
        c["bias"] = _normal(name + ".b", (N,), 0.5)
        c["add"] = _normal(name + ".add", (c["add_rows"] or M, N)) if "a" in flags else None
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _LIN[key] = c
    return _LIN[key]


def lin_add_rows(c):
    """The added tensor row by row [M, N] (fp64), or None."""
    if c["add"] is None:
        return None
    a = c["add"].astype(F64)
    return a[np.arange(c["M"]) % c["add_rows"]] if c["add_rows"] else a


def linear64(c):
    x = silu64(c["x"]) if c["silu_in"] else c["x"].astype(F64)
    v = x @ c["w"].astype(F64).T + c["bias"].astype(F64)
    if c["silu_out"]:
        v = silu64(v)
    a = lin_add_rows(c)
    return v if a is None else v + a


def lin_depth(route, K):
    """Roundings on an output's longest path.  k_small_linear: a lane's strided FMA chain of ceil(K / 64) terms, 6 butterfly
    additions, the bias, the added tensor.  k_small_linear_t: a k-eighth's chain of ceil(K / 8) terms, 7 additions of the eight
    partial sums, the bias, the added tensor."""
    return -(-K // 64) + 8 if route == 0 else -(-K // 8) + 9


def linear_bound(c):
    """[M, N].  Without SiLU: depth u (sum_k |x_k w_k| + |bias| + |add|) - every rounding is half an ulp of a partial result,
    which is at most that sum.
    silu_in: the staged x_k = silu(in_k) is off by e_k <= silu_allow(in_k); the dot moves by sum_k e_k |w_k| and its roundings
    see |x_k| + e_k.
    silu_out: the pre-activation v carries ev = (depth - 1) u (sum |x w| + |bias|) (+ the input term): every rounding but the
    last addition; SiLU is 1.1-Lipschitz and adds its own allowance at an argument within ev of v; then, with an added tensor,
    one rounding of the sum, u (|silu(v)| + |add|) and the error carried so far."""
    D = lin_depth(c["route"], c["K"])
    xin = c["x"].astype(F64)
    aw = np.abs(c["w"].astype(F64)).T
    ex = silu_allow(xin) if c["silu_in"] else np.zeros_like(xin)
    x = silu64(xin) if c["silu_in"] else xin
    absdot = (np.abs(x) + ex) @ aw + np.abs(c["bias"].astype(F64))[None, :]
    prop = ex @ aw
    a = lin_add_rows(c)
    aa = 0.0 if a is None else np.abs(a)
    if not c["silu_out"]:
        return D * U * (absdot + aa) + prop
    v = x @ c["w"].astype(F64).T + c["bias"].astype(F64)
    ev = (D - 1) * U * absdot + prop
    es = SILU_LIP * ev + silu_allow(v, ev, SILU_LIP * ev)
    return es if a is None else es + U * (np.abs(silu64(v)) + es + aa)


def linear_torch32(c):
    F = torch.nn.functional
    t = lambda a: torch.from_numpy(np.array(a, dtype=F32))  # noqa: E731
    x = F.silu(t(c["x"])) if c["silu_in"] else t(c["x"])
    v = F.linear(x, t(c["w"]), t(c["bias"]))
    if c["silu_out"]:
        v = F.silu(v)
    a = lin_add_rows(c)
    return (v if a is None else v + t(a)).numpy()


def silu32(v):
    """v / (1 + exp(-v)) in float32 steps (the exponential through torch's float32 routine)."""
    v = np.asarray(v, dtype=F32)
    return v / (F32(1) + _t32(torch.exp, -v))


def _fma32(a, b, c):
    """fmaf: the product of two float32 is exact in fp64; (the fp64 sum rounds once more - no bit-exact model, one of the arithmetic)."""
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


LIN_FAULTS = ("drop_eighth", "add_mod_mr", "add_rows_ignored", "bias_after_silu")


def linear_emulate(c, fault=None):
    """The two kernels' arithmetic in float32 -> [M, N].  Faults: "drop_eighth" (route 1) the k-eighth is floor(K / 8) long, so
    the last K % 8 terms are dropped; "add_mod_mr" (route 1) a chunk looks its added row up with the row index inside the chunk;
    "add_rows_ignored" (route 1) row r adds add[r] (behind the table: the sentinel 7.0 of the buffers); "bias_after_silu"."""
    M, K, N, route = c["M"], c["K"], c["N"], c["route"]
    x = silu32(c["x"]) if c["silu_in"] else c["x"]
    w = c["w"]
    if route == 0:
        nk = -(-K // 64)
        xp, wp = np.zeros((M, nk * 64), F32), np.zeros((N, nk * 64), F32)
        xp[:, :K], wp[:, :K] = x, w
        acc = np.zeros((M, N, 64), F32)
        for i in range(nk):                                           # lane l: k = l, l + 64, ...
            acc = _fma32(xp[:, None, i * 64:(i + 1) * 64], wp[None, :, i * 64:(i + 1) * 64], acc)
        lanes = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):                                # wave_sum's butterfly
            acc = acc + acc[:, :, lanes ^ o]
        v = acc[:, :, 0]
    else:
        kq = K // 8 if fault == "drop_eighth" else -(-K // 8)
        v = np.zeros((M, N), F32)
        for e in range(8):
            acc = np.zeros((M, N), F32)
            for k in range(e * kq, min(K, (e + 1) * kq)):
                acc = _fma32(x[:, k:k + 1], w[None, :, k], acc)
            v = v + acc
    b = c["bias"][None, :]
    if fault != "bias_after_silu" or not c["silu_out"]:
        v = v + b
    if c["silu_out"]:
        v = silu32(v)
        if fault == "bias_after_silu":
            v = v + b
    if c["add"] is not None:
        rows = np.arange(M)
        mr = 16 if 8 < M <= 16 else 8
        if fault == "add_mod_mr" and route == 1:
            rows = rows % mr
        table = np.concatenate([c["add"], np.full((M, N), 7.0, F32)], 0)
        if c["add_rows"] and fault != "add_rows_ignored":
            rows = rows % c["add_rows"]
        v = v + table[rows]
    return v.astype(F32)


# ------------------------------------------------------------------------------------------------------------ mean token, pooling
MEAN_CASES = [(B, L, D) for L in (1, 63, 64, 256) for D in (64, 32, 130) for B in (1, 3)]      # D = 130: the 128-thread column loop wraps
# (B, S, D, heads, kind): plain = unit-scale q and k; peak80 = per head one key 80 above the rest (its position moves with the
# head and the utterance, the last key included); equal = every key of a head alike; big = scores of order 1e4
POOL_CASES = ([(B, S, D, 8, "plain") for S in (2, 64, 65, 129) for D in (64, 32) for B in (1, 3)]
              + [(3, S, D, 8, kind) for kind in ("peak80", "equal", "big") for S, D in ((129, 64), (65, 32), (2, 64))])


def mean_case(B, L, D):
    name = "mean_B%d_L%d_D%d" % (B, L, D)
    x = (_normal(name + ".x", (B, L, D)).astype(F64) + 0.25).astype(F32)
    pos = _normal(name + ".pos", (D,), 1.0 / math.sqrt(D))
    return x, pos


def mean_token64(x, pos):
    return np.asarray(x, F64).mean(1) + np.asarray(pos, F64)[None, :]


def mean_bound(x, pos):
    """[B, D]: a sequential float32 sum of L terms (L - 1 roundings, each at most u sum_r |x_r|), the division by L (u |sum| / L)
    and the addition of pos (u (|mean| + |pos|)): (L + 1) u (sum_r |x_r| / L + |pos|)."""
    x = np.asarray(x, F64)
    L = x.shape[1]
    return (L + 1) * U * (np.abs(x).sum(1) / L + np.abs(np.asarray(pos, F64))[None, :])


def mean_emulate(x, pos, fault=None):
    """k_mean_token in float32: rows added in order, / L, + pos.  Fault "lp1": divided by L + 1."""
    x = np.asarray(x, F32)
    s = np.zeros((x.shape[0], x.shape[2]), F32)
    for r in range(x.shape[1]):
        s = s + x[:, r]
    return s / F32(x.shape[1] + (1 if fault == "lp1" else 0)) + np.asarray(pos, F32)[None, :]


def mean_torch32(x, pos):
    x = torch.from_numpy(np.array(x, dtype=F32))
    return (x.mean(dim=1) + torch.from_numpy(np.array(pos, dtype=F32))).numpy()


_POOL = {}


def pool_case(B, S, D, heads, kind):
    """q [B, D], kv [B S, 2 D] (keys | values), float32, read-only."""
    key = (B, S, D, heads, kind)
    if key not in _POOL:
        name = "pool_B%d_S%d_D%d_%s" % (B, S, D, kind)
        dph = D // heads
        q = _normal(name + ".q", (B, D))
        k = _normal(name + ".k", (B, S, D))
        v = (_normal(name + ".v", (B, S, D)).astype(F64) + 0.5).astype(F32)
        if kind == "equal":
            k = np.repeat(k[:, :1], S, 1)
        elif kind == "big":
            q, k = (q.astype(F64) * 60).astype(F32), (k.astype(F64) * 60).astype(F32)
        elif kind == "peak80":
            # q = 4 on a head's first channel: the score is 4 k_0 / sqrt(dph); the rest of the keys score within +- 0.02
            q = np.zeros((B, D), F32)
            q[:, ::dph] = 4.0
            k = (k.astype(F64) * 1e-3).astype(F32)
            for b in range(B):
                for h in range(heads):
                    s0 = S - 1 if (h + b) % 3 == 0 else (37 * h + 11 * b + 3) % S
                    k[b, s0, h * dph] = F32(80.0 * math.sqrt(dph) / 4.0)
        kv = np.concatenate([k, v], 2).reshape(B * S, 2 * D)
        for a in (q, kv):
            a.setflags(write=False)
        _POOL[key] = (q, kv)
    return _POOL[key]


def _heads(q, kv, heads):
    B, D = q.shape
    S = kv.shape[0] // B
    dph = D // heads
    kv = np.asarray(kv).reshape(B, S, 2, heads, dph)
    return np.asarray(q).reshape(B, heads, dph), kv[:, :, 0].transpose(0, 2, 1, 3), kv[:, :, 1].transpose(0, 2, 1, 3), dph   # k, v [B, H, S, dph]


def pool64(q, kv, heads):
    qh, k, v, dph = _heads(np.asarray(q, F64), np.asarray(kv, F64), heads)
    sc = np.einsum("bhc,bhsc->bhs", qh * dph ** -0.25, k * dph ** -0.25)
    p = np.exp(sc - sc.max(-1, keepdims=True))
    p = p / p.sum(-1, keepdims=True)
    return np.einsum("bhs,bhsc->bhc", p, v).reshape(np.shape(q))


def pool_bound(q, kv, heads):
    """[B, D].  scale = 1 / sqrtf(sqrtf(dph)) is within 2.5 u (0.5 u handed on by the inner root, u the outer, u the division);
    each factor q scale, k scale one more rounding, their product one: a term of the score is within 2 (2.5 + 1) u + u = 8 u of
    itself, the dph additions u each of at most the sum of the terms' magnitudes:  e_s = (dph + 8) u sum_c |q_c k_sc| / sqrt(dph).
    The weight expf(sc_s - mx) sees e_s + e_max from the two scores, u |sc_s - mx| from the subtraction and 2 u from expf:
    relative eps_s = expm1(e_s + e_max + u |sc_s - mx|) + 2 u.  Numerator and denominator are sums of ceil(S / 64) terms per lane
    and a 6-step butterfly, the numerator's terms products: n_acc = 2 (ceil(S / 64) + 6) + 1 roundings relative to
    sum_s p_s |v_s|, and the division one of |out|.  With p the exact softmax, first order in eps:
      |d out_c| <= sum_s p_s eps_s (|v_sc| + |out_c|) + (n_acc + 1) u sum_s p_s |v_sc|."""
    q64, kv64 = np.asarray(q, F64), np.asarray(kv, F64)
    qh, k, v, dph = _heads(q64, kv64, heads)
    S = k.shape[2]
    sc = np.einsum("bhc,bhsc->bhs", qh, k) / math.sqrt(dph)
    e = (dph + 8) * U * np.einsum("bhc,bhsc->bhs", np.abs(qh), np.abs(k)) / math.sqrt(dph)
    top = sc.argmax(-1)[..., None]
    gap = np.abs(sc - np.take_along_axis(sc, top, -1))
    eps = np.expm1(e + np.take_along_axis(e, top, -1) + U * gap) + 2 * U
    p = np.exp(-gap)
    p = p / p.sum(-1, keepdims=True)
    out = np.einsum("bhs,bhsc->bhc", p, v)
    pav = np.einsum("bhs,bhsc->bhc", p, np.abs(v))
    n_acc = 2 * (-(-S // 64) + 6) + 1
    b = np.einsum("bhs,bhsc->bhc", p * eps, np.abs(v)) + (p * eps).sum(-1)[..., None] * np.abs(out) + (n_acc + 1) * U * pav
    return b.reshape(np.shape(q))


POOL_FAULTS = ("scale_once", "v_from_k")


def pool_emulate(q, kv, heads, fault=None):
    """k_pool_attn in float32: lane l takes keys l, l + 64, ...; running products in order; butterfly sums.
    Faults: "scale_once" the dph^-1/4 on q only; "v_from_k" the value channels read from the key half."""
    qh, k, v, dph = _heads(np.asarray(q, F32), np.asarray(kv, F32), heads)
    if fault == "v_from_k":
        v = k
    B, H, S, _ = k.shape
    scale = F32(1) / np.sqrt(np.sqrt(F32(dph)))
    ks = k if fault == "scale_once" else k * scale
    sc = np.zeros((B, H, S), F32)
    for c in range(dph):
        sc = sc + (qh[:, :, None, c] * scale) * ks[..., c]
    w = _t32(torch.exp, sc - sc.max(-1, keepdims=True))
    n = -(-S // 64) * 64
    wp = np.zeros((B, H, n), F32)
    wp[..., :S] = w
    vp = np.zeros((B, H, n, dph), F32)
    vp[:, :, :S] = v
    den, acc = np.zeros((B, H, 64), F32), np.zeros((B, H, 64, dph), F32)
    for i in range(n // 64):
        den = den + wp[..., i * 64:(i + 1) * 64]
        acc = acc + wp[..., i * 64:(i + 1) * 64, None] * vp[:, :, i * 64:(i + 1) * 64]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        den = den + den[..., lanes ^ o]
        acc = acc + acc[:, :, lanes ^ o]
    return (acc[:, :, 0] / den[:, :, :1]).reshape(np.shape(q)).astype(F32)


def pool_torch32(q, kv, heads, dtype=torch.float32):
    """AttentionPooling.forward's attention lines on given projections (embeddings.py:89-92) in `dtype`."""
    qh, k, v, dph = _heads(np.asarray(q), np.asarray(kv), heads)
    t = lambda a: torch.from_numpy(np.array(a)).to(dtype)  # noqa: E731
    scale = 1.0 / math.sqrt(math.sqrt(dph))
    w = torch.matmul(t(qh)[:, :, None, :] * scale, (t(k) * scale).transpose(-1, -2))
    w = torch.softmax(w, dim=-1)
    return torch.matmul(w, t(v)).reshape(np.shape(q)).numpy()


# ------------------------------------------------------------------------------------------------------------ the criterion
def fraction(got, want, bound):
    """Worst |got - want| / bound over the elements (a zero bound with a zero error counts 0, with any error inf), and where."""
    err = np.abs(np.asarray(got, F64) - np.asarray(want, F64))
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(err == 0, 0.0, err / bound)
    f = np.where(np.isfinite(np.asarray(got, F64)), f, np.inf)
    i = np.unravel_index(int(np.argmax(f)), f.shape)
    return float(f[i]), tuple(int(v) for v in i)
