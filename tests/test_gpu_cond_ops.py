"""GPU: the conditioning path's fp32 kernels (csrc/kernels_misc.hip) one by one, through dv_op_timestep_embedding /
dv_op_small_linear / dv_op_pool_attention - the launchers the cond and step schedules call - against the fp64 restatements and the
derived per-element bounds of tests/cond_cases.py (tests/test_cond_reference.py shows on the CPU that the bounds can be met and
that ten planted faults break them).

  k_timestep_sincos   every element within sincos_bound(t, j); a row at t = 0 is exactly [1 .. 1 | 0 .. 0]; column 0 and column
                      half carry no argument error at all (the frequency at j = 0 is exactly 1: they are cosf(t) and sinf(t),
                      within the library's ulp of cos(t) and sin(t)); rows of equal t are bit-equal.
  k_small_linear      the pairwise covering ROUTE0; M = 32, K = 512 fills 64 KiB and runs, M = 33 is refused before a launch.
  k_small_linear_t    the pairwise covering ROUTE1 and, bit for bit: every row of an M = 50 launch equals the row launched alone,
                      inside an M = 8 and inside an M = 16 launch (MR 8 chunks, one MR 8 chunk, one MR 16 chunk), and a repeat.
  k_mean_token, k_pool_attn   L / S at and around the 64 lanes, D = 130 past the 128 threads, dph 8 and 4; a key 80 above the
                      rest, equal scores, scores of order 1e4: nothing but numbers; D / heads = 16 refused before a launch.
  SiLU                the measured worst of v / (1 + __expf(-v)) over every argument of the cases, in the unit of SILU_C.

Unwritten memory, as in tests/test_gpu_unwritten_memory.py: input rows behind M, input columns between K and ldin and everything
behind the weights, the bias and the added tensor hold NaN - a read of any of it shows in the result -; output columns between N and
ldo and the rows behind the last hold a sentinel that must survive bit for bit.

Each test prints its worst element as a fraction of its bound; DVITS_PARITY_REPORT=1 appends those lines to
profiles/cond_ops_parity.txt."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cond_cases as cc
from conftest import ROOT
from diff_vits_amd import _lib

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SENT = F32(12345.0)
INVALID = -1


def _report(line):
    print(line)
    if os.environ.get("DVITS_PARITY_REPORT") == "1":
        with open(os.path.join(ROOT, "profiles", "cond_ops_parity.txt"), "a") as f:
            f.write(line + "\n")


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _padded(a, rows, pitch, fill):
    """a [r, c] -> device [rows, pitch] with `fill` around it."""
    buf = np.full((rows, pitch), fill, dtype=F32)
    buf[:a.shape[0], :a.shape[1]] = a
    return torch.from_numpy(buf).cuda()


def _tailed(a, fill=np.nan, tail=64):
    """a flat on the device with `tail` elements of `fill` behind it."""
    return torch.from_numpy(np.concatenate([np.asarray(a, F32).reshape(-1), np.full(tail, fill, F32)])).cuda()


def small_linear(x, w, bias, add, route, silu_in=0, silu_out=0, add_rows=0, ldin=None, ldo=None, expect=0):
    """x [M, K], w [N, K] (transposed here for route 1), bias [N] or None, add [rows, N] or None -> out [M, N]; checks the sentinels."""
    M, K = x.shape
    N = w.shape[0]
    ldin, ldo = ldin or K, ldo or N
    d_in = _padded(x, M + 2, ldin, np.nan)
    d_w = _tailed(w if route == 0 else np.ascontiguousarray(w.T))
    d_b = None if bias is None else _tailed(bias)
    d_add = None if add is None else _padded(add, add.shape[0] + 2, ldo, np.nan)
    d_out = torch.full((M + 2, ldo), float(SENT), device="cuda")
    rc = _lib.lib().dv_op_small_linear(_lib.ptr(d_in), ldin, _lib.ptr(d_w), _lib.ptr(d_b), _lib.ptr(d_add), _lib.ptr(d_out), ldo, M, K, N,
                                       silu_in, silu_out, route, add_rows, _lib.stream_ptr())
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    if expect != 0:
        assert rc == expect and np.array_equal(bits(out), bits(np.full_like(out, SENT))), rc
        return None
    _lib.check(rc, "dv_op_small_linear")
    assert np.array_equal(bits(out[M:]), bits(np.full_like(out[M:], SENT))), "rows behind M written"
    assert np.array_equal(bits(out[:M, N:]), bits(np.full_like(out[:M, N:], SENT))), "columns between N and ldo written"
    return out[:M, :N].copy()


def run_case(c, silu_out=None, add=True):
    return small_linear(c["x"], c["w"], c["bias"], c["add"] if add else None, c["route"], c["silu_in"], c["silu_out"] if silu_out is None else silu_out,
                        c["add_rows"] if add else 0, c["ldin"], c["ldo"])


def _linear_cases(route, specs, kernel):
    worst, failed = (0.0, "", ()), []
    for spec in specs:
        c = cc.lin_case(route, spec)
        got = run_case(c)
        f, at = cc.fraction(got, cc.linear64(c), cc.linear_bound(c))
        print("%-32s worst element at %.3f of its bound %s" % (c["name"], f, at))
        if f > worst[0]:
            worst = (f, c["name"], at)
        if not f <= 1.0:
            failed.append((c["name"], f, at))
    _report("%-18s %3d cases: worst element at %.3f of its bound (%s %s)" % ((kernel, len(specs)) + worst))
    assert not failed, failed


# ------------------------------------------------------------------------------------------------------------ sinusoid
def timestep_embedding(t, dim):
    B = len(t)
    d_t = _tailed(t, tail=3)
    d_out = torch.full((B + 2, dim), float(SENT), device="cuda")
    _lib.check(_lib.lib().dv_op_timestep_embedding(_lib.ptr(d_t), _lib.ptr(d_out), B, dim, _lib.stream_ptr()), "dv_op_timestep_embedding")
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.array_equal(bits(out[B:]), bits(np.full_like(out[B:], SENT))), "rows behind B written"
    return out[:B].copy()


def test_timestep_embedding_within_the_formula_bound():
    worst = (0.0, "", ())
    for B, dim in cc.TS_CASES:
        t, half = cc.ts_times(B), dim // 2
        got = timestep_embedding(t, dim)
        want, bound = cc.sincos64(t, dim), cc.sincos_bound(t, dim)
        f, at = cc.fraction(got, want, bound)
        print("B = %3d dim = %3d: worst element at %.3f of its bound %s" % (B, dim, f, at))
        assert f <= 1.0, (B, dim, f, at)
        if f > worst[0]:
            worst = (f, "B%d_dim%d" % (B, dim), at)
        # t = 0: exact.  j = 0: the frequency is exactly 1, so the two columns are cosf(t) and sinf(t) of the input itself
        zero = t == 0
        assert np.all(got[zero, :half] == 1.0) and np.all(got[zero, half:] == 0.0)
        for col, fn in ((0, np.cos), (half, np.sin)):
            w = fn(t.astype(F64))
            assert np.all(np.abs(got[:, col] - w) <= cc.ULP1 * np.abs(w)), (B, dim, col)
        for b in range(B):          # equal t (TS_VALUES holds 1000 twice, and repeats every 9 rows): equal bits
            first = int(np.nonzero(t == t[b])[0][0])
            assert np.array_equal(bits(got[b]), bits(got[first])), (B, dim, b)
    _report("%-18s %3d cases: worst element at %.3f of its bound (%s %s)" % (("k_timestep_sincos", len(cc.TS_CASES)) + worst))


# ------------------------------------------------------------------------------------------------------------ small linears
def test_small_linear_route0_covering():
    _linear_cases(0, cc.ROUTE0, "k_small_linear")


def test_small_linear_t_route1_covering():
    _linear_cases(1, cc.ROUTE1 + cc.BITWISE, "k_small_linear_t")


def test_small_linear_lds_limits_are_refused_before_a_launch():
    L = _lib.lib()
    c = cc.lin_case(0, (32, 512, 130, 0, 0, "aio"))          # exactly 64 KiB: runs (test_small_linear_route0_covering holds it to its bound)
    assert run_case(c).shape == (32, 130)
    x = np.ones((33, 512), F32)
    w = np.ones((5, 512), F32)
    small_linear(x, w, None, None, 0, expect=INVALID)
    assert b"64 KiB" in L.dv_last_error() and b"33 x 512" in L.dv_last_error()
    small_linear(np.ones((2, 513), F32), np.ones((5, 513), F32), None, None, 1, expect=INVALID)
    assert b"512" in L.dv_last_error() and b"K = 513" in L.dv_last_error()
    small_linear(x[:2, :8], w[:, :8], None, None, 1, add_rows=3, expect=INVALID)          # add_rows without an add tensor
    assert b"add_rows" in L.dv_last_error()
    small_linear(x[:2, :8], w[:, :8], None, np.ones((2, 5), F32), 0, add_rows=2, expect=INVALID)      # ... or on route 0
    small_linear(x[:2, :8], w[:, :8], None, None, 2, expect=INVALID)
    assert b"route" in L.dv_last_error()
    small_linear(x[:2, :8], w[:, :8], None, None, 0, silu_in=2, expect=INVALID)
    f = torch.full((64,), float(SENT), device="cuda")
    p, s = _lib.ptr(f), _lib.stream_ptr()
    for args in ((None, 4, p, None, None, p, 4, 2, 4, 4, 0, 0, 0, 0, s), (p, 4, None, None, None, p, 4, 2, 4, 4, 0, 0, 0, 0, s),
                 (p, 4, p, None, None, None, 4, 2, 4, 4, 0, 0, 0, 0, s)):
        assert L.dv_op_small_linear(*args) == INVALID and b"null" in L.dv_last_error()
    for args in ((p, 3, p, None, None, p, 4, 2, 4, 4, 0, 0, 0, 0, s), (p, 4, p, None, None, p, 3, 2, 4, 4, 0, 0, 1, 0, s)):
        assert L.dv_op_small_linear(*args) == INVALID and b"ldin" in L.dv_last_error()
    for M, K, N in ((0, 4, 4), (2, 0, 4), (2, 4, 0), (65537, 4, 4)):
        assert L.dv_op_small_linear(p, max(K, 1), p, None, None, p, max(N, 1), M, K, N, 0, 0, 0, 0, s) == INVALID and b"M =" in L.dv_last_error()
    for args in ((None, p, 1, 32, s), (p, None, 1, 32, s), (p, p, 0, 32, s), (p, p, 1, 31, s), (p, p, 1, 0, s)):
        assert L.dv_op_timestep_embedding(*args) == INVALID
    torch.cuda.synchronize()
    assert bool((f == float(SENT)).all())


@pytest.mark.parametrize("spec", cc.BITWISE, ids=[cc.lin_name(1, s) for s in cc.BITWISE])
def test_small_linear_t_rows_are_bit_equal_in_every_launch_form(spec):
    """"per row the same arithmetic, bit for bit" (launch_small_linear_t) and "identical bits per row" (the step schedule's comment
    on the batched chain): with B in 9..16 a step runs the MR 16 form and the sampler's table of all evaluations the MR 8 chunks."""
    c = cc.lin_case(1, spec)
    M = c["M"]
    table = cc.lin_add_rows(c)                             # the added tensor row by row (exact: float32 values)
    add = (lambda rows: None) if table is None else (lambda rows: table[rows].astype(F32))
    run = lambda rows, **kw: small_linear(c["x"][rows], c["w"], c["bias"], add(rows), 1, c["silu_in"], c["silu_out"], 0, c["ldin"], c["ldo"], **kw)  # noqa: E731
    whole = run_case(c)
    assert np.array_equal(bits(whole), bits(run_case(c))), "two identical launches differ"
    for r in range(M):
        assert np.array_equal(bits(run(slice(r, r + 1))[0]), bits(whole[r])), ("alone", r)
    for width in (8, 16):
        for r0 in (0, 9, 17, M - width):
            got = run(slice(r0, r0 + width))
            differ = [r0 + i for i in range(width) if not np.array_equal(bits(got[i]), bits(whole[r0 + i]))]
            assert not differ, ("M = %d launch from row %d" % (width, r0), differ)
    # the wrapping lookup inside one chunk
    got = small_linear(c["x"][:8], c["w"], c["bias"], c["add"], 1, c["silu_in"], c["silu_out"], c["add_rows"], c["ldin"], c["ldo"])
    assert np.array_equal(bits(got), bits(whole[:8]))


def _silu_on_gpu(v, route, position):
    """silu of float32 values v through a K = 1, N = 1 launch with a unit weight: the dot is exact, the output is the SiLU alone."""
    out = []
    step = 16384 if route == 0 else 65536
    one = np.ones((1, 1), F32)
    for i in range(0, len(v), step):
        out.append(small_linear(v[i:i + step, None], one, None, None, route, int(position == "in"), int(position == "out"))[:, 0])
    return np.concatenate(out)


def test_silu_constant_covers_the_measured_worst():
    """SILU_C = 2 x the worst observed here (and not below float32 torch on the CPU, test_cond_reference.py)."""
    args = []
    for route, specs in ((0, cc.ROUTE0), (1, cc.ROUTE1 + cc.BITWISE)):
        for spec in specs:
            c = cc.lin_case(route, spec)
            if c["silu_in"]:
                args.append(c["x"].reshape(-1))
            if c["silu_out"]:          # the float32 pre-activation as the kernel forms it: the same launch without SiLU and add
                args.append(run_case(c, silu_out=0, add=False).reshape(-1))
    v = np.concatenate(args)
    worst = 0.0
    for route in (0, 1):
        for position in ("in", "out"):
            got = _silu_on_gpu(v, route, position)
            w = float(cc.silu_units(got, v).max())
            print("SiLU through route %d, %s position: worst %.3f u (1 + |v|) |silu(v)| over %d arguments" % (route, position, w, v.size))
            worst = max(worst, w)
    cpu = float(cc.silu_units(torch.nn.functional.silu(torch.from_numpy(v)).numpy(), v).max())
    _report("SiLU v / (1 + __expf(-v)): worst %.3f u (1 + |v|) |silu(v)| over %d arguments, |v| <= %.2f; float32 torch on the CPU %.3f; SILU_C = %.2f"
            % (worst, v.size, float(np.abs(v).max()), cpu, cc.SILU_C))
    assert worst <= cc.SILU_C and cpu <= cc.SILU_C


# ------------------------------------------------------------------------------------------------------------ mean token, pooling
def mean_token(x, pos):
    B, L, D = x.shape
    seq = np.full((B, L + 1, D), np.nan, F32)              # row 0 is written, never read
    seq[:, 1:] = x
    d_seq = _tailed(seq, fill=SENT)
    d_pos = _tailed(pos)
    _lib.check(_lib.lib().dv_op_pool_attention(_lib.ptr(d_seq), _lib.ptr(d_pos), None, None, None, B, L, D, 8, 0, _lib.stream_ptr()), "dv_op_pool_attention")
    torch.cuda.synchronize()
    out = d_seq.cpu().numpy()
    assert np.array_equal(bits(out[B * (L + 1) * D:]), bits(np.full(64, SENT))), "written behind seq"
    out = out[:B * (L + 1) * D].reshape(B, L + 1, D)
    assert np.array_equal(bits(out[:, 1:]), bits(x)), "rows 1..L touched"
    return out[:, 0].copy()


def pool_attention(q, kv, heads, expect=0):
    B, D = q.shape
    S = kv.shape[0] // B
    d_q, d_kv = _tailed(q), _tailed(kv)
    d_out = torch.full((B + 2, D), float(SENT), device="cuda")
    rc = _lib.lib().dv_op_pool_attention(None, None, _lib.ptr(d_q), _lib.ptr(d_kv), _lib.ptr(d_out), B, S - 1, D, heads, 1, _lib.stream_ptr())
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    if expect != 0:
        assert rc == expect and np.array_equal(bits(out), bits(np.full_like(out, SENT))), rc
        return None
    _lib.check(rc, "dv_op_pool_attention")
    assert np.array_equal(bits(out[B:]), bits(np.full_like(out[B:], SENT))), "rows behind B written"
    return out[:B].copy()


def test_mean_token_in_place():
    worst = (0.0, "", ())
    for spec in cc.MEAN_CASES:
        x, pos = cc.mean_case(*spec)
        got = mean_token(x, pos)
        f, at = cc.fraction(got, cc.mean_token64(x, pos), cc.mean_bound(x, pos))
        print("B = %d L = %3d D = %3d: worst element at %.3f of its bound %s" % (spec + (f, at)))
        assert f <= 1.0, (spec, f, at)
        if f > worst[0]:
            worst = (f, "B%d_L%d_D%d" % spec, at)
    _report("%-18s %3d cases: worst element at %.3f of its bound (%s %s)" % (("k_mean_token", len(cc.MEAN_CASES)) + worst))


def test_pool_attention_and_its_value_edges():
    worst = (0.0, "", ())
    for spec in cc.POOL_CASES:
        q, kv = cc.pool_case(*spec)
        got = pool_attention(q, kv, spec[3])
        assert np.all(np.isfinite(got)), spec
        f, at = cc.fraction(got, cc.pool64(q, kv, spec[3]), cc.pool_bound(q, kv, spec[3]))
        print("B = %d S = %3d D = %2d heads = %d %-6s: worst element at %.3f of its bound %s" % (spec + (f, at)))
        assert f <= 1.0, (spec, f, at)
        if f > worst[0]:
            worst = (f, "B%d_S%d_D%d_h%d_%s" % spec, at)
        if spec[4] == "equal":          # equal scores: every weight is exactly 1, the result the plain mean of the values
            B, S, D = spec[:3]
            mean = kv.reshape(B, S, 2 * D)[:, :, D:].astype(F64).mean(1)
            assert float(np.abs(got - mean).max()) <= (-(-S // 64) + 8) * cc.U * float(np.abs(kv).max())
    _report("%-18s %3d cases: worst element at %.3f of its bound (%s %s)" % (("k_pool_attn", len(cc.POOL_CASES)) + worst))


def test_pool_attention_refusals_come_before_a_launch():
    L = _lib.lib()
    q, kv = np.ones((2, 128), F32), np.ones((2 * 3, 256), F32)
    pool_attention(q, kv, 8, expect=INVALID)                                   # D / heads = 16
    assert b"D / heads = 16" in L.dv_last_error()
    pool_attention(q[:, :60], kv[:, :120], 8, expect=INVALID)                  # 60 is no multiple of 8
    assert b"multiple of heads" in L.dv_last_error()
    f = torch.full((4096,), float(SENT), device="cuda")
    p, s = _lib.ptr(f), _lib.stream_ptr()
    for args in ((p, p, None, None, None, 1, 3, 64, 8, 2, s), (p, None, None, None, None, 1, 3, 64, 8, 0, s), (p, p, p, None, None, 1, 3, 64, 8, 0, s),
                 (None, None, p, p, None, 1, 3, 64, 8, 1, s), (p, None, p, p, p, 1, 3, 64, 8, 1, s), (p, p, None, None, None, 0, 3, 64, 8, 0, s),
                 (p, p, None, None, None, 1, 0, 64, 8, 0, s), (None, None, p, p, p, 1, 3, 0, 8, 1, s), (None, None, p, p, p, 1, 3, 64, 0, 1, s)):
        assert L.dv_op_pool_attention(*args) == INVALID, args[5:10]
    torch.cuda.synchronize()
    assert bool((f == float(SENT)).all())
