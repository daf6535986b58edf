"""CPU: the restatements, bounds and case lists of tests/cond_cases.py (what tests/test_gpu_cond_ops.py holds the conditioning path's
kernels to).

  - the fp64 restatements agree with this repository's torch modules (Timesteps, TimestepEmbedding, AttentionPooling) run in fp64
    to 1e-12.  The modules pin float32 in three places (the arange of the frequencies, timesteps.float(), the softmax's
    w.float()); the test lifts those pins for the call - the name `torch` inside
    embeddings.py hands out an fp64 arange, the inputs are of a tensor class whose .float() stays fp64 -, nothing else is patched;
  - the float32 torch route and the float32 emulation of each kernel's documented arithmetic stay inside every derived bound on
    every case: the bounds can be met;
  - ten planted faults each break a bound on at least one listed case: the bounds are not vacuous.  The margins are printed
    (profiles/cond_ops_parity.txt holds a copy);
  - SILU_C is not below what float32 torch.nn.functional.silu shows against fp64 on the values the cases put through a SiLU;
  - the two explicit case lists of the small linears cover every pair of parameter values."""
import itertools
import math

import numpy as np
import pytest
import torch

import cond_cases as cc
from diff_vits_amd import synth
from diff_vits_amd.unet1d import embeddings

F32, F64 = np.float32, np.float64


class _Torch64:
    """`torch` as embeddings.py sees it, with arange producing fp64 whatever dtype is asked for."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def arange(*a, **kw):
        kw["dtype"] = torch.float64
        return torch.arange(*a, **kw)


class _Keep64(torch.Tensor):
    """An fp64 tensor whose .float() stays fp64; what is computed from it is of this class too."""

    def float(self):
        return self.double()


def _in64(a):
    return torch.from_numpy(np.array(a, dtype=F64)).as_subclass(_Keep64)


def _out(t):
    assert t.dtype == torch.float64
    return t.as_subclass(torch.Tensor).numpy()


@pytest.fixture
def fp64_modules(monkeypatch):
    """Only the name `torch` inside embeddings.py is replaced; the .float() pins are lifted by the class of the INPUT tensors."""
    monkeypatch.setattr(embeddings, "torch", _Torch64())


def _lin(x, w, bias, add=None, silu_in=0, silu_out=0, route=0):
    return dict(route=route, M=x.shape[0], K=x.shape[1], N=w.shape[0], x=x, w=w, bias=bias, add=add, add_rows=0, silu_in=silu_in, silu_out=silu_out)


def test_restatements_match_the_torch_modules_in_fp64(fp64_modules):
    for B, dim in cc.TS_CASES:
        t = cc.ts_times(B)
        got = _out(embeddings.Timesteps(dim, True, 0)(_in64(t)))
        assert float(np.abs(got - cc.sincos64(t, dim)).max()) <= 1e-12
    # TimestepEmbedding: Linear -> SiLU -> Linear, as two calls of the linear restatement
    C0, E = 128, 512
    shapes = {"linear_1.weight": (E, C0), "linear_1.bias": (E,), "linear_2.weight": (E, E), "linear_2.bias": (E,)}
    sd = synth.make_state_dict(shapes, seed=11)
    m = embeddings.TimestepEmbedding(C0, E).double()
    m.load_state_dict({k: torch.from_numpy(v).double() for k, v in sd.items()})
    x = cc.sincos64(cc.ts_times(5), C0).astype(F32)
    with torch.no_grad():
        got = _out(m(_in64(x)))
    h = cc.linear64(_lin(x, sd["linear_1.weight"], sd["linear_1.bias"], silu_out=1))
    want = h @ sd["linear_2.weight"].astype(F64).T + sd["linear_2.bias"].astype(F64)
    assert float(np.abs(got - want).max()) <= 1e-12 * max(1.0, float(np.abs(want).max()))
    # AttentionPooling: mean token, three Linears, the pooling
    for B, L, D, heads in ((3, 63, 64, 8), (1, 1, 32, 8), (2, 128, 64, 8)):
        shapes = {"positional_embedding": (1, D)}
        for n in "qkv":
            shapes[n + "_proj.weight"], shapes[n + "_proj.bias"] = (D, D), (D,)
        sd = synth.make_state_dict(shapes, seed=12)
        sd["positional_embedding"] = synth.normal(12, "pos", (1, D), 1.0 / math.sqrt(D))
        m = embeddings.AttentionPooling(heads, D).double()
        m.load_state_dict({k: torch.from_numpy(v).double() for k, v in sd.items()})
        x, _ = cc.mean_case(B, L, D)
        with torch.no_grad():
            got = _out(m(_in64(x)))
        token = cc.mean_token64(x, sd["positional_embedding"][0])
        seq = np.concatenate([token[:, None, :], x.astype(F64)], 1)
        lin = lambda a, n: a @ sd[n + "_proj.weight"].astype(F64).T + sd[n + "_proj.bias"].astype(F64)  # noqa: E731
        kv = np.concatenate([lin(seq, "k"), lin(seq, "v")], 2).reshape(B * (L + 1), 2 * D)
        want = cc.pool64(lin(token, "q"), kv, heads)
        assert float(np.abs(got - want).max()) <= 1e-12, (B, L, D)
    # and the attention lines alone, as pool_torch32 restates them
    for spec in cc.POOL_CASES:
        q, kv = cc.pool_case(*spec)
        w = cc.pool64(q, kv, spec[3])
        assert float(np.abs(cc.pool_torch32(q.astype(F64), kv.astype(F64), spec[3], torch.float64) - w).max()) <= 1e-12 * max(1.0, float(np.abs(w).max()))


def test_case_lists_cover_every_pair():
    for route, cases in ((0, cc.ROUTE0), (1, cc.ROUTE1)):
        fac = cc.FACTORS[route]
        assert len(set(cases)) == len(cases)
        for spec in cases:
            assert all(v in f for v, f in zip(spec, fac)), spec
            assert spec[5] != "a5" or spec[0] == 50
        for a, b in itertools.combinations(range(6), 2):
            seen = {(s[a], s[b]) for s in cases}
            for va, vb in itertools.product(fac[a], fac[b]):
                if "a5" in (va, vb) and ((a == 0 and va != 50) or (b == 0 and vb != 50)):
                    continue
                assert (va, vb) in seen, (route, a, va, b, vb)
    assert (32, 512) in {(s[0], s[1]) for s in cc.ROUTE0}                  # exactly 64 KiB of staged rows
    assert cc.lin_depth(0, 512) == 16 and cc.lin_depth(0, 65) == 10 and cc.lin_depth(1, 13) == 11 and cc.lin_depth(1, 512) == 73


def _worst(results):
    """results: iterable of (label, got, want, bound) -> (worst fraction, label, index)."""
    best = (-1.0, "", ())
    for label, got, want, bound in results:
        f, at = cc.fraction(got, want, bound)
        if f > best[0]:
            best = (f, label, at)
    return best


def _sincos(fn):
    for B, dim in cc.TS_CASES:
        t = cc.ts_times(B)
        yield "B%d_dim%d" % (B, dim), fn(t, dim), cc.sincos64(t, dim), cc.sincos_bound(t, dim)


def _linear(route, fn, only=lambda c: True):
    for spec in (cc.ROUTE0 if route == 0 else cc.ROUTE1 + cc.BITWISE):
        c = cc.lin_case(route, spec)
        if only(c):
            yield c["name"], fn(c), cc.linear64(c), cc.linear_bound(c)


def _mean(fn):
    for spec in cc.MEAN_CASES:
        x, pos = cc.mean_case(*spec)
        yield "B%d_L%d_D%d" % spec, fn(x, pos), cc.mean_token64(x, pos), cc.mean_bound(x, pos)


def _pool(fn):
    for spec in cc.POOL_CASES:
        q, kv = cc.pool_case(*spec)
        yield "B%d_S%d_D%d_h%d_%s" % spec, fn(q, kv, spec[3]), cc.pool64(q, kv, spec[3]), cc.pool_bound(q, kv, spec[3])


EMULATED_N = 130          # the emulation of k_small_linear holds [M, N, 64] lanes: the N = 4100 cases (two columns per wave: indexing,
                          # not arithmetic) are left to the torch route


def test_float32_routes_stay_inside_every_bound():
    routes = {
        "sinusoid": (_sincos(cc.sincos_torch32), _sincos(cc.sincos_emulate)),
        "k_small_linear": (_linear(0, cc.linear_torch32), _linear(0, cc.linear_emulate, lambda c: c["N"] <= EMULATED_N)),
        "k_small_linear_t": (_linear(1, cc.linear_torch32), _linear(1, cc.linear_emulate)),
        "mean token": (_mean(cc.mean_torch32), _mean(cc.mean_emulate)),
        "pooling": (_pool(cc.pool_torch32), _pool(cc.pool_emulate)),
    }
    for op, (torch_route, emulation) in routes.items():
        for label, results in (("float32 torch", torch_route), ("float32 emulation", emulation)):
            f, name, at = _worst(results)
            print("%-17s %-18s worst element at %.3f of its bound (%s %s)" % (op, label, f, name, at))
            assert f <= 1.0, (op, label, name, at, f)
    for spec in cc.POOL_CASES:                       # the value edges produce nothing that is not a number
        q, kv = cc.pool_case(*spec)
        assert np.all(np.isfinite(cc.pool_emulate(q, kv, spec[3]))) and np.all(np.isfinite(cc.pool_torch32(q, kv, spec[3])))


def _silu_arguments():
    """Every float32 value the cases put through a SiLU: the inputs of the silu_in cases, the pre-activations of the silu_out ones."""
    out = []
    for route, cases in ((0, cc.ROUTE0), (1, cc.ROUTE1 + cc.BITWISE)):
        for spec in cases:
            c = cc.lin_case(route, spec)
            if c["silu_in"]:
                out.append(c["x"].reshape(-1))
            if c["silu_out"]:
                out.append(cc.linear64(dict(c, silu_out=0, add=None)).astype(F32).reshape(-1))
    return np.concatenate(out)


def test_silu_constant_is_not_below_float32_torch():
    v = _silu_arguments()
    got = torch.nn.functional.silu(torch.from_numpy(v)).numpy()
    worst = float(cc.silu_units(got, v).max())
    print("float32 torch.nn.functional.silu on the CPU over %d arguments, |v| <= %.2f: worst %.3f u (1 + |v|) |silu(v)|; SILU_C = %.2f"
          % (v.size, float(np.abs(v).max()), worst, cc.SILU_C))
    assert v.size > 10000 and float(np.abs(v).max()) > 4.0
    assert cc.SILU_C >= worst


# (number, fault, what runs it): each must exceed its bound on at least one listed case
def _faulted():
    lt = lambda f, only=lambda c: True: _linear(1, lambda c: cc.linear_emulate(c, f), only)  # noqa: E731
    yield 1, "sin and cos swapped (the flip left out)", _sincos(lambda t, d: cc.sincos_emulate(t, d, "swap"))
    yield 2, "half - 1 as the divisor", _sincos(lambda t, d: cc.sincos_emulate(t, d, "half_m1"))
    yield 3, "ln(10000) rounded to bf16", _sincos(lambda t, d: cc.sincos_emulate(t, d, "ln_bf16"))
    yield 4, "last k-eighth dropped when K % 8 != 0", lt("drop_eighth")
    yield 5, "row index modulo MR in a chunk's add lookup", lt("add_mod_mr", lambda c: c["add"] is not None)
    yield 6, "add_rows ignored", lt("add_rows_ignored", lambda c: c["add_rows"] > 0)
    yield 7, "bias added after the output SiLU", itertools.chain(
        _linear(0, lambda c: cc.linear_emulate(c, "bias_after_silu"), lambda c: c["silu_out"] and c["N"] <= EMULATED_N),
        lt("bias_after_silu", lambda c: c["silu_out"]))
    yield 8, "pooling scale applied once", _pool(lambda q, kv, h: cc.pool_emulate(q, kv, h, "scale_once"))
    yield 9, "mean token divided by L + 1", _mean(lambda x, p: cc.mean_emulate(x, p, "lp1"))
    yield 10, "value channels read from the key half", _pool(lambda q, kv, h: cc.pool_emulate(q, kv, h, "v_from_k"))


def test_planted_faults_break_their_bounds():
    for number, what, results in _faulted():
        results = list(results)
        fr = [(cc.fraction(g, w, b)[0], label) for label, g, w, b in results]
        caught = [f for f in fr if f[0] > 1.0]
        worst = max(fr)
        print("fault %2d  %-46s caught on %3d of %3d cases, worst element %.3g x its bound (%s)" % (number, what, len(caught), len(fr), worst[0], worst[1]))
        assert caught, (number, what)
    # the faults of the chunked launch are seen where they live: on the rows of the second and later chunks, and only there
    c = cc.lin_case(1, (50, 13, 65, 0, 0, "a5"))
    w, b = cc.linear64(c), cc.linear_bound(c)
    bad = np.abs(cc.linear_emulate(c, "add_mod_mr").astype(F64) - w) > b
    assert not bad[:8].any() and bad[8:].any()
