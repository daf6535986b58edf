"""GPU: normalisation statistics at value edges on the kernels the forward runs, through dv_op_layer_norm / _into, dv_op_prompt_pre,
dv_op_linear_ln and dv_op_linear_gn.  Cases, emulations, bounds and the assertions themselves: tests/norm_cases.py (what those
bounds can and cannot see: tests/test_norm_reference.py, profiles/norm_reference.txt; measured figures: profiles/norm_ops_parity.txt).
Every output buffer is pre-filled with NaN (0x7fc1 in the planes), every op is called twice and must return the same bits."""
import numpy as np
import pytest
import torch

import norm_cases as nc

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
EPS = 1e-5
OFFSET_EDGES = ["offset%d" % o for o in nc.OFFSET_GRID]
ALL_EDGES = [e for e in nc.EDGES if not e.startswith("offset")] + OFFSET_EDGES


def _L():
    from diff_vits_amd import _lib as L
    return L


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan(shape):
    return torch.full(shape, float("nan"), device="cuda")


def _planes_buf(shape):
    return torch.full(shape, 0x7fc1, dtype=torch.int16, device="cuda")    # a bf16 NaN in every element


def _twice(call, outs):
    """Runs the op twice; returns the host copies of `outs` after the second call, having compared them with the first."""
    call()
    torch.cuda.synchronize()
    first = [o.cpu().numpy().copy() for o in outs]
    call()
    torch.cuda.synchronize()
    second = [o.cpu().numpy() for o in outs]
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes(), "two calls of the same op differ"
    return second


def _report(figs):
    for k in sorted(figs):
        print("norm_ops %-60s %.3e" % (k, figs[k]))


ROW_SHAPES = [(M, C) for C in (4, 100, 128, 512, 2048) for M in (1, 5, 130)]
_POP = {}


def _row_population(route, edge, C, gname):
    """The emulation's worst row (fp32 output, planes) over every M of this C, edge and gamma: norm_cases.check_rows pop_worst."""
    key = (route in ("rows",), route == "apply", edge, C, gname)
    if key not in _POP:
        w32 = wpl = 0.0
        for M in sorted({m for m, c in ROW_SHAPES if c == C}):
            x = nc.edge_values(edge, (M, C), "rows.%d.%d" % (M, C))
            g, b = (None, None) if route == "apply" else nc.affine(C, gname)
            _, _, emu = nc.ln_emulate(x, g, b, eps=EPS, fma=route.startswith("affine"))
            want = nc.ln64(x, g, b, EPS)[2]
            w32 = max(w32, nc.emu_worst(emu, want, edge == "constant"))
            wpl = max(wpl, nc.emu_worst(nc.planes(emu), want, edge == "constant"))
        _POP[key] = (w32, wpl)
    return _POP[key]


@pytest.mark.parametrize("edge", ALL_EDGES)
@pytest.mark.parametrize("route", ["stats", "rows", "apply", "affine", "affine-masked"])
def test_layer_norm_rows(route, edge):
    """k_ln_rows<false> / <true>, k_ln_apply, k_ln_affine: C covers one float4 per row, a lane-ragged C and the loop's last slot, M
    partial four-row workgroups; the mask has masked rows at both ends.  Mean: 9 units (16 additions on the longest path)."""
    L = _L()
    lib, figs = L.lib(), {}
    for M, C in ROW_SHAPES:
        for gname in (nc.GAMMAS if C == 128 and route not in ("stats", "apply") else ("plain",)):
            x = nc.edge_values(edge, (M, C), "rows.%d.%d" % (M, C))
            g, b = nc.affine(C, gname)
            mask = None
            if route == "affine-masked":
                mask = np.ones(M, dtype=F32)
                mask[[0, M - 1]] = 0
                if M > 8:
                    mask[[1, 7, M - 2]] = 0
            dx, dg, db, dm = _dev(x), _dev(g), _dev(b), (None if mask is None else _dev(mask))
            tag = "%s %s M=%d C=%d %s" % (route, edge, M, C, gname)
            m64, r64, n64 = nc.ln64(x, eps=EPS)
            pop = _row_population(route, edge, C, gname)
            if route == "stats":
                mean, rstd = _nan((M,)), _nan((M,))
                mean_h, rstd_h = _twice(lambda: L.check(lib.dv_op_layer_norm(L.ptr(dx), None, None, None, None, None, None, L.ptr(mean), L.ptr(rstd),
                                                                             M, C, EPS, L.LN_STATS, None), tag), [mean, rstd])
                nc.check_stats(tag, mean_h, rstd_h, x.astype(F64)[:, None, :], EPS, nc.DEPTH["ln_rows"], figs)
                continue
            const = edge == "constant"
            if route == "rows":
                y = _nan((M, C))
                (got,) = _twice(lambda: L.check(lib.dv_op_layer_norm(L.ptr(dx), L.ptr(dg), L.ptr(db), None, L.ptr(y), None, None, None, None, M, C, EPS,
                                                                     L.LN_ROWS, None), tag), [y])
                _, _, emu = nc.ln_emulate(x, g, b, eps=EPS)
                nc.check_rows(tag, got, emu, nc.ln64(x, g, b, EPS)[2], False, const, figs, None, pop[0])
                if const:
                    assert np.array_equal(got, np.broadcast_to(b, (M, C))), tag
            elif route == "apply":
                hi, lo = _planes_buf((M, C)), _planes_buf((M, C))
                hb, lb = _twice(lambda: L.check(lib.dv_op_layer_norm(L.ptr(dx), None, None, None, None, L.ptr(hi), L.ptr(lo), None, None, M, C, EPS,
                                                                     L.LN_APPLY, None), tag), [hi, lo])
                got = nc.from_planes(hb.view(np.uint16), lb.view(np.uint16))
                _, _, emu = nc.ln_emulate(x, eps=EPS)
                nc.check_rows(tag, got, nc.planes(emu), n64, True, const, figs, None, pop[1])
                if const:
                    assert not got.any(), tag
            else:
                y, hi, lo = _nan((M, C)), _planes_buf((M, C)), _planes_buf((M, C))
                yh, hb, lb = _twice(lambda: L.check(lib.dv_op_layer_norm(L.ptr(dx), L.ptr(dg), L.ptr(db), L.ptr(dm), L.ptr(y), L.ptr(hi), L.ptr(lo), None,
                                                                         None, M, C, EPS, L.LN_AFFINE, None), tag), [y, hi, lo])
                _, _, emu = nc.ln_emulate(x, g, b, mask, eps=EPS, fma=True)
                want = nc.ln64(x, g, b, EPS)[2] * (1.0 if mask is None else mask[:, None].astype(F64))
                keep = None if mask is None else mask != 0
                if keep is None or keep.any():
                    nc.check_rows(tag, yh, emu, want, False, const, figs, keep, pop[0])
                    nc.check_rows(tag + " planes", nc.from_planes(hb.view(np.uint16), lb.view(np.uint16)), nc.planes(emu), want, True, const, figs, keep, pop[1])
                if mask is not None:
                    assert not yh[mask == 0].any() and not (hb.view(np.uint16)[mask == 0] & 0x7fff).any(), tag
                assert np.array_equal(nc.planes(yh), nc.from_planes(hb.view(np.uint16), lb.view(np.uint16))), tag   # planes = the split of y
    _report(figs)


@pytest.mark.parametrize("edge", ["unit", "offset300", "constant"])
def test_layer_norm_into_remap(edge):
    """k_ln_rows<true> with the re-mapping of the pooled-text sequence: 2 utterances of 5 rows into 6-row slots at offset 1.  The slot
    rows nobody maps to keep their NaN pattern bit for bit."""
    L = _L()
    lib, figs = L.lib(), {}
    for C in (4, 100, 128):
        x = nc.edge_values(edge, (10, C), "into.%d" % C)
        g, b = nc.affine(C, "signs")
        dx, dg, db = _dev(x), _dev(g), _dev(b)
        y = _nan((12, C))
        before = y.cpu().numpy().copy()
        (got,) = _twice(lambda: L.check(lib.dv_op_layer_norm_into(L.ptr(dx), L.ptr(dg), L.ptr(db), L.ptr(y), 10, C, EPS, 5, 6, 1, None), "into"), [y])
        got = got.reshape(2, 6, C)
        assert got[:, 0].tobytes() == before.reshape(2, 6, C)[:, 0].tobytes()
        _, _, emu = nc.ln_emulate(x, g, b, eps=EPS)
        nc.check_rows("into %s C=%d" % (edge, C), got[:, 1:].reshape(10, C), emu, nc.ln64(x, g, b, EPS)[2], False, edge == "constant", figs)
    _report(figs)
    lib_rc = lib.dv_op_layer_norm_into(L.ptr(dx), L.ptr(dg), L.ptr(db), L.ptr(y), 10, C, EPS, 5, 5, 1, None)
    assert lib_rc == -1 and b"do not fit" in lib.dv_last_error()


def test_layer_norm_refuses():
    """A C the launchers refuse is an error, not a fall-back; so is an output a route does not write."""
    L = _L()
    lib = L.lib()
    x, y = _dev(np.zeros((4, 2052), dtype=F32)), _nan((4, 2052))
    g = _dev(np.ones(2052, dtype=F32))
    for C in (6, 2052):
        assert lib.dv_op_layer_norm(L.ptr(x), L.ptr(g), L.ptr(g), None, L.ptr(y), None, None, None, None, 4, C, EPS, L.LN_ROWS, None) == -1
        assert b"multiple of 4" in lib.dv_last_error()
    assert lib.dv_op_layer_norm(L.ptr(x), L.ptr(g), L.ptr(g), None, L.ptr(y), None, None, None, None, 4, 128, EPS, 7, None) == -1
    assert lib.dv_op_layer_norm(L.ptr(x), None, None, None, L.ptr(y), None, None, L.ptr(y), L.ptr(y), 4, 128, EPS, L.LN_STATS, None) == -1
    assert lib.dv_op_prompt_pre(L.ptr(x), L.ptr(x), L.ptr(g), L.ptr(g), L.ptr(y), None, L.ptr(y), 1, 100, 4, 64, EPS, None) == -1
    assert lib.dv_op_linear_ln(L.ptr(x), L.ptr(x), None, None, L.ptr(g), L.ptr(g), L.ptr(x), None, 4, 32, 544, 8, 1, L.ptr(y), L.ptr(y), L.ptr(y), None) == -1
    assert b"16 partials" in lib.dv_last_error()
    # the column slab and k_stat16 have no padded-row form
    for route in (L.GN_SLAB, L.GN_KSTAT16):
        assert lib.dv_op_linear_gn(L.ptr(x), L.ptr(x), None, L.ptr(g), L.ptr(g), 1, 40, 64, 32, 32, 2, EPS, route, L.ptr(y), None, L.ptr(y), L.ptr(y), None) == -1
        assert b"padded-row" in lib.dv_last_error()
    assert torch.isnan(y).all()


@pytest.mark.parametrize("edge", ["unit", "offset30", "offset300", "constant", "outlier", "small-sigma"])
def test_prompt_pre(edge):
    """k_prompt_pre at the model's prompt width (100 -> 128), C = 1 and C = cpad = 512; L = 33, ragged keep, one utterance all padding.
    Columns [C, cpad) are exactly zero, key_bias exactly 0 / -1e30, a padding frame holds beta.  C = 1: every frame is constant."""
    L = _L()
    lib, figs = L.lib(), {}
    B, Ln = 3, 33
    lengths = [33, 0, 17]
    keep = np.zeros((B, Ln), dtype=F32)
    for i, n in enumerate(lengths):
        keep[i, :n] = 1
    for C, cpad in ((100, 128), (1, 32), (512, 512)):
        for gname in nc.GAMMAS:
            xr = nc.edge_values(edge, (B, Ln, C), "prompt.%d" % C)                        # rows = frames
            prompt = np.ascontiguousarray(xr.transpose(0, 2, 1))                          # [B, C, L]
            g, b = nc.affine(C, gname)
            dp, dk, dg, db = _dev(prompt), _dev(keep), _dev(g), _dev(b)
            hi, lo, kb = _planes_buf((B * Ln, cpad)), _planes_buf((B * Ln, cpad)), _nan((B, Ln))
            tag = "prompt_pre %s C=%d %s" % (edge, C, gname)
            hb, lb, kbh = _twice(lambda: L.check(lib.dv_op_prompt_pre(L.ptr(dp), L.ptr(dk), L.ptr(dg), L.ptr(db), L.ptr(hi), L.ptr(lo), L.ptr(kb), B, C, Ln,
                                                                      cpad, EPS, None), tag), [hi, lo, kb])
            hb, lb = hb.view(np.uint16).reshape(B, Ln, cpad), lb.view(np.uint16).reshape(B, Ln, cpad)
            assert not hb[:, :, C:].any() and not lb[:, :, C:].any(), tag
            assert np.array_equal(kbh, np.where(keep != 0, F32(0), F32(-1e30))), tag
            got = nc.from_planes(hb, lb)[:, :, :C]
            pad = keep == 0
            assert np.array_equal(got[pad], np.broadcast_to(nc.planes(b), got[pad].shape)), tag
            valid = ~pad
            _, _, emu = nc.ln_emulate(xr, g, b, eps=EPS, fma=True)
            nc.check_rows(tag, got, nc.planes(emu), nc.ln64(xr, g, b, EPS)[2], True, edge == "constant" or C == 1, figs, valid)
    _report(figs)


LN_SHAPES = [(M, C) for C in (128, 256, 384, 512) for M in (33, 64, 130)]


def _linear_ln(L, x, w1, b1, res, g, b, w2, b2, fused):
    M, K = x.shape
    C, N = w1.shape[0], w2.shape[0]
    d = [None if a is None else _dev(a) for a in (x, w1, b1, res, g, b, w2, b2)]
    y1, rs, y2 = _nan((M, C)), _nan((M, C // 32, 2)), _nan((M, N))
    out = _twice(lambda: L.check(L.lib().dv_op_linear_ln(*[L.ptr(t) for t in d], M, K, C, N, fused, L.ptr(y1), L.ptr(rs), L.ptr(y2), None),
                                 "dv_op_linear_ln"), [y1, rs, y2])
    assert np.isnan(out[1]).all() if not fused else not np.isnan(out[1]).any()
    return out


@pytest.mark.parametrize("edge", ALL_EDGES)
@pytest.mark.parametrize("family", ["exact", "general"])
def test_linear_ln(family, edge):
    """The fused LayerNorm of the default schedule (producer partials, consumer combination, folded finish) and the DVITS_FUSE_LN=0
    route.  exact: the producer is a permutation, every operand dyadic - y1 is the permuted input bit for bit and what is left in y2
    is the statistic, its combination and fp32 accumulation.  Row partials: sum 9.5 units (17 additions), mean and rstd recombined on
    the host in fp64 from the GPU's words."""
    L = _L()
    figs, exact = {}, family == "exact"
    for M, C in LN_SHAPES:
        N = 96
        x = nc.edge_values(edge, (M, C), "ln.%d.%d" % (M, C), dyadic=exact)
        p, w1, b1 = nc.producer(C, exact)
        res = None if exact else (0.25 * nc._normal("ln.res.%d.%d" % (M, C), (M, C))).astype(F32)
        g, b = nc.affine(C, "signs" if M == 64 else "plain", dyadic=exact)
        w2, b2 = nc.consumer(N, C, exact)
        for fused in (1, 0):
            tag = "linear_ln %s %s M=%d C=%d fused=%d" % (family, edge, M, C, fused)
            y1, rs, y2 = _linear_ln(L, x, w1, b1, res, g, b, w2, b2, fused)
            assert not np.isnan(y1).any() and not np.isnan(y2).any(), tag
            if exact:
                assert np.array_equal(y1, x[:, p]), tag
            const = edge == "constant" and exact
            if fused:
                blk = y1.astype(F64).reshape(M, C // 32, 32)
                nc.check_words(tag + " rowstat", rs, blk, nc.DEPTH["rowstat"], figs)
                w = rs.astype(F64)
                mean = w[..., 0].sum(-1) / C
                m2 = (w[..., 1] + 32.0 * (w[..., 0] / 32.0 - mean[:, None]) ** 2).sum(-1)
                nc.check_stats(tag + " rowstat", mean, 1.0 / np.sqrt(m2 / C + EPS), blk, EPS, nc.DEPTH["rowstat"], figs)
            emu = nc.linear_ln_emulate(y1, g, b, w2, b2, fused=bool(fused), eps=EPS)
            nc.check_rows(tag + " y2", y2, emu, nc.linear_ln64(y1, g, b, w2, b2, EPS), False, const, figs)
    _report(figs)


GN_SHAPES = [(C, T, Tp) for C in (128, 256) for (T, Tp) in ((64, 64), (40, 64), (33, 64))]


def _linear_gn(L, x, w, b, g, be, B, T, Tp, G, route):
    K, C = x.shape[-1], w.shape[0]
    d = [None if a is None else _dev(a) for a in (x, w, b, g, be)]
    nst = (B * Tp // 32) * (C if route == L.GN_SLAB else C // 16) * 2
    y, st, hi, lo = _nan((B, Tp, C)), _nan((nst,)), _planes_buf((B, Tp, C)), _planes_buf((B, Tp, C))
    yh, sth, hb, lb = _twice(lambda: L.check(L.lib().dv_op_linear_gn(*[L.ptr(t) for t in d], B, T, Tp, K, C, G, EPS, route, L.ptr(y), L.ptr(st),
                                                                     L.ptr(hi), L.ptr(lo), None), "dv_op_linear_gn"), [y, st, hi, lo])
    return yh, sth, nc.from_planes(hb.view(np.uint16), lb.view(np.uint16))


@pytest.mark.parametrize("edge", ALL_EDGES + ["two-offsets"])
@pytest.mark.parametrize("route", ["stat16", "slab", "kstat16"])
@pytest.mark.parametrize("family", ["exact", "general"])
def test_linear_gn(family, route, edge):
    """GroupNorm behind a k = 1 GEMM in the padded row space: the epilogue's 32x16 block statistics (padded-row form included), the
    column slab, the standalone k_stat16, and k_gn_apply's fp64 reduction of each.  Block sums: 8 units (14 additions; the slab 4.5),
    group mean / rstd recombined on the host in fp64 from the GPU's words with the parallel-variance formula."""
    L = _L()
    figs, exact = {}, family == "exact"
    rid = {"stat16": L.GN_STAT16, "slab": L.GN_SLAB, "kstat16": L.GN_KSTAT16}[route]
    B, G = 2, 8
    for C, T, Tp in GN_SHAPES:
        if route != "stat16" and T != Tp:
            continue
        x = nc.group_values(edge, B, T, Tp, C, G, "gn.%d.%d" % (C, T), dyadic=exact)
        p, w, b = nc.producer(C, exact)
        g, be = nc.affine(C, "signs" if T == 40 or C == 256 else "plain", dyadic=exact)
        tag = "linear_gn %s %s %s C=%d T=%d/%d" % (family, route, edge, C, T, Tp)
        y, st, yn = _linear_gn(L, x, w, b, g, be, B, T, Tp, G, rid)
        assert not y[:, T:].any() and not np.isnan(y).any() and not np.isnan(yn).any() and not np.isnan(st).any(), tag
        if exact:
            assert np.array_equal(y[:, :T], x[:, :T][:, :, p]), tag
        cols = 1 if route == "slab" else 16
        words = st.reshape(B, Tp // 32, C // cols, 2)
        cnt = nc._counts(T, Tp).astype(int)
        yb = nc._blocks(y.astype(F64), cols)
        for rb in range(Tp // 32):
            blk = yb[:, rb, :, :cnt[rb], :].reshape(B, C // cols, -1)
            nc.check_words("%s block row %d" % (tag, rb), words[:, rb], blk, nc.DEPTH["slab" if route == "slab" else "stat16"], figs, route == "slab")
        mean, rstd = nc.words_to_group_stats(words, T, Tp, G, cols, EPS)
        nc.check_group_stats(tag + " words", mean, rstd, y, T, G, cols, EPS, nc.DEPTH["slab" if route == "slab" else "stat16"], figs)
        emu_words = nc.block_words_emulate(y, T, cols)
        m_e, r_e = nc.block_words_combine(emu_words, T, Tp, G, cols, EPS)
        emu = nc.planes(nc.gn_apply_emulate(y, m_e, r_e, g, be))
        want = nc.gn64(y, T, G, g, be, EPS)[2]
        valid = np.arange(Tp)[None, :].repeat(B, 0) < T
        nc.check_rows(tag + " y_norm", yn, emu, want, True, edge == "constant" and exact, figs, valid)
        if T < Tp:      # padding rows: the affine of a zero row, as documented - absolutely (they have no norm of their own to divide by)
            nc.check_rows(tag + " y_norm padding", yn, emu, want, True, True, figs, ~valid)
    _report(figs)
