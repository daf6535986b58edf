"""GPU: k_gemm's convolution operand path (gemm_tile.h prep_a / advance / utt_of) through dv_op_conv_rows, strict per element and per
frame.  Cases, restated gather, emulation, bounds and assertions: tests/conv_rows_cases.py (what they can and cannot see:
tests/test_conv_rows_reference.py; measured figures: profiles/conv_rows_parity.txt).  Every case runs on the heuristic's tile and on
every forced tile the prepare-time tuner would try on it; four cases run the whole menu.  Every output buffer is pre-filled with NaN
(0x7fc1 in the planes) and has guard rows behind row B x Tp_out; the input padding rows hold 3e4 sigma garbage."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_rows_cases as cr
import gemm_cases as gc

pytestmark = pytest.mark.gpu
GUARD = 3           # rows behind the last output row that nothing may write
FILL = 0x7fc1       # a bf16 NaN pattern no result can take
_SEEN = {}          # (variant id, menu entry, NSPLIT) -> {mode: worst element / bound} over every launch of this module


def _L():
    from diff_vits_amd import _lib as L
    return L


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _shape(c, nb=cr.B):
    return [nb, c["T"], c["Tp_in"], c["c0"], c["c1"], c["c_sc"], c["Cout"], c["taps"], c["stride"], c["up"], c["up_T"], c["Tp_out"]]


def _variant(L, c, tile, ns):
    """((variant id, menu entry, NSPLIT), [candidate tiles]) as the library reports them (host only)."""
    v, kind, n = C.c_int32(), C.c_int32(), C.c_int32()
    cand = (C.c_int32 * 8)()
    L.check(L.lib().dv_op_conv_rows_variant(*_shape(c), tile, 0 if ns == 3 else 1, C.byref(v), C.byref(kind), C.byref(n), cand, 8),
            "dv_op_conv_rows_variant")
    assert n.value == ns
    return (v.value, kind.value, n.value), [t for t in cand if t]


def _run(L, c, dev, tile, ns, nb=cr.B, stats=None):
    """One launch: y [nb, Tp_out (+ GUARD rows behind the last utterance), Cout] float32, hi, lo planes (uint16) and the stats16 words."""
    rows, N = nb * c["Tp_out"], c["Cout"]
    stats = c["stats"] if stats is None else stats
    y = torch.full((rows + GUARD, N), float("nan"), device="cuda")
    hi = torch.full((rows + GUARD, N), FILL, dtype=torch.int32, device="cuda").to(torch.int16)
    lo = hi.clone()
    st = torch.full((rows // 32 + 1, N // 16, 2), float("nan"), device="cuda") if stats else None
    x0, x1, w, b, xs, ws = dev
    L.check(L.lib().dv_op_conv_rows(L.ptr(x0), L.ptr(x1), L.ptr(w), L.ptr(b), L.ptr(xs), L.ptr(ws), L.ptr(y), L.ptr(hi), L.ptr(lo), L.ptr(st),
                                    *_shape(c, nb), tile, 0 if ns == 3 else 1, None), "dv_op_conv_rows %s tile 0x%x" % (c["name"], tile))
    torch.cuda.synchronize()
    return (y.cpu().numpy(), hi.cpu().numpy().view(np.uint16), lo.cpu().numpy().view(np.uint16), None if st is None else st.cpu().numpy())


def _check_launch(L, c, dev, label, tile, ns, exp, twice=False):
    """Every criterion of one (case, tile, operand mode); returns the valid rows [B x Tv_out, Cout] of the fp32 result."""
    rows, N, Tv = cr.B * c["Tp_out"], c["Cout"], c["Tv_out"]
    tag = "%s %s NSPLIT=%d" % (c["name"], label, ns)
    key, _ = _variant(L, c, tile, ns)
    y, hi, lo, st = _run(L, c, dev, tile, ns)
    if twice:
        for a, b in zip((y, hi, lo, st), _run(L, c, dev, tile, ns)):
            assert a is None or a.tobytes() == b.tobytes(), tag + ": two calls differ"
    assert np.isnan(y[rows:]).all() and (hi[rows:] == FILL).all(), tag + ": written behind the last row"
    words = None
    if st is not None:
        assert np.isnan(st[rows // 32:]).all(), tag + ": stats16 written behind the last block"
        words = st[:rows // 32]
        assert np.isfinite(words).all(), tag + ": a stats16 word was not written"
    full = y[:rows].reshape(cr.B, c["Tp_out"], N)
    j = cr.check(tag, exp, full, words, bm=key[0] & 255)
    # the planes are the split of the fp32 result of the same launch (zeros in the padding rows); bf16 mode leaves y_lo alone
    want_hi, want_lo = gc.planes_of(y[:rows])
    assert np.array_equal(hi[:rows], want_hi), tag + ": hi plane is not bf16_rne(y)"
    if ns == 3:
        assert np.array_equal(lo[:rows], want_lo) and (lo[rows:] == FILL).all(), tag + ": lo plane is not bf16_rne(y - hi)"
    else:
        assert (lo == FILL).all(), tag + ": y_lo touched in bf16 mode"
    seen = _SEEN.setdefault(key, {})
    for m in cr.mode_of(c):
        seen[m] = max(seen.get(m, 0.0), j["element"])
    return full[:, :Tv].reshape(-1, N)


def _case_on_its_tiles(L, c, ns):
    exp = cr.Expected.of(c, ns)
    dev = tuple(_dev(a) for a in cr.inputs(c))
    _, cand = _variant(L, c, 0, ns)
    y_auto = None
    for label, tile in cr.tiles_for(c, cand):
        got = _check_launch(L, c, dev, label, tile, ns, exp, twice=label == "auto")
        if label == "auto":
            y_auto = got
        else:
            tag = "%s %s NSPLIT=%d" % (c["name"], label, ns)
            r = gc.check_agreement(tag, exp, got, y_auto)
            print("conv_rows %-40s agreement with the heuristic's tile: %.3f of the two element bounds" % (tag, r))


@pytest.mark.parametrize("ns", [3, 1], ids=["bf16x3", "bf16"])
@pytest.mark.parametrize("name", cr.CASE_NAMES)
def test_conv_rows_case(name, ns):
    """One case of tests/conv_rows_cases.py on the heuristic's tile, on every tile the tuner would try and (four cases) on the whole
    menu: element-wise and per frame against the host emulation, whole tensor against fp64, padding rows exactly zero, stats16 against
    fp64, planes = the split of y, nothing written behind the last row, and every tile inside the sum of both element bounds of the
    heuristic's tile."""
    _case_on_its_tiles(_L(), cr.case(name), ns)


@pytest.mark.parametrize("ns", [3, 1], ids=["bf16x3", "bf16"])
@pytest.mark.parametrize("name", ["s1.T31.p31.loud", "s2.T33.64|32", "up.26-44", "s1.T65.p96.sc32"])
def test_no_utterance_sees_its_neighbours(name, ns):
    """Bitwise: the utterances launched one by one (B = 1) on the same forced tile give the rows, and the stats16 words, of the
    launch that holds all of them."""
    L = _L()
    c = cr.case(name)
    x0, x1, w, b, xs, ws = cr.inputs(c)
    dev = tuple(_dev(a) for a in (x0, x1, w, b, xs, ws))
    Tp = c["Tp_out"]
    for tname in ("T2", "T4", "T0S"):
        tile = gc.TILE_ID[tname]
        y, hi, _, st = _run(L, c, dev, tile, ns)
        for u in range(cr.B):
            one = tuple(_dev(a) for a in (x0[u:u + 1], None if x1 is None else x1[u:u + 1], w, b, None if xs is None else xs[u:u + 1], ws))
            y1, hi1, _, st1 = _run(L, c, one, tile, ns, nb=1)
            tag = "%s %s NSPLIT=%d utterance %d" % (name, tname, ns, u)
            assert y[u * Tp:(u + 1) * Tp].tobytes() == y1[:Tp].tobytes(), tag + ": rows differ from the single launch"
            assert np.array_equal(hi[u * Tp:(u + 1) * Tp], hi1[:Tp]), tag
            if st is not None:
                assert st[u * Tp // 32:(u + 1) * Tp // 32].tobytes() == st1[:Tp // 32].tobytes(), tag + ": stats16 differ"


def test_refusals_come_before_the_launch():
    """With real buffers: a refused call leaves every output byte as it was."""
    import test_conv_rows_reference as ref
    L = _L()
    z = torch.zeros(1 << 18, device="cuda")
    y = torch.full((3 * 128, 80), float("nan"), device="cuda")
    for why in ("taps 2", "stride 3", "segment two with stride 2", "c0 not a multiple of 32", "c1 not a multiple of 32",
                "BK64 with a 32-wide source", "Tp_out < Tv_out", "up_T with stride 2"):
        a = dict(ref.GOOD)
        a.update(ref.REFUSED[why])
        rc = L.lib().dv_op_conv_rows(L.ptr(z), L.ptr(z) if a["c1"] else None, L.ptr(z), L.ptr(z), L.ptr(z) if a["c_sc"] else None,
                                     L.ptr(z) if a["c_sc"] else None, L.ptr(y), None, None, None, *[a[k] for k in ref.ORDER], None)
        assert rc == -1 and L.lib().dv_last_error(), why
        torch.cuda.synchronize()
        assert torch.isnan(y).all(), why
    # pointers that do not go with the shape
    g = [ref.GOOD[k] for k in ref.ORDER]
    assert L.lib().dv_op_conv_rows(L.ptr(z), L.ptr(z), L.ptr(z), None, None, None, L.ptr(y), None, None, None, *g, None) == -1     # x1 without c1
    assert L.lib().dv_op_conv_rows(L.ptr(z), None, L.ptr(z), None, None, None, None, None, None, None, *g, None) == -1             # no output
    torch.cuda.synchronize()
    assert torch.isnan(y).all()


def test_zz_covers_every_tile():
    """Runs last in this module: every entry of the menu (9 tiles 32 deep, 7 of them 64 deep, both operand modes), as
    dv_op_conv_rows_variant reports what the launches ran on, has run a stride-2, a size-upsampled and a two-source case; the worst
    element per mode and instantiation is printed for profiles/conv_rows_parity.txt."""
    L = _L()
    need = {"stride2", "size", "two-source"}
    if any(not need <= set(_SEEN.get(k, {})) for k in gc.menu()):     # (selected alone, this test makes the launches itself)
        for c in cr.CASES:
            if c["all_tiles"]:
                for ns in (3, 1):
                    _case_on_its_tiles(L, c, ns)
    names = {v: k for k, v in gc.TILE_ID.items()}
    for (v, kind, ns), modes in sorted(_SEEN.items()):
        print("conv_rows instantiation %3dx%-3d BK=%d k-groups=%d %-3s NSPLIT=%d  worst element / bound:  %s" % (
            v & 255, (v >> 8) & 255, (v >> 16) & 255, v >> 24, names[kind], ns,
            "  ".join("%s %.3f" % (m, modes[m]) for m in ("stride2", "size", "x2", "two-source", "segment2", "stride1") if m in modes)))
    assert set(_SEEN) >= gc.menu(), sorted(gc.menu() - set(_SEEN))
    for k in gc.menu():
        assert need <= set(_SEEN[k]), (k, sorted(_SEEN[k]))
