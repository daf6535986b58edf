"""GPU: every k_gemm instantiation, in both operand modes, at tile edges, through dv_op_gemm.  Cases, host emulation, bounds and the
assertions themselves: tests/gemm_cases.py (what those criteria can and cannot see: tests/test_gemm_reference.py,
profiles/gemm_reference.txt; measured figures: profiles/gemm_ops_parity.txt).  Every case runs on the heuristic's tile and on every
forced tile that can run it; no environment knob is touched.  Every output buffer is pre-filled with NaN (0x7fc1 in the planes) and
has guard rows behind row M, every launch is made twice and must return the same bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import gemm_cases as gc

pytestmark = pytest.mark.gpu
GUARD = 3           # rows behind row M that nothing may write
FILL = 0x7fc1       # a bf16 NaN pattern no result can take
_SEEN = {}          # (variant id, menu entry, NSPLIT) -> [worst element / bound, worst row / cpu32 row] over every launch of this module
_AUTO = {}          # (case, NSPLIT) -> the heuristic tile's result


def _L():
    from diff_vits_amd import _lib as L
    return L


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _variant(L, c, tile, ns):
    v, kind, n = C.c_int32(), C.c_int32(), C.c_int32()
    L.check(L.lib().dv_op_gemm_variant(c["M"], c["K"], c["N"], c["K0"], c["epi"], tile, c["splitk"], 0 if ns == 3 else 1,
                                       C.byref(v), C.byref(kind), C.byref(n)), "dv_op_gemm_variant")
    assert n.value == ns
    return v.value, kind.value, n.value


def _run(L, c, dev, tile, ns, with_f32=True, with_planes=True):
    """One launch, twice: (y, hi, lo) host arrays [M + GUARD, ldo] (None where not asked for); lo is passed in both modes."""
    M, ldo = c["M"], c["ldo"]
    dx, dw, db, dr, dm = dev
    outs = []
    for _ in range(2):
        y = torch.full((M + GUARD, ldo), float("nan"), device="cuda") if with_f32 else None
        hi = torch.full((M + GUARD, ldo), FILL, dtype=torch.int32, device="cuda").to(torch.int16) if with_planes else None
        lo = hi.clone() if with_planes else None
        L.check(L.lib().dv_op_gemm(L.ptr(dx), L.ptr(dw), L.ptr(db), L.ptr(dr), L.ptr(dm), L.ptr(y), L.ptr(hi), L.ptr(lo), M, c["K"], c["N"],
                                   c["K0"], ldo, c["ldres"], c["epi"], c["relu"], tile, c["splitk"], 0 if ns == 3 else 1, None),
                "dv_op_gemm %s tile 0x%x" % (c["name"], tile))
        torch.cuda.synchronize()
        outs.append([None if t is None else t.cpu().numpy() for t in (y, hi, lo)])
    for a, b in zip(*outs):
        assert (a is None and b is None) or a.tobytes() == b.tobytes(), "%s: two calls differ" % c["name"]
    y, hi, lo = outs[1]
    return y, (None if hi is None else hi.view(np.uint16)), (None if lo is None else lo.view(np.uint16))


def _check_launch(L, c, dev, label, tile, ns, exp):
    """Every criterion of one (case, tile, operand mode); returns the fp32 result [M, n_out]."""
    M, N = c["M"], c["N"]
    n_out = N // 2 if c["epi"] == gc.GEGLU else N
    tag = "%s %s NSPLIT=%d" % (c["name"], label, ns)
    y, hi, lo = _run(L, c, dev, tile, ns)
    # nothing beyond column n_out of a row, nothing in the guard rows
    assert np.isnan(y[:M, n_out:]).all() and np.isnan(y[M:]).all(), tag + ": fp32 written outside [M, n_out]"
    assert (hi[:M, n_out:] == FILL).all() and (hi[M:] == FILL).all(), tag + ": hi plane written outside [M, n_out]"
    got = y[:M, :n_out]
    j = gc.check(tag, exp, got)
    # the planes are the split of the fp32 result of the same launch; bf16 mode leaves y_lo alone
    want_hi, want_lo = gc.planes_of(got)
    assert np.array_equal(hi[:M, :n_out], want_hi), tag + ": hi plane is not bf16_rne(y)"
    if ns == 3:
        assert np.array_equal(lo[:M, :n_out], want_lo), tag + ": lo plane is not bf16_rne(y - hi)"
        assert (lo[:M, n_out:] == FILL).all() and (lo[M:] == FILL).all(), tag + ": lo plane written outside [M, n_out]"
    else:
        assert (lo == FILL).all(), tag + ": y_lo touched in bf16 mode"
    key = _variant(L, c, tile, ns)
    s = _SEEN.setdefault(key, [0.0, 0.0])
    s[0] = max(s[0], j.get("element", 0.0))
    s[1] = max(s[1], 4.0 * j["row"])
    return got, key


@pytest.mark.parametrize("ns", [3, 1], ids=["bf16x3", "bf16"])
@pytest.mark.parametrize("name", gc.CASE_NAMES)
def test_gemm_case(name, ns):
    """One case of tests/gemm_cases.py on the heuristic's tile and on every forced tile that can run it: element-wise and per-row
    against the host emulation, whole tensor against fp64, bit-equal across two calls, planes = the split of y, no write outside
    [M, n_out], and every tile inside the sum of both element bounds of the heuristic's tile."""
    L = _L()
    c = gc.case(name)
    exp = gc.Expected.of(c, ns)
    dev = tuple(_dev(a) for a in gc.inputs(c))
    y_auto = None
    for label, tile in gc.tiles_for(c):
        got, _ = _check_launch(L, c, dev, label, tile, ns, exp)
        if label == "auto":
            y_auto = _AUTO[(name, ns)] = got
        else:
            r = gc.check_agreement("%s %s NSPLIT=%d" % (name, label, ns), exp, got, y_auto)
            print("gemm_ops %-44s agreement with the heuristic's tile: %.3f of the two element bounds" % ("%s %s NSPLIT=%d" % (name, label, ns), r))


@pytest.mark.parametrize("ns", [3, 1], ids=["bf16x3", "bf16"])
@pytest.mark.parametrize("name", ["geglu.129x256x192.al", "plain.131x128x320", "res.65x72x192", "plain.33x17x96"])
def test_gemm_planes_only(name, ns):
    """Planes without the fp32 output take other store paths (16-byte plane stores where N and the pitch allow, store_planes16 in the
    GEGLU epilogue): bit-equal to the planes of the launch that also wrote fp32; fp32 alone equals it too."""
    L = _L()
    c = gc.case(name)
    dev = tuple(_dev(a) for a in gc.inputs(c))
    for label, tile in gc.tiles_for(c):
        y, hi, lo = _run(L, c, dev, tile, ns)
        _, hi2, lo2 = _run(L, c, dev, tile, ns, with_f32=False)
        y3, _, _ = _run(L, c, dev, tile, ns, with_planes=False)
        tag = "%s %s NSPLIT=%d" % (name, label, ns)
        assert np.array_equal(hi, hi2) and np.array_equal(lo, lo2), tag + ": planes-only launch differs"
        assert y.tobytes() == y3.tobytes(), tag + ": fp32-only launch differs"


def test_exact_operands_agree_across_modes():
    """Operands that are exact in bf16 have zero lo planes: both modes sum the same products, the emulations are equal and the two
    results agree inside the sum of their element bounds."""
    L = _L()
    c = gc.case("exact.65x65x192")
    e3, e1 = gc.Expected.of(c, 3), gc.Expected.of(c, 1)
    assert np.array_equal(e3.emu, e1.emu) and np.array_equal(e1.emu, e1.ref)
    dev = tuple(_dev(a) for a in gc.inputs(c))
    for label, tile in gc.tiles_for(c):
        y3 = _run(L, c, dev, tile, 3)[0][:c["M"], :c["N"]].astype(np.float64)
        y1 = _run(L, c, dev, tile, 1)[0][:c["M"], :c["N"]].astype(np.float64)
        r = float((np.abs(y3 - y1) / (e3.bound + e1.bound)).max())
        print("gemm_ops exact %-8s bf16 vs bf16x3: %.3f of the two element bounds" % (label, r))
        assert r <= 1.0, (label, r)


def test_offset_operands_use_the_lo_planes():
    """The 30 sigma case is only a test of the lo planes if they matter there: the single-bf16 emulation is >= 100 x further from
    fp64 than the split one."""
    c = gc.case("offset30.65x65x192")
    assert gc.Expected.of(c, 1).emu_ref > 100 * gc.Expected.of(c, 3).emu_ref


def test_refusals_come_before_the_launch():
    """With real buffers: a refused call leaves every output byte as it was."""
    L = _L()
    c = gc.case("plain.65x65x192")
    dx, dw, db, _, _ = (_dev(a) for a in gc.inputs(c))
    y = torch.full((c["M"], c["N"]), float("nan"), device="cuda")
    for kw in (dict(tile=gc.TILE_ID["T0"] | gc.BK64), dict(epi=gc.GEGLU), dict(splitk=4), dict(ldo=c["N"] - 1), dict(res=True), dict(relu=2)):
        a = dict(tile=0, epi=gc.STORE, splitk=0, ldo=c["N"], res=False, relu=0)
        a.update(kw)
        rc = L.lib().dv_op_gemm(L.ptr(dx), L.ptr(dw), L.ptr(db), L.ptr(dx) if a["res"] else None, None, L.ptr(y), None, None, c["M"], c["K"],
                                c["N"], 0, a["ldo"], 0, a["epi"], a["relu"], a["tile"], a["splitk"], 0, None)
        assert rc == -1 and L.lib().dv_last_error(), kw
        torch.cuda.synchronize()
        assert torch.isnan(y).all(), kw


def test_zz_every_instantiation_ran():
    """Runs last in this module: what the launches above really ran on, as dv_op_gemm_variant reports it, is the whole menu; the worst
    figures per instantiation are printed for profiles/gemm_ops_parity.txt."""
    L = _L()
    for c in gc.CASES[:len(gc.SHAPES)]:               # (selected alone, this test makes the launches itself: first case per entry)
        for label, tile in gc.tiles_for(c):
            for ns in (3, 1):
                if _variant(L, c, tile, ns) not in _SEEN:
                    _check_launch(L, c, tuple(_dev(a) for a in gc.inputs(c)), label, tile, ns, gc.Expected.of(c, ns))
    names = {v: k for k, v in gc.TILE_ID.items()}
    for (v, kind, ns), (el, row) in sorted(_SEEN.items()):
        print("gemm_ops instantiation %3dx%-3d BK=%d k-groups=%d %-3s NSPLIT=%d  worst element / bound %.3f  worst row / cpu32 row %.2f" % (
            v & 255, (v >> 8) & 255, (v >> 16) & 255, v >> 24, names[kind], ns, el, row))
    assert set(_SEEN) == gc.menu(), sorted(set(_SEEN) ^ gc.menu())
