"""CPU: what the criteria of tests/conv_rows_cases.py can and cannot see, and what dv_op_conv_rows refuses before it launches anything.
The kernel runs in tests/test_gpu_conv_rows.py; here the restated gather is held against torch's own operators, the float32 CPU
route against every bound, and eleven faults of the row gather are planted in the emulation."""
import ctypes as C

import numpy as np
import pytest

import conv_rows_cases as cr
import gemm_cases as gc

F64 = np.float64


@pytest.mark.parametrize("name", cr.CASE_NAMES)
def test_restatement_is_conv1d_of_interpolate(name):
    """rows_of() + weight_rows() in fp64 = F.conv1d(F.interpolate(x, mode="nearest")) + the 1x1 segment, to 1e-12 of the largest value."""
    c = cr.case(name)
    a, b = cr.restatement(c), cr.reference(c)
    assert a.shape == b.shape == (cr.B, c["Tv_out"], c["Cout"])
    assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), np.abs(a - b).max() / np.abs(b).max()


def test_float_rule_pairs_are_what_they_claim():
    """ATen's float rule (nearest_index) is F.interpolate's choice on the CPU for every T < 130, T < U <= 4 T; the listed pairs are
    among those where the exact rational index differs; no legal pair makes the T - 1 clamp bind."""
    import torch
    import torch.nn.functional as F
    differ = set()
    for T in range(1, 130):
        ramp = torch.arange(T, dtype=torch.float32)[None, None]
        for U in range(T + 1, 4 * T + 1):
            t = np.arange(U)
            want = F.interpolate(ramp, size=U, mode="nearest")[0, 0].numpy().astype(np.int64)
            assert np.array_equal(cr.nearest_index(t, T, U), want), (T, U)
            assert np.array_equal(cr.nearest_index(t, T, U, "no_clamp"), want), (T, U)
            if not np.array_equal(cr.nearest_index(t, T, U, "nearest_rational"), want):
                differ.add((T, U))
    assert set(cr.FLOAT_RULE_PAIRS) <= differ
    for c in cr.CASES:
        if c["up"] == cr.UP_SIZE and (c["T"], c["up_T"]) not in cr.FLOAT_RULE_PAIRS:
            assert (c["T"], c["up_T"]) not in differ, c["name"]


@pytest.mark.parametrize("ns", [3, 1], ids=["bf16x3", "bf16"])
def test_cpu32_route_is_inside_every_bound(ns):
    """A float32 accumulation of the same products on the CPU passes every criterion of check(), on every case."""
    for c in cr.CASES:
        y = cr.result(c, ns, f32=True)
        cr.check("%s cpu32 NSPLIT=%d" % (c["name"], ns), cr.Expected.of(c, ns), y, cr.block_words(c, y) if c["stats"] else None)


def _first_miss(fault, ns):
    for c in cr.CASES:
        y = cr.result(c, ns, fault)
        try:
            cr.check("%s %s NSPLIT=%d" % (c["name"], fault, ns), cr.Expected.of(c, ns), y, cr.block_words(c, y) if c["stats"] else None)
        except cr.Miss as e:
            return c["name"], str(e)
    return None


# no_clamp is planted like the others but CANNOT show: floor((float)t * ((float)T / (float)U)) <= T - 1 for every t < U of every legal
# (T, U) (test_float_rule_pairs_are_what_they_claim walks them), and t >= U never reaches the index (T_virt bounds the gather first).
# The clamp is a guard, not arithmetic; the test below asserts that removing it changes no result bit.
@pytest.mark.parametrize("ns", [3, 1], ids=["bf16x3", "bf16"])
@pytest.mark.parametrize("fault", [f for f in cr.FAULTS if f != "no_clamp"])
def test_planted_fault_breaks_a_criterion(fault, ns):
    hit = _first_miss(fault, ns)
    print("conv_rows fault %-24s NSPLIT=%d first seen: %s" % (fault, ns, hit))
    assert hit is not None, "%s passes every criterion on every case" % fault


def test_missing_clamp_changes_nothing_on_legal_sizes():
    for c in cr.CASES:
        if c["up"] == cr.UP_SIZE:
            assert np.array_equal(cr.result(c, 3, "no_clamp"), cr.result(c, 3)), c["name"]


def test_unfaulted_emulation_passes():
    """(the other side of the planted faults: with no fault the emulation is at zero distance from itself)"""
    for c in cr.CASES:
        y = cr.result(c, 3)
        j = cr.check(c["name"] + " emu", cr.Expected.of(c, 3), y, cr.block_words(c, y) if c["stats"] else None)
        assert j["element"] == 0.0 and j["row"] == 0.0


# test_conv1d's shapes (tests/test_gpu_ops.py: Cin, T, Cout, k, stride, up_T) - one source, one segment, the unpadded row space
CONV1D_SHAPES = [(64, 50, 96, 3, 1, 0), (224, 256, 128, 3, 1, 0), (128, 64, 128, 1, 1, 0), (96, 37, 96, 3, 2, 0), (64, 19, 64, 3, 1, 37),
                 (64, 20, 64, 3, 1, 40), (128, 1024, 128, 3, 1, 0), (512, 16, 80, 3, 1, 0)]


def test_whole_tensor_bound_on_the_old_shapes_misses_single_frame_faults():
    """Why this file exists.  test_conv1d holds k_gemm's gather to a whole-tensor rel-L2 of 1e-4 on eight shapes in the unpadded row
    space.  Two faults that put ONE wrong frame into every utterance are planted on exactly those shapes: the exact-rational nearest
    index, and Tp_in bounding the gather where T should.  Both leave every result bit unchanged there - no listed (T, U) tells the
    two index rules apart, no listed shape has a padded pitch - so that test cannot see them; the list of this module does."""
    for fault in ("nearest_rational", "Tp_in_bounds"):
        worst = 0.0
        for cin, T, cout, k, stride, up_T in CONV1D_SHAPES:
            c = cr._case("conv1d", T, cin, cout, Tp_in=T, taps=k, stride=stride, up=cr.UP_SIZE if up_T else cr.UP_NONE, up_T=up_T)
            x0 = np.ones((cr.B, T, cin), dtype=np.float32) * np.arange(1, T + 1, dtype=np.float32)[None, :, None]
            a, b = cr.rows_of(c, x0, None, None, fault), cr.rows_of(c, x0, None, None)
            worst = max(worst, float(np.abs(a.astype(F64) - b).max()))
        print("conv_rows %-18s on test_conv1d's shapes: largest operand difference %.1f" % (fault, worst))
        assert worst == 0.0, fault
        assert _first_miss(fault, 3) is not None


# ---- refusals: host only (dv_op_conv_rows makes its shape checks before it looks at a pointer or touches the device) ----
GOOD = dict(B=3, T=33, Tp_in=64, c0=64, c1=0, c_sc=0, Cout=80, taps=3, stride=1, up_mode=0, up_T=0, Tp_out=64, tile=0, precision=0)
REFUSED = {
    "taps 2": dict(taps=2),
    "stride 3": dict(stride=3),
    "segment two with stride 2": dict(c_sc=32, stride=2, Tp_out=32),
    "segment two with upsampling": dict(c_sc=32, up_mode=cr.UP_X2, Tp_out=96),
    "c0 not a multiple of 32": dict(c0=80),
    "c1 not a multiple of 32": dict(c1=48),
    "c_sc not a multiple of 32": dict(c_sc=16),
    "BK64 with a 32-wide source": dict(c1=32, tile=gc.TILE_ID["T2"] | gc.BK64),
    "BK64 with a 32-wide second segment": dict(c_sc=32, tile=gc.TILE_ID["T2"] | gc.BK64),
    "Tp_out < Tv_out": dict(Tp_out=32),
    "up_T with stride 2": dict(stride=2, up_mode=cr.UP_SIZE, up_T=75, Tp_out=64),
    "up_T without DV_UP_SIZE": dict(up_T=75, Tp_out=96),
    "x2 with stride 2": dict(stride=2, up_mode=cr.UP_X2),
    "Tp_in < T": dict(Tp_in=32),
    "128x128 tile 64 deep": dict(tile=gc.TILE_ID["T0"] | gc.BK64),
    "precision": dict(precision=7),
}
ORDER = ("B", "T", "Tp_in", "c0", "c1", "c_sc", "Cout", "taps", "stride", "up_mode", "up_T", "Tp_out", "tile", "precision")


def args_of(kw):
    a = dict(GOOD)
    a.update(kw)
    return [a[k] for k in ORDER]


def _lib():
    from diff_vits_amd import _lib as L
    return L.lib()


def test_variant_query_accepts_the_good_shape():
    v, kind, n = C.c_int32(), C.c_int32(), C.c_int32()
    cand = (C.c_int32 * 8)()
    assert _lib().dv_op_conv_rows_variant(*args_of({}), C.byref(v), C.byref(kind), C.byref(n), cand, 8) == 0
    assert n.value == 3 and (v.value & 255) in (32, 64, 128) and 1 <= kind.value <= 9
    assert 0 < len([t for t in cand if t]) < 8


@pytest.mark.parametrize("why", list(REFUSED))
def test_refusals_need_no_device(why):
    lib = _lib()
    v, kind, n = C.c_int32(), C.c_int32(), C.c_int32()
    a = args_of(REFUSED[why])
    assert lib.dv_op_conv_rows_variant(*a, C.byref(v), C.byref(kind), C.byref(n), None, 0) == -1 and lib.dv_last_error(), why
    assert lib.dv_op_conv_rows(*([None] * 10), *a, None) == -1 and lib.dv_last_error(), why


def test_stats16_needs_whole_blocks():
    """stats16 is checked with the shape: Cout % 16, Tp_out = the frames rounded up to 32 - before any pointer is read."""
    lib = _lib()
    one = C.c_void_p(16)                        # (never dereferenced: the shape is refused first)
    for kw in (dict(Cout=17), dict(Tp_out=40), dict(Tp_out=96)):
        a = args_of(kw)
        assert lib.dv_op_conv_rows(None, None, None, None, None, None, None, None, None, one, *a, None) == -1 and lib.dv_last_error(), kw
