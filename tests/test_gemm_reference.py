"""CPU: what the criteria of tests/gemm_cases.py can and cannot see, and what dv_op_gemm refuses before it launches anything.
tools/gemm_reference.py plants faults in the host emulation of k_gemm's arithmetic and sends the results through the assertions the
GPU results go through (tests/test_gpu_gemm_ops.py); profiles/gemm_reference.txt is its output.  Every planted fault breaks a
criterion at a committed case, in each operand mode it can occur in; the unfaulted float32 accumulation - in k order and cut into two
k-groups - stays inside every criterion at every case."""
import ctypes as C
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gemm_cases as gc  # noqa: E402
import gemm_reference as gr  # noqa: E402
from diff_vits_amd import _lib  # noqa: E402


@pytest.fixture(scope="module")
def table():
    return gr.table()


def test_every_planted_fault_breaks_a_criterion(table):
    res, lines = table
    print("\n".join(lines))
    assert {f for f, _ in res} == {"drop_lohi", "trunc", "drop_last_ktile", "dup_ktile", "drop_kgroup_half", "src1_offset",
                                   "mask_before_bias", "geglu_swap"}
    assert set(res) == set(gc.FIRST_SEEN)
    for key, (hit, ratio) in res.items():
        assert hit is not None and hit == gc.FIRST_SEEN[key], (key, hit, ratio)
        assert ratio >= 5.0, (key, ratio)              # far outside, not at the edge of a bound


def test_correct_arithmetic_stays_inside():
    rows = gr.correct_stays_inside()
    assert len(rows) == 4 * len(gc.CASES)
    for name, ns, order, crit, r in rows:
        assert r <= 1.0, (name, ns, order, crit, r)
    # the k-group cut is another summation order, not the yardstick itself: it must differ from it somewhere and stay well inside
    assert max(r for _, _, order, crit, r in rows if order == "two k-groups" and crit == "row") <= 0.5


def test_profile_is_the_tools_output(table):
    want = open(os.path.join(ROOT, "profiles", "gemm_reference.txt")).read().splitlines()
    assert [l for l in want if not l.startswith("#")] == table[1]


def test_case_list_reaches_the_edges():
    ks = {c["K"] for c in gc.CASES}
    assert {32, 64, 96, 192, 320, 1536} <= ks and max(k for k in ks if k != 1536) <= gc.ELEMENT_MAX_K
    for bm in (32, 64, 128):
        assert {1, bm - 1, bm + 1, 2 * bm + 3} <= {c["M"] for c in gc.CASES}
        assert {8, 17, bm + 1, 2 * bm} <= {c["N"] for c in gc.CASES}
    assert {(c["K0"], c["K"] - c["K0"]) for c in gc.CASES if c["K0"]} >= {(64, 64), (32, 96)}
    assert {c["splitk"] for c in gc.CASES} == {0, 2, 3, 2 | gc.SPLITK_FUSED}
    assert all(c["K"] == 1536 for c in gc.CASES if c["splitk"])
    assert any(c["epi"] == gc.RESIDUAL and c["ldres"] != c["N"] for c in gc.CASES)
    assert any(c["epi"] == gc.GEGLU and c["ldo"] % 4 for c in gc.CASES)
    assert {"offset30", "exact"} <= {c["values"] for c in gc.CASES}


# ---- the library's own account of what it would launch (host only: dv_op_gemm_variant runs dv_op_gemm's checks, launches nothing) ----
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def variant(lib, c, tile, nsplit):
    v, kind, ns = C.c_int32(), C.c_int32(), C.c_int32()
    rc = lib.dv_op_gemm_variant(c["M"], c["K"], c["N"], c["K0"], c["epi"], tile, c["splitk"], 0 if nsplit == 3 else 1,
                                C.byref(v), C.byref(kind), C.byref(ns))
    return rc, (v.value, kind.value, ns.value)


def test_cases_cover_every_instantiation(lib):
    """The set of (variant id, menu entry, NSPLIT) over the case list, as the library reports it, is the whole menu kernels_gemm.hip
    builds: Tiles<32> has nine entries (T0 two k-groups, T0S, T1, T2, T2S, T2G, T3, T4, T4G: one k-group), Tiles<64> seven (T0 / T0S
    are 32 deep only; T1, T2, T3, T4 on two k-groups, T2S, T2G, T4G on one), each in two operand modes: 32.  (T2 and T2S at BK = 32
    share one template instance: 30 distinct kernels.)"""
    want = gc.menu()
    assert len(want) == 32
    have, per = set(), {}
    for c in gc.CASES:
        for label, tile in gc.tiles_for(c):
            for ns in (3, 1):
                rc, got = variant(lib, c, tile, ns)
                assert rc == 0, (c["name"], label, lib.dv_last_error())
                have.add(got)
                if label != "auto" and c["splitk"] == 0 and c["K"] <= gc.ELEMENT_MAX_K:
                    per.setdefault(got, set()).add((c["M"], c["N"]))
    assert have == want, sorted(want ^ have)
    for (v, kind, ns), shapes in per.items():          # every instantiation: M and N on both sides of ITS tile, more than one tile
        bm, bn = v & 255, (v >> 8) & 255
        ms, nn = {m for m, _ in shapes}, {n for _, n in shapes}
        assert min(ms) < bm < max(ms) and max(ms) > 2 * bm and min(nn) < bn and max(nn) >= 2 * bn, (v, kind, ns, sorted(shapes))


def test_forced_variant_is_the_menu_entry(lib):
    c = gc.case("plain.65x65x192")
    for name, (bm, bn, kg32, kg64, _) in gc.TILES.items():
        assert variant(lib, c, gc.TILE_ID[name], 3) == (0, (gc.variant_id(bm, bn, 32, kg32), gc.TILE_ID[name], 3))
        if kg64 is not None:
            assert variant(lib, c, gc.TILE_ID[name] | gc.BK64, 1) == (0, (gc.variant_id(bm, bn, 64, kg64), gc.TILE_ID[name], 1))


REFUSED = [
    ("64-deep tile, K = 96", dict(M=64, K=96, N=64, tile=gc.TILE_ID["T2"] | gc.BK64), b"multiples of 64"),
    ("64-deep tile, sources 32 + 96", dict(M=64, K=128, N=64, K0=32, tile=gc.TILE_ID["T3"] | gc.BK64), b"multiples of 64"),
    ("128x128 tile 64 deep", dict(M=64, K=128, N=64, tile=gc.TILE_ID["T0"] | gc.BK64), b"32-deep"),
    ("K0 not a multiple of 32", dict(M=64, K=128, N=64, K0=48), b"multiples of 32"),
    ("K0 = K", dict(M=64, K=128, N=64, K0=128), b"K0"),
    ("K not a multiple of 32", dict(M=64, K=100, N=64), b"multiples of 32"),
    ("GEGLU on a tile without a 64-column block per wave", dict(M=64, K=64, N=128, epi=gc.GEGLU, tile=gc.TILE_ID["T2"]), b"64-column block"),
    ("GEGLU with N % 64 != 0", dict(M=64, K=64, N=96, epi=gc.GEGLU), b"N % 64"),
    ("split-K with GEGLU", dict(M=64, K=1536, N=128, epi=gc.GEGLU, splitk=2), b"split-K"),
    ("four slices", dict(M=64, K=1536, N=64, splitk=4), b"splitk"),
    ("three fused slices", dict(M=64, K=1536, N=64, splitk=3 | gc.SPLITK_FUSED), b"splitk"),
    ("more slices than k-tiles", dict(M=64, K=128, N=64, splitk=3), b"fewer"),
    ("unknown tile", dict(M=64, K=64, N=64, tile=10), b"tile"),
    ("BK64 without a tile", dict(M=64, K=64, N=64, tile=gc.BK64), b"tile"),
    ("unknown epilogue", dict(M=64, K=64, N=64, epi=3), b"epilogue"),
    ("unknown precision", dict(M=64, K=64, N=64, precision=2), b"precision"),
    ("no rows", dict(M=0, K=64, N=64), b"rows"),
]


@pytest.mark.parametrize("what,args,msg", REFUSED, ids=[r[0] for r in REFUSED])
def test_unsupported_combinations_are_refused_before_launch(lib, what, args, msg):
    a = dict(K0=0, epi=gc.STORE, tile=0, splitk=0, precision=0)
    a.update(args)
    v, kind, ns = C.c_int32(-7), C.c_int32(-7), C.c_int32(-7)
    rc = lib.dv_op_gemm_variant(a["M"], a["K"], a["N"], a["K0"], a["epi"], a["tile"], a["splitk"], a["precision"],
                                C.byref(v), C.byref(kind), C.byref(ns))
    assert rc == -1 and msg in lib.dv_last_error(), (what, rc, lib.dv_last_error())
    assert (v.value, kind.value, ns.value) == (-7, -7, -7)
    # dv_op_gemm makes the same checks first: with these arguments it returns before it looks at a pointer or touches the device
    rc = lib.dv_op_gemm(None, None, None, None, None, None, None, None, a["M"], a["K"], a["N"], a["K0"], a["N"], 0, a["epi"], 0,
                        a["tile"], a["splitk"], a["precision"], None)
    assert rc == -1 and msg in lib.dv_last_error(), (what, rc, lib.dv_last_error())
