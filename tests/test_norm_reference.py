"""CPU: what the bounds of tests/norm_cases.py can and cannot see.  tools/norm_reference.py runs float32 emulations of the correct
arithmetic (summed in another order than the emulation that sets the bound) and of planted faults through the assertions the GPU
results go through (tests/test_gpu_norm_ops.py); profiles/norm_reference.txt is its output.

Every planted fault is seen at >= 5 x its bound at a point the GPU test runs; none stays out of reach.  The figure the issue of this
test also asked for - the correct arithmetic inside a THIRD of the bound at that point - does not hold everywhere and cannot: the row
bound is 2 x the emulation's own worst row, so arithmetic whose rounding error equals the emulation's sits at 0.5 (the exact-operand
fused LayerNorm: every partial sum is exact, both orders give the same bits).  What is asserted is that it stays inside the bound
with the margin measured: <= 0.65 everywhere."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import norm_cases as nc  # noqa: E402
import norm_reference as nr  # noqa: E402


@pytest.fixture(scope="module")
def table():
    return nr.table()


def test_every_fault_is_seen_where_recorded(table):
    res, lines = table
    print("\n".join(lines))
    assert set(res) == set(nc.FIRST_SEEN)
    for key, (hit, ratio, _) in res.items():
        assert hit == nc.FIRST_SEEN[key], (key, hit, ratio)
        assert ratio >= 5.0, (key, ratio)


def test_recorded_points_are_gpu_cases():
    import test_gpu_norm_ops as t
    assert set(nc.FIRST_SEEN.values()) <= set(t.ALL_EDGES)


def test_correct_arithmetic_stays_inside(table):
    for route in nr.ROUTE_FAULTS:
        for p in nr.POINTS:
            r, at = nr.judge(route, p, None, True)
            assert r <= 0.65, (route, p, r, at)


def test_profile_is_the_tools_output(table):
    want = open(os.path.join(ROOT, "profiles", "norm_reference.txt")).read().splitlines()
    assert [l for l in want if not l.startswith("#")] == table[1]
