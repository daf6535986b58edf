"""What the criteria of tests/gemm_cases.py can and cannot see (CPU).  Faults are planted in the host emulation of k_gemm's arithmetic
(float32 accumulation of the plane products, as a kernel would run them) and the faulted results go through the assertions the GPU
results go through (tests/test_gpu_gemm_ops.py).  Per fault and operand mode: the first case of the committed list, in list order, at which a
criterion breaks, which one, and by how much.  The unfaulted float32 accumulation - in k order, and cut into two k-groups as the
64-deep tiles cut it - must stay inside every criterion at every case.
  python tools/gemm_reference.py > profiles/gemm_reference.txt"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import diff_vits_amd  # noqa: E402,F401
import gemm_cases as gc  # noqa: E402

# fault -> (what it is, the cases it can show at, NSPLITs, k-tile depths)
FAULTS = {
    "drop_lohi": ("the lo.hi product dropped", lambda c: True, (3,), (32,)),
    "trunc": ("operand split truncated instead of rounded to nearest", lambda c: c["values"] != "exact", (3, 1), (32,)),
    "drop_last_ktile": ("the last k-tile dropped", lambda c: True, (3, 1), (32, 64)),
    "dup_ktile": ("one k-tile added twice", lambda c: True, (3, 1), (32, 64)),
    "drop_kgroup_half": ("odd k-tile count: the second k-group's half of the last tile dropped", lambda c: (c["K"] // 64) % 2 == 1 and c["K"] % 64 == 0, (3, 1), (64,)),
    "src1_offset": ("source 1 read at source 0's column offset", lambda c: c["K0"] > 0, (3, 1), (32,)),
    "mask_before_bias": ("the row mask applied before the bias and the ReLU", lambda c: c["mask"], (3, 1), (32,)),
    "geglu_swap": ("GEGLU gate and value columns swapped", lambda c: c["epi"] == gc.GEGLU, (3, 1), (32,)),
}


def faulted(c, nsplit, fault, bk):
    x, w, b, res, mask = gc.inputs(c)
    if c["K"] % bk != 0:
        return None
    acc = gc.accumulate(c, x, w, nsplit, f32=True, fault=fault, bk=bk)
    return gc.epilogue(c, acc, b, res, mask, fault=fault)


def kgroup_order(c, nsplit):
    """The unfaulted sums cut as a 64-deep tile with two k-groups cuts them: each group its 32 columns of every tile, added at the end."""
    x, w, b, res, mask = gc.inputs(c)
    K = c["K"]
    cols = np.arange(K)
    g0, g1 = cols[(cols // 32) % 2 == 0], cols[(cols // 32) % 2 == 1]
    acc = np.zeros((c["M"], c["N"]), dtype=np.float32)
    for g in (g0, g1):
        if len(g):
            acc = acc + gc.accumulate(dict(c, K=len(g)), x[:, g], w[:, g], nsplit, f32=True)
    return gc.epilogue(c, acc, b, res, mask)


def worst(j):
    k = max(j, key=lambda n: j[n])
    return k, j[k]


def first_seen(fault, ns):
    _, applies, _, bks = FAULTS[fault]
    for c in gc.CASES:
        if not applies(c):
            continue
        for bk in bks:
            y = faulted(c, ns, fault, bk)
            if y is None:
                continue
            crit, r = worst(gc.judge(gc.Expected.of(c, ns), y))
            if r > 1.0:
                return (c["name"], bk, crit), r
    return None, 0.0


def table():
    res, lines = {}, []
    for fault, (what, _, nsplits, _) in FAULTS.items():
        for ns in nsplits:
            hit, r = first_seen(fault, ns)
            res[(fault, ns)] = (hit, r)
            lines.append("%-17s NSPLIT=%d %-73s first seen: %s  at %.3g x its bound" % (
                fault, ns, what, "NOWHERE" if hit is None else "%s BK=%d %s" % hit, r))
    return res, lines


def correct_stays_inside():
    """[(case, NSPLIT, order, criterion, ratio)] the worst criterion of the unfaulted float32 sums at every case."""
    out = []
    for c in gc.CASES:
        for ns in (3, 1):
            exp = gc.Expected.of(c, ns)
            for order, y in (("k order", exp.cpu32), ("two k-groups", kgroup_order(c, ns))):
                crit, r = worst(gc.judge(exp, y))
                out.append((c["name"], ns, order, crit, r))
    return out


if __name__ == "__main__":
    print("# tools/gemm_reference.py: planted faults against the criteria of tests/gemm_cases.py")
    for line in table()[1]:
        print(line)
    rows = correct_stays_inside()
    w = max(rows, key=lambda r: r[4])
    print("# unfaulted float32 accumulation, %d (case, NSPLIT, order) points: worst %.3f of a bound (%s NSPLIT=%d, %s, %s)" % (
        len(rows), w[4], w[0], w[1], w[2], w[3]))
