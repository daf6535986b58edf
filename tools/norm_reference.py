"""What the bounds of tests/norm_cases.py can and cannot see (CPU).  Per route of tests/test_gpu_norm_ops.py, the float32 emulation of
the CORRECT arithmetic - summed in another order than the emulation that sets the bound - and emulations of planted faults go through
the same assertions the GPU results go through.  Per fault: the smallest point of the offset grid (and the other value edges) at which
it exceeds its bound by at least 5 x, and whether the correct arithmetic stays inside a third of the bound there.
  python tools/norm_reference.py > profiles/norm_reference.txt"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import diff_vits_amd  # noqa: E402,F401
import norm_cases as nc  # noqa: E402

EPS = 1e-5
F64 = np.float64
POINTS = ["offset%d" % o for o in nc.OFFSET_GRID] + ["unit", "small-sigma", "outlier"]
# route -> the faults that route's arithmetic can have
ROUTE_FAULTS = {
    "ln_rows": ("var_e2", "no_eps"),
    "prompt_pre": ("var_e2", "no_eps", "mean_cpad"),
    "linear_ln": ("var_e2", "no_dm2", "no_eps"),
    "gn_stat16": ("var_e2", "no_eps", "pad32"),
    "gn_slab": ("slab_fp32", "no_eps"),
}


def _ratio(figs):
    """Largest (figure / its bound) over what one judged case recorded."""
    worst, at = 0.0, ""
    for k, v in figs.items():
        if k.endswith(" bound"):
            continue
        if k.endswith(" worst row"):
            b = figs[k[:-len(" worst row")] + " bound"]
        elif k.endswith(" rstd rel"):
            b = nc.RSTD_REL
        elif k.endswith(" units"):
            b = figs["_units_bound"]
        elif k.endswith(" M2 / tol"):
            b = 1.0
        else:
            continue
        r = v / b if b > 0 else (0.0 if v == 0 else float("inf"))
        if r > worst:
            worst, at = r, k
    return worst, at


def judge(route, edge, fault, reverse):
    """-> (largest figure / bound, which figure) of the route's assertions on the emulated outputs (exact-operand family)."""
    figs = {}
    nc.REVERSED = reverse
    try:
        out = _outputs(route, edge, fault)
    finally:
        nc.REVERSED = False
    try:
        _assertions(route, edge, out, figs)
    except nc.Miss:
        pass
    return _ratio(figs)


def _inputs(route, edge):
    if route == "ln_rows":
        M, C = 130, 512
        return dict(x=nc.edge_values(edge, (M, C), "ref.rows"), gb=nc.affine(C, "signs"))
    if route == "prompt_pre":
        return dict(x=nc.edge_values(edge, (99, 100), "ref.prompt"), gb=nc.affine(100, "signs"))
    if route == "linear_ln":
        M, C, N = 130, 512, 96
        return dict(y1=nc.edge_values(edge, (M, C), "ref.ln", dyadic=True), gb=nc.affine(C, "plain", dyadic=True), w=nc.consumer(N, C, True))
    B, T, Tp, C, G = 2, (40 if route == "gn_stat16" else 64), 64, 128, 8
    y = nc.group_values(edge, B, T, Tp, C, G, "ref.gn", dyadic=True)
    y[:, T:] = 0
    return dict(y=y, T=T, Tp=Tp, G=G, gb=nc.affine(C, "signs", dyadic=True))


def _outputs(route, edge, fault):
    i = _inputs(route, edge)
    g, b = i["gb"]
    if route == "ln_rows":
        mu, rs, y = nc.ln_emulate(i["x"], g, b, eps=EPS, fault=fault)
        return dict(i, mean=mu, rstd=rs, out=y)
    if route == "prompt_pre":
        _, _, y = nc.ln_emulate(i["x"], g, b, eps=EPS, fault=fault, cpad=128, fma=True)
        return dict(i, out=nc.planes(y))
    if route == "linear_ln":
        w2, b2 = i["w"]
        return dict(i, out=nc.linear_ln_emulate(i["y1"], g, b, w2, b2, True, fault, EPS))
    cols = 1 if route == "gn_slab" else 16
    words = nc.block_words_emulate(i["y"], i["T"], cols, fault if fault in ("pad32", "slab_fp32") else None)
    m, r = nc.block_words_combine(words, i["T"], i["Tp"], i["G"], cols, EPS, fault)
    return dict(i, words=words, out=nc.planes(nc.gn_apply_emulate(i["y"], m, r, g, b)), cols=cols, fault=fault)


def _assertions(route, edge, o, figs):
    g, b = o["gb"]
    if route == "ln_rows":
        figs["_units_bound"] = nc.DEPTH["ln_rows"] / 2 + 1
        _, _, emu = nc.ln_emulate(o["x"], g, b, eps=EPS)
        nc.check_rows("y", o["out"], emu, nc.ln64(o["x"], g, b, EPS)[2], False, False, figs)
        nc.check_stats("stats", o["mean"], o["rstd"], o["x"].astype(F64)[:, None, :], EPS, nc.DEPTH["ln_rows"], figs)
    elif route == "prompt_pre":
        _, _, emu = nc.ln_emulate(o["x"], g, b, eps=EPS, fma=True)
        nc.check_rows("planes", o["out"], nc.planes(emu), nc.ln64(o["x"], g, b, EPS)[2], True, False, figs)
    elif route == "linear_ln":
        w2, b2 = o["w"]
        nc.check_rows("y2", o["out"], nc.linear_ln_emulate(o["y1"], g, b, w2, b2, True, None, EPS), nc.linear_ln64(o["y1"], g, b, w2, b2, EPS), False, False, figs)
    else:
        depth = nc.DEPTH["slab" if route == "gn_slab" else "stat16"]
        figs["_units_bound"] = depth / 2 + 1
        cols, T, Tp, G = o["cols"], o["T"], o["Tp"], o["G"]
        m, r = nc.block_words_combine(nc.block_words_emulate(o["y"], T, cols), T, Tp, G, cols, EPS)
        emu = nc.planes(nc.gn_apply_emulate(o["y"], m, r, g, b))
        valid = np.arange(Tp)[None, :].repeat(o["y"].shape[0], 0) < T
        try:
            nc.check_rows("y_norm", o["out"], emu, nc.gn64(o["y"], T, G, g, b, EPS)[2], True, False, figs, valid)
        finally:
            if o["fault"] != "slab_fp32":     # (those words are (sum, sum of squares): only their consumer reads them that way)
                mean, rstd = nc.words_to_group_stats(o["words"], T, Tp, G, cols, EPS)
                nc.check_group_stats("words", mean, rstd, o["y"], T, G, cols, EPS, depth, figs)


def table():
    """-> {(route, fault): (first point with ratio >= 5 or None, ratio there or the largest seen, correct ratio there)}, lines."""
    res, lines = {}, []
    for route, faults in ROUTE_FAULTS.items():
        correct = {p: judge(route, p, None, True) for p in POINTS}
        lines.append("%-10s correct arithmetic, reversed summation order: %s" % (route, "  ".join("%s %.2f" % (p, correct[p][0]) for p in POINTS)))
        for f in faults:
            rs = {p: judge(route, p, f, False) for p in POINTS}
            hit = next((p for p in POINTS if rs[p][0] >= 5.0), None)
            lines.append("%-10s %-10s %s" % (route, f, "  ".join("%s %.3g" % (p, rs[p][0]) for p in POINTS)))
            if hit is None:
                best = max(POINTS, key=lambda p: rs[p][0])
                res[(route, f)] = (None, rs[best][0], None)
                lines.append("%-10s %-10s OUT OF REACH: at most %.2f x its bound (at %s, %s)" % (route, f, rs[best][0], best, rs[best][1]))
            else:
                res[(route, f)] = (hit, rs[hit][0], correct[hit][0])
                lines.append("%-10s %-10s first seen at %s: %.3g x its bound (%s); correct arithmetic there %.2f x (%s a third)" % (
                    route, f, hit, rs[hit][0], rs[hit][1], correct[hit][0], "inside" if correct[hit][0] <= 1 / 3 else "NOT inside"))
    return res, lines


def main():
    print("# tools/norm_reference.py: emulated outputs through the assertions of tests/norm_cases.py; figures are (error / bound), 1 = the bound.\n"
          "# Points: the offset grid %s, then the unit draw, sigma = 1e-3, the 1e4 outlier." % (nc.OFFSET_GRID,))
    _, lines = table()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
