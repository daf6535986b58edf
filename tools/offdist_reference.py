"""Reference-side figures of the trained-like regime (tests/offdist_cases.py): for every severity of SEVERITY_GRID and both shapes of
tests/test_gpu_offdist.py, the oracle in fp32 against itself in fp64 on every probe (conditions (a) and (b): a third of the
layer-wise bounds, the floor guard) and the regime its fp64 intermediates reach (condition (c): median |mean| / sigma of the rows
at a LayerNorm of every width and of the groups at a GroupNorm of every level).  CPU.
  python tools/offdist_reference.py > profiles/offdist_reference.txt"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import diff_vits_amd  # noqa: E402,F401
import offdist_cases as oc  # noqa: E402
from conftest import UNET_CASES  # noqa: E402
from parity_metrics import FRAME_BOUND, LOCALISATION_BOUND  # noqa: E402


def main():
    kw = UNET_CASES["cfg1"][0]
    rows, ok, detail = [], {}, []
    for s in (0.0,) + oc.SEVERITY_GRID:
        for case, (B, T, L, _) in oc.CASES.items():
            sd, sample, t, enc, mask = oc.case_tensors(kw, B, T, L, severity=s)
            pick = sorted({0, B - 1})
            (y32, p32), (y64, p64) = oc.oracle_pair(kw, sd, sample[pick], t[pick], enc[pick], mask[pick])
            lines, worst = oc.reference_margins(p32, y32, p64, y64)
            fig = oc.regime_figures(p64)
            a, c = oc.margins_ok(worst), oc.regime_reached(fig)
            ok[s] = ok.get(s, True) and a and c
            rows.append("# severity %.2f %-15s (a) tensor %.2e frame %.2e ratio %.2f (b) %s -> %s; (c) LayerNorm %s GroupNorm %s -> %s" % (
                s, case, worst["rel_l2"], worst["frame"], worst["ratio"], "ok" if worst["floored_ok"] else "FLOORED", "ok" if a else "no",
                " ".join("C=%d %.2f" % kv for kv in sorted(fig["ln_by_width"].items())),
                " ".join("L%d %.2f" % kv for kv in sorted(fig["gn_by_level"].items())), "ok" if c else "no"))
            if s == oc.PROFILES["trained"]["severity"]:
                emb = p64["emb"][:, 0]
                sc = [float(torch.nn.functional.linear(torch.nn.functional.silu(emb), sd[k].double(), sd[k[:-6] + "bias"].double())
                            .chunk(2, -1)[0].abs().median()) for k in sd if k.endswith("time_emb_proj.weight")]
                detail.append("# %s at severity %.2f: median |time_emb_proj scale| over the 22 resnet blocks %.2f .. %.2f; largest row |mean| / sigma "
                              "at a LayerNorm input %.2f (%s), largest group figure %.2f (%s)" % (
                                  case, s, min(sc), max(sc), max(f for _, f in fig["ln"].values()), max(fig["ln"], key=lambda n: fig["ln"][n][1]),
                                  max(f for _, f in fig["gn"].values()), max(fig["gn"], key=lambda n: fig["gn"][n][1])))
                detail += ["# %s B=%d T=%d L=%d severity %.2f: fp32 oracle vs fp64 oracle" % (case, B, T, L, s)] + lines
                detail += ["%-58s %s |mean|/sigma %.2f" % (n, "LayerNorm input C=%d" % c_, f) for n, (c_, f) in fig["ln"].items()]
                detail += ["%-58s %s |mean|/sigma %.2f" % (n, "GroupNorm input level %d" % l_, f) for n, (l_, f) in fig["gn"].items()]
    best = max([s for s in oc.SEVERITY_GRID if ok[s]], default=None)
    print("# Trained-like regime (tests/offdist_cases.py), reference side only (tools/offdist_reference.py, CPU).\n"
          "# (a) fp32 oracle vs fp64 oracle on every probe and y, utterances 0 and B - 1: whole tensor < %.2e, every frame < %.2e, localisation\n"
          "#     ratio < %.2f (a third of 2e-4, FRAME_BOUND, LOCALISATION_BOUND); (b) at most 1 %% of the frames on the norm floor;\n"
          "# (c) median row |mean| / sigma >= %.0f at a LayerNorm input of every width, median |group mean| / sigma >= %.0f at a GroupNorm input\n"
          "#     of every level (the best LayerNorm per width / GroupNorm per level is listed)." % (2e-4 / 3, FRAME_BOUND / 3, LOCALISATION_BOUND / 3,
                                                                                                   oc.REGIME_MIN, oc.REGIME_MIN))
    print("\n".join(rows))
    print("# Largest severity of the grid with (a), (b), (c) on both shapes: %s (PROFILES[\"trained\"] uses %.2f). One profile serves the offset and\n"
          "# the gain / outlier family: no per-family profiles." % (best, oc.PROFILES["trained"]["severity"]))
    print("\n".join(detail))
    assert best == oc.PROFILES["trained"]["severity"], (best, oc.PROFILES)


if __name__ == "__main__":
    main()
