"""Reference-side figures of the trained-like regime of the two encoder engines (tests/offdist_enc_cases.py): for every
(severity, logit gain) of its GRID and every case of tests/test_gpu_offdist_enc.py, the oracle in fp32 against itself in fp64 on
every probe and output (a third of the whole-tensor and per-frame bounds, the 1 % floor cap), whether the reference's -1e4 key mask
still is a mask (the largest |logit| of any valid query and key below MASK_LOGIT_MAX), and the regime the fp64 intermediates reach.  The rule of
tools/offdist_reference.py: per engine, the largest grid point that keeps the reference inside is the profile.  CPU.
  python tools/offdist_enc_reference.py > profiles/offdist_enc_reference.txt"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import diff_vits_amd  # noqa: E402,F401
import offdist_enc_cases as ec  # noqa: E402
import prompt_cases as pc  # noqa: E402
import tenc_cases as tc  # noqa: E402
from parity_metrics import FRAME_BOUND  # noqa: E402

# oracle.text_enc_ref masks padded keys with masked_fill(-1e4) and the kernel leaves them out: the same result only while
# -1e4 - (row maximum) underflows exp() in fp32, i.e. while the valid logits stay well inside +-1e4.
MASK_LOGIT_MAX = 9000.0


def _cases(engine, profile):
    """Yields (case id, lengths, fp32 tensors, fp64 tensors, stats of the fp64 restatement, largest |logit|)."""
    if engine == "tenc":
        sd = ec.tenc_state_dict(**profile)
        sd64 = {k: v.double() for k, v in sd.items()}
        for name in ec.TENC_CASES:
            _, B, T, lengths = tc.case(name)
            ids, tone, lang, ln, g = ec.tenc_inputs(B, T, lengths, **profile)
            for tag, gg in (("g", g), ("no-g", None)):
                p32, p64 = ec.tenc_pair(sd, ids, ln, tone, lang, gg)
                st = {}
                ec.tenc_layers(sd64, p64, ln, gg, stats=st)
                yield "%s %s" % (name, tag), lengths, p32, p64, st
    else:
        for name in ec.PENC_CASES:
            _, fl, B, L, lengths = pc.case(name)
            sd = ec.penc_state_dict(fl, **profile)
            n_layers = pc.FLAVOURS[fl][0]["n_layers"]
            prompt, ln = ec.penc_inputs(fl, B, L, lengths, **profile)
            p32, p64 = ec.penc_pair(sd, prompt, ln, n_layers)
            st = {}
            ec.penc_layers({k: v.double() for k, v in sd.items()}, p64, ln, n_layers, stats=st)
            yield name, lengths, p32, p64, st


def _point(engine, profile):
    """One grid point: the worst reference margins over the cases, the largest |logit| of a valid query, the regime per model and
    the detail lines."""
    worst = {"rel_l2": 0.0, "frame": 0.0, "ratio": 0.0, "floored": 0.0, "ratio_at": ""}
    stats, lines, logit = {}, [], 0.0
    for cid, lengths, p32, p64, st in _cases(engine, profile):
        ls, w = ec.reference_margins(p32, p64, lengths)
        for k in ("rel_l2", "frame", "floored"):
            worst[k] = max(worst[k], w[k])
        if w["ratio"] > worst["ratio"]:
            worst["ratio"], worst["ratio_at"] = w["ratio"], "%s of %s" % (w["ratio_at"], cid)
        stats[cid] = st
        logit = max(logit, max(v[3] for v in st["attn"].values()))
        lines += ["# %s %s: fp32 oracle vs fp64 oracle" % (engine, cid)] + ls
        lines += ["%-22s LayerNorm input: median |mean|/sigma %.2f" % kv for kv in st["ln"].items()]
        lines += ["%-22s attention: median top-1 probability %.3f, median max |logit| %.1f, %d keys, largest |logit| %.1f" % ((k,) + v)
                  for k, v in st["attn"].items()]
    return worst, logit, ec.regime_by_model(engine, stats), lines


def _regime_text(regs):
    out = []
    for model, reg in regs.items():
        out.append("%s (r1) %s: worst layer %.2f%s [%s] (r2) %s: top-1 %.3f%s" % (
            model, "reached" if reg["ln_ok"] else "MISSED", reg["ln_min"],
            "" if reg["ln_ok"] else ", short of %.0f by %.2f" % (ec.REGIME_MIN, ec.REGIME_MIN - reg["ln_min"]),
            " ".join("%.2f" % f for f in reg["ln_per_layer"]), "reached" if reg["top1_ok"] else "MISSED", reg["top1"],
            "" if reg["top1_ok"] else ", short of %.1f by %.3f" % (ec.TOP1_MIN, ec.TOP1_MIN - reg["top1"])))
    return "; ".join(out)


def main():
    print("# Trained-like regime of the encoder engines (tests/offdist_enc_cases.py), reference side only (tools/offdist_enc_reference.py, CPU).\n"
          "# (a) fp32 oracle vs fp64 oracle, every probe and output, valid frames: whole tensor < %.2e, every frame < %.2e (a third of 2e-4 and\n"
          "#     FRAME_BOUND); the localisation bound of the GPU test is 3 x the largest ratio measured here, so no third applies to it;\n"
          "# (b) at most 1 %% of the valid reference frames of any probe on the norm floor;\n"
          "# (c) text encoder: the largest |logit| of any valid (query, key) pair of any attention < %.0f (the reference's -1e4 key mask is still a\n"
          "#     mask for every query);\n"
          "# regime, reported per MODEL (the text encoder; the prompt encoder's flavours D and P apart, each over all of its layers) and not a\n"
          "#     condition of the choice: (r1) median row |mean| / sigma >= %.0f at a LayerNorm input of every layer (per layer the best of its\n"
          "#     LayerNorm inputs over the model's cases), (r2) median top-1 probability >= %.1f at one attention on a case with more than 32 keys." % (
              2e-4 / 3, FRAME_BOUND / 3, MASK_LOGIT_MAX, ec.REGIME_MIN, ec.TOP1_MIN))
    for engine in ("tenc", "penc"):
        best, detail = None, {}
        for s, lg in ec.GRID:
            worst, logit, regs, lines = _point(engine, dict(severity=s, logit_gain=lg))
            ok = ec.margins_ok(worst) and (engine != "tenc" or logit < MASK_LOGIT_MAX)
            print("# %s severity %.2f logit gain %g: (a) tensor %.2e frame %.2e, localisation %.2f (%s) (b) floored %.3f (c) largest |logit| %.0f -> %s; "
                  "regime: %s" % (engine, s, lg, worst["rel_l2"], worst["frame"], worst["ratio"], worst["ratio_at"], worst["floored"], logit,
                                  "ok" if ok else "no", _regime_text(regs)))
            if ok:
                best = (s, lg)
                detail = {"lines": lines, "worst": worst, "regs": regs}
        worst = detail["worst"]
        print("# %s: the largest point of the grid with (a), (b), (c): severity %.2f, logit gain %g (PROFILES[\"%s\"]).  Reference-side localisation\n"
              "#   maximum %.2f at %s (LOCALISATION_REF_MAX[\"%s\"]).\n#   Regime at this point: %s." % (
                  engine, best[0], best[1], engine, worst["ratio"], worst["ratio_at"], engine, _regime_text(detail["regs"])))
        print("\n".join(detail["lines"]))
        assert dict(severity=best[0], logit_gain=best[1]) == ec.PROFILES[engine], (engine, best, ec.PROFILES[engine])
        assert "%.2f" % worst["ratio"] == "%.2f" % ec.LOCALISATION_REF_MAX[engine], (engine, worst["ratio"], ec.LOCALISATION_REF_MAX[engine])
    # the second text-encoder point, chosen by hand and not by the rule (offdist_enc_cases.PROFILES)
    prof = ec.PROFILES["tenc-mild"]
    worst, logit, regs, lines = _point("tenc", prof)
    print("# tenc-mild: severity %.2f, logit gain %g, not chosen by the rule: a point whose softmax is peaked, not saturated.  (a) tensor %.2e frame\n"
          "#   %.2e (b) floored %.3f (c) largest |logit| %.0f; reference-side localisation maximum %.2f at %s (LOCALISATION_REF_MAX[\"tenc-mild\"]).\n"
          "#   Regime: %s." % (prof["severity"], prof["logit_gain"], worst["rel_l2"], worst["frame"], worst["floored"], logit, worst["ratio"],
                              worst["ratio_at"], _regime_text(regs)))
    print("\n".join(lines))
    assert ec.margins_ok(worst) and logit < MASK_LOGIT_MAX
    assert "%.2f" % worst["ratio"] == "%.2f" % ec.LOCALISATION_REF_MAX["tenc-mild"], worst["ratio"]


if __name__ == "__main__":
    torch.set_num_threads(min(16, torch.get_num_threads()))
    main()
