"""Reference-side figures of the vocoder parity tests (CPU only): writes profiles/vocoder_reference.txt.

For every case of tests/vocoder_cases.py with the trained-like weights: what the inputs exercise (log-magnitude span, share of
bins at the 1e2 clip, phase sigma), the fp32 torch restatement and the two-plane emulation against fp64 (whole tensor, worst
256-sample block, worst frame of every probe, localisation ratio), and the condition asked of every such profile: the fp32
reference alone stays inside a third of every bound the GPU test uses.

    python tools/vocoder_reference.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import parity_metrics as pm  # noqa: E402
import vocoder_cases as vc  # noqa: E402


def main():
    lines = ["vocoder: reference-side figures (tools/vocoder_reference.py; fp64 restatement = tests/vocoder_cases.reference)", ""]
    ok_all = True
    loc_max = 0.0
    for cfg_name, cfg, cases in (("C512/I1536/L8", vc.CFG_FULL, vc.CASES), ("C128/I384/L2", vc.CFG_SMALL, vc.CASES[2:3])):
        sd = vc.make_weights(cfg)
        for B, T, lengths in cases:
            mel = vc.make_mel(B, T, lengths)
            want = vc.reference(sd, cfg, mel, lengths)
            f32 = vc.reference(sd, cfg, mel, lengths, dtype=torch.float32)
            emu = vc.reference(sd, cfg, mel, lengths, emulate=True)
            rows = [b for b, L in enumerate(lengths) if 2 <= L <= T]
            head = torch.cat([want["head"][b, :lengths[b]] for b in rows])
            m, p = head[:, :vc.BINS], head[:, vc.BINS:]
            lines.append("%s  B=%d T=%d lengths=%s" % (cfg_name, B, T, lengths))
            lines.append("  log-magnitude %.1f .. %.1f, %.3f %% of the bins at the 1e2 clip, phase sigma %.2f rad, |p| max %.1f"
                         % (float(m.min()), float(m.max()), 100.0 * float((m > 4.60517).double().mean()), float(p.std()), float(p.abs().max())))
            for tag, other in (("fp32 torch", f32), ("two-plane emulation", emu)):
                worst_probe, worst_whole, worst_loc = 0.0, 0.0, 0.0
                for name in vc.probe_names(cfg["n_layers"]):
                    _, fig = vc.probe_failures(name, other[name], want[name], lengths, T)
                    worst_probe, worst_whole = max(worst_probe, fig["worst"]), max(worst_whole, fig["rel_l2"])
                    if fig["rel_l2"] > 1e-7:
                        worst_loc = max(worst_loc, fig["loc"])
                g, nb = vc.wave_blocks(other["wave"], lengths, T)
                w, _ = vc.wave_blocks(want["wave"], lengths, T)
                fe = pm.masked_frame_errors(g, w, nb)
                _, hf = vc.probe_failures("head", other["head"], want["head"], lengths, T)
                lines.append("  %-20s wave: tensor %.2e, worst block %.2e; head worst frame %.2e; probes: tensor <= %.2e, frame <= %.2e, localisation <= %.2f"
                             % (tag, fe["rel_l2"], fe["worst"], hf["worst"], worst_whole, worst_probe, worst_loc))
                if tag == "fp32 torch":
                    loc_max = max(loc_max, worst_loc)
                    _, wf = vc.wave_failures(other["wave"], emu["wave"], want["wave"], lengths, T)
                    third = (worst_whole <= vc.WHOLE_BOUND / 3 and worst_probe <= pm.FRAME_BOUND / 3 and fe["worst"] <= wf["bound"] / 3
                             and fe["rel_l2"] <= wf["bound"] / 3)
                    ok_all = ok_all and third
                    lines.append("  %-20s inside a third of every bound (2e-4 / 3, 1e-3 / 3, wave bound %.2e / 3): %s" % ("", wf["bound"], "yes" if third else "NO"))
            lines.append("")
    lines.append("largest localisation ratio of the fp32 restatement, every probe of every case: %.2f (vocoder_cases.LOCALISATION_REF_MAX = %.2f)"
                 % (loc_max, vc.LOCALISATION_REF_MAX))
    lines.append("fp32 reference inside a third of every bound at every case: %s" % ("yes" if ok_all else "NO"))
    text = "\n".join(lines) + "\n"
    with open(os.path.join(ROOT, "profiles", "vocoder_reference.txt"), "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
