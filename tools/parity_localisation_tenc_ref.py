"""Localisation ratio of the REFERENCE side for the text encoder: oracle.text_enc_ref in fp32 against itself in fp64 (state
dict and g .double()) on every case of tests/tenc_cases.py, with and without g, every probe + the three outputs, valid frames
only.  CPU.
  python tools/parity_localisation_tenc_ref.py > profiles/parity_localisation_tenc_ref.txt"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import diff_vits_amd  # noqa: E402,F401
import tenc_cases as tc  # noqa: E402
from prompt_cases import report_line  # noqa: E402
from parity_metrics import masked_frame_errors  # noqa: E402


def main():
    lines, top, per_case = [], (0.0, ""), []
    sd = tc.state_dict()
    for name, B, T, lengths in tc.CASES:
        ids, tone, lang, ln, g = tc.inputs(B, T, lengths)
        for with_g in (True, False):
            gg = g if with_g else None
            with torch.no_grad():
                o32, p32 = tc.oracle_probes(sd, ids, ln, tone, lang, gg, torch.float32)
                o64, p64 = tc.oracle_probes(sd, ids, ln, tone, lang, gg, torch.float64)
            lines.append("# %s B=%d T=%d lengths=%s %s" % (name, B, T, ",".join(str(v) for v in lengths), "with g" if with_g else "without g"))
            worst = 0.0
            for k in list(p32) + ["x", "m", "logs"]:
                a, b = (p32[k], p64[k]) if k in p32 else (o32["x m logs".split().index(k)], o64["x m logs".split().index(k)])
                fe = masked_frame_errors(a, b, lengths)
                lines.append(report_line(k, fe))
                ratio = fe["worst"] / max(fe["rel_l2"], 1e-300)
                worst = max(worst, ratio)
                if ratio > top[0]:
                    top = (ratio, "%s of %s %s" % (k, name, "with g" if with_g else "without g"))
            per_case.append("#   %-6s %-9s largest ratio %.2f" % (name, "with g" if with_g else "without g", worst))
    print("# Localisation ratio (worst-frame relative error / whole-tensor relative L2 over the VALID frames, tests/parity_metrics.py)\n"
          "# of the REFERENCE side of the text-encoder tests: oracle.text_enc_ref in fp32 against itself in fp64, every probe + the\n"
          "# outputs x / m / logs, every case of tests/tenc_cases.py with and without the speaker vector\n"
          "# (tools/parity_localisation_tenc_ref.py).\n%s\n"
          "# Largest ratio: %.2f (%s).\n"
          "# The GPU tests bound the HIP path's ratio at 3 x that = %.2f (tests/tenc_cases.py TENC_LOCALISATION_BOUND = 3 x %.2f)."
          % ("\n".join(per_case), top[0], top[1], 3 * top[0], tc.TENC_LOCALISATION_REF_MAX))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
