"""Localisation ratio of the REFERENCE side for the prompt encoder: oracle fp32 against oracle fp64 (state dict and prompt
.double()) on every case of tests/prompt_cases.py, every probe + the output, valid frames only.  CPU.
  python tools/parity_localisation_penc_ref.py > profiles/parity_localisation_penc_ref.txt"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import diff_vits_amd  # noqa: E402,F401
import prompt_cases as pc  # noqa: E402
from parity_metrics import LOCALISATION_REF_MAX, PENC_LOCALISATION_BOUND, masked_frame_errors, prompt_oracle_probes  # noqa: E402


def main():
    lines, top = [], (0.0, "")
    for name, flavour, B, L, lengths in pc.CASES:
        sd = pc.state_dict(flavour)
        prompt, ln = pc.inputs(flavour, B, L, lengths)
        n_layers = pc.FLAVOURS[flavour][0]["n_layers"]
        with torch.no_grad():
            y32, p32 = prompt_oracle_probes(sd, prompt, ln, n_layers)
            y64, p64 = prompt_oracle_probes({k: v.double() for k, v in sd.items()}, prompt.double(), ln, n_layers)
        lines.append("# %s B=%d L=%d lengths=%s" % (name, B, L, ",".join(str(v) for v in lengths)))
        for k in list(p32) + ["y"]:
            fe = masked_frame_errors(y32 if k == "y" else p32[k], y64 if k == "y" else p64[k], lengths)
            lines.append(pc.report_line(k, fe))
            ratio = fe["worst"] / max(fe["rel_l2"], 1e-300)
            if ratio > top[0]:
                top = (ratio, "%s of %s" % (k, name))
    print("# Localisation ratio (worst-frame relative error / whole-tensor relative L2 over the VALID frames, tests/parity_metrics.py)\n"
          "# of the REFERENCE side of the prompt-encoder tests: oracle.prompt_ref in fp32 against itself in fp64, every probe + the\n"
          "# output y, every case of tests/prompt_cases.py (tools/parity_localisation_penc_ref.py).\n"
          "# Largest ratio: %.2f (%s); the denoiser's reference maximum LOCALISATION_REF_MAX is %.2f.\n"
          "# The GPU tests bound the HIP path's ratio at 3 x the largest = %.2f (tests/parity_metrics.py PENC_LOCALISATION_BOUND)."
          % (top[0], top[1], LOCALISATION_REF_MAX, PENC_LOCALISATION_BOUND))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
