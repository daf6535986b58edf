"""The prompt-encoder cases of the layer-wise parity tests (tests/test_gpu_prompt_layerwise.py, the planted faults of
tests/test_parity_metrics.py, tools/parity_localisation_penc_ref.py): the two flavours the product runs, seeded weights and
prompts, and the check of one tensor under the criteria of tests/parity_metrics.py.  Plain helper module: no fixtures, no hooks.

Flavour D is the denoiser's conditioning encoder (Diffusion_Encoder.prompt_encoder: 100 -> 128 -> 128 channels, 4 layers, head
dim 16); its weights are the `prompt_encoder.` entries of the Diffusion_Encoder state dict the goldens were made with, so the
B = 2 / L = 40 case is the golden one.  Flavour P is the prior's o_proj (128 -> 256 -> 128, 6 layers, head dim 32, no `g`),
which runs over frames."""
import torch

from parity_metrics import FRAME_BOUND, PENC_LOCALISATION_BOUND, describe, masked_frame_errors

FLAVOURS = {
    "D": (dict(in_channels=100, hidden_channels=128, out_channels=128, n_layers=4), "prompt_encoder."),
    "P": (dict(in_channels=128, hidden_channels=256, out_channels=128, n_layers=6), "o_proj."),
}

_RAGGED_16x256 = [256] * 16
_RAGGED_16x256[5], _RAGGED_16x256[11] = 200, 97

# (id, flavour, B, L, lengths)
CASES = [
    # the benchmark's conditioning shape; a length on every side of a 32- and a 64-row boundary, one utterance shorter than the
    # nine-tap window, one single frame
    ("D-8x256", "D", 8, 256, [256, 255, 224, 129, 33, 32, 9, 1]),
    ("D-16x256", "D", 16, 256, _RAGGED_16x256),                                 # M = 4096: the large-tile menu
    ("D-16x36", "D", 16, 36, [36] * 16),                                        # configuration 5's prompts
    ("D-3x75", "D", 3, 75, [75, 1, 50]),
    ("D-2x40", "D", 2, 40, [40, 27]),                                           # the goldens' (tests/golden/prompt_cfg.npz)
    ("D-1x1", "D", 1, 1, [1]),
    ("D-1x5", "D", 1, 5, [5]),
    ("D-2x300", "D", 2, 300, [300, 77]),                                        # more than 256 keys, L % 32 != 0
    ("P-8x1024", "P", 8, 1024, [1024, 1023, 993, 512, 300, 99, 64, 7]),         # o_proj at the benchmark length
    ("P-16x99", "P", 16, 99, [99, 98, 97, 96, 65, 64, 63, 50, 33, 32, 31, 17, 10, 9, 2, 1]),
    ("P-2x36", "P", 2, 36, [36, 20]),
    ("P-1x2048", "P", 1, 2048, [2048]),
]
IDS = [c[0] for c in CASES]


def case(name):
    return CASES[IDS.index(name)]


def state_dict(flavour):
    """{PromptEncoder parameter name: float32 tensor}, seeded (synth.make_state_dict keys every tensor by its full name)."""
    from diff_vits_amd import synth
    from diff_vits_amd.model3 import PromptEncoder
    kw, prefix = FLAVOURS[flavour]
    with torch.device("meta"):
        shapes = {prefix + k: tuple(v.shape) for k, v in PromptEncoder(p_dropout=0.2, backend="torch", **kw).state_dict().items()}
    return {k[len(prefix):]: torch.from_numpy(v) for k, v in synth.make_state_dict(shapes, seed=1234).items()}


def inputs(flavour, B, L, lengths, tag="pe.prompt"):
    from diff_vits_amd import synth
    prompt = torch.from_numpy(synth.normal(1234, tag, (B, FLAVOURS[flavour][0]["in_channels"], L)))
    return prompt, torch.tensor(lengths, dtype=torch.int64)


def report_line(name, fe):
    return ("%-14s rel_l2 %.3e worst_frame %.3e at (%d, %d) ratio %5.2f floored %d/%d padding_zero %s" %
            (name, fe["rel_l2"], fe["worst"], fe["at"][0], fe["at"][1], fe["worst"] / max(fe["rel_l2"], 1e-300), fe["floored"],
             fe["frames"], fe["padding_zero"]))


def check(name, got, want, lengths, report, failures, masked=True, loc_bound=PENC_LOCALISATION_BOUND):
    """One [B, L, C] tensor against the oracle's on its valid frames: whole tensor < 2e-4, every frame < FRAME_BOUND, localisation
    < PENC_LOCALISATION_BOUND, at most 1 % of the valid frames on the norm floor, every padding frame exactly zero (masked=False: a
    tensor the schedule does not mask - layerN.ffn1; loc_bound: the localisation bound measured for other weights,
    tests/offdist_enc_cases.py).  Appends the figures to `report` and, if a criterion fails, describe()'s
    line (probe, utterance, frame, block) with the reasons to `failures`."""
    fe = masked_frame_errors(got, want, lengths)
    if not masked:
        fe["padding_zero"] = "n/a"
    ratio = fe["worst"] / max(fe["rel_l2"], 1e-300)
    report.append(report_line(name, fe))
    why = []
    if not fe["floored_ok"]:
        why.append("%d of %d valid reference frames sit on the norm floor" % (fe["floored"], fe["frames"]))
    if not fe["rel_l2"] < 2e-4:
        why.append("whole tensor %.2e >= 2e-4" % fe["rel_l2"])
    if not fe["worst"] < FRAME_BOUND:
        why.append("a frame at %.2e >= %.0e" % (fe["worst"], FRAME_BOUND))
    if not ratio < loc_bound:
        why.append("localisation %.2f >= %.2f" % (ratio, loc_bound))
    if masked and not fe["padding_zero"]:
        why.append("padding frame %d of utterance %d is not zero" % (fe["first_nonzero"][1], fe["first_nonzero"][0]))
    if why:
        failures.append("%s  [%s]" % (describe(name, got, want, lengths), "; ".join(why)))
    return fe
