"""The text-encoder cases of the layer-wise parity tests (tests/test_gpu_tenc_layerwise.py, the planted faults of
tests/test_tenc_cpu.py, tools/parity_localisation_tenc_ref.py): the product's configuration (H = 256, 2 heads of 128 channels, 6
layers, k = 3, window 4, speaker vector in front of layer 2), seeded weights and ids, the oracle's named intermediates and the
check of one tensor under the criteria of tests/parity_metrics.py.  Plain helper module: no fixtures, no hooks."""
import math

import torch

from parity_metrics import FRAME_BOUND, describe, masked_frame_errors
from prompt_cases import report_line

KW = dict(n_vocab=108, out_channels=128, hidden_channels=256, filter_channels=256, n_heads=2, n_layers=6, kernel_size=3,
          p_dropout=0.1, gin_channels=256, n_tones=11, n_languages=3)
WINDOW, COND_LAYER = 4, 2

# (id, B, T, lengths)
CASES = [
    ("1x1", 1, 1, [1]),
    ("2x5", 2, 5, [5, 3]),
    ("3x75", 3, 75, [75, 40, 9]),
    ("3x33", 3, 33, [33, 32, 31]),
    ("16x36", 16, 36, [36, 34, 32, 30, 28, 26, 24, 22, 20, 18, 16, 14, 12, 10, 8, 7]),     # configuration 5's token count
    ("2x300", 2, 300, [300, 257]),
]
IDS = [c[0] for c in CASES]

# Largest localisation ratio (worst valid frame / whole tensor) the reference side shows against itself on these cases - the
# oracle in fp32 against the oracle in fp64, every probe and output, with and without g: profiles/parity_localisation_tenc_ref.txt
# (tools/parity_localisation_tenc_ref.py).  The largest is 1.79 (layer0.ln1 of 3x33).  The bound for the HIP path is 3 x that, the rule of
# PENC_LOCALISATION_BOUND.  No case is excluded from the ratio criterion: 1x1 has one frame, its ratio is 1 on either side.
TENC_LOCALISATION_REF_MAX = 1.79
TENC_LOCALISATION_BOUND = 3 * TENC_LOCALISATION_REF_MAX


def case(name):
    return CASES[IDS.index(name)]


def state_dict(seed=1234):
    """{TextEncoder parameter name (relative to enc_p.): float32 tensor}, seeded under the full reference names."""
    from diff_vits_amd import synth
    from diff_vits_amd.model3 import TextEncoder
    with torch.device("meta"):
        shapes = {"enc_p." + k: tuple(v.shape) for k, v in TextEncoder(**KW).state_dict().items()}
    return {k[len("enc_p."):]: torch.from_numpy(v) for k, v in synth.make_state_dict(shapes, seed=seed).items()}


def inputs(B, T, lengths, tag="te"):
    """(ids, tone, language int64 [B, T], lengths int64 [B], g float32 [B, gin, 1]), seeded."""
    from diff_vits_amd import synth
    def idx(name, n):
        u = synth.uniform(1234, "%s.%s" % (tag, name), (B, T), 1.0)
        return torch.from_numpy(((u * 0.5 + 0.5) * n).astype("int64").clip(0, n - 1))
    g = torch.from_numpy(synth.normal(1234, tag + ".g", (B, KW["gin_channels"], 1)))
    return (idx("ids", KW["n_vocab"]), idx("tone", KW["n_tones"]), idx("lang", KW["n_languages"]),
            torch.tensor(lengths, dtype=torch.int64), g)


def probe_names(n_layers=KW["n_layers"]):
    """Names of the text encoder's intermediates (dv_tenc_probe, include/dvits_hip.h), in schedule order."""
    names = ["emb"]
    for i in range(n_layers):
        names += ["layer%d.attn" % i, "layer%d.ln1" % i, "layer%d.ffn1" % i, "layer%d" % i]
    return names + ["proj"]


def oracle_probes(sd, ids, lengths, tone, language, g, dtype=torch.float32):
    """oracle.text_enc_ref.text_encoder with its named intermediates, keyed like the engine's probes, channels-last [B, T, C]
    and MASKED (the engine keeps padding rows at zero; the reference lets them drift, no valid frame reads them):
    ((x, m, logs) channels-last, dict).  Taken by wrapping rel_attention / _ln_c / ffn, which the oracle calls through its module
    globals; the wrappers return what the originals return."""
    import torch.nn.functional as F
    from oracle import prompt_ref, text_enc_ref as R
    sd = {k: v.to(dtype) for k, v in sd.items()}
    g = None if g is None else g.to(dtype)
    T = ids.shape[1]
    mask = prompt_ref.sequence_mask(lengths, T).to(dtype)[:, :, None]             # [B, T, 1]
    out, state = {}, {"ln": 0}
    orig = {n: getattr(R, n) for n in ("rel_attention", "_ln_c", "ffn")}

    def cl(v):
        return v.transpose(1, 2).contiguous() * mask

    def rel_attention(sdd, p, x, attn_mask, n_heads, window):
        y = orig["rel_attention"](sdd, p, x, attn_mask, n_heads, window)
        out["layer%d.attn" % int(p.split("attn_layers.")[1].split(".")[0])] = cl(x + y)
        return y

    def _ln_c(x, gamma, beta, eps=1e-5):
        y = orig["_ln_c"](x, gamma, beta, eps)
        i, second = divmod(state["ln"], 2)
        out["layer%d" % i if second else "layer%d.ln1" % i] = cl(y)
        state["ln"] += 1
        return y

    def ffn(sdd, p, x, x_mask, kernel_size):
        pad = ((kernel_size - 1) // 2, kernel_size // 2)
        h = torch.relu(F.conv1d(F.pad(x * x_mask, pad), sdd[p + "conv_1.weight"], sdd[p + "conv_1.bias"]))
        out["layer%d.ffn1" % int(p.split("ffn_layers.")[1].split(".")[0])] = cl(h)
        return orig["ffn"](sdd, p, x, x_mask, kernel_size)

    R.rel_attention, R._ln_c, R.ffn = rel_attention, _ln_c, ffn
    try:
        x, m, logs, x_mask = R.text_encoder(sd, ids, lengths, tone, language, g, KW["n_heads"], KW["n_layers"], KW["kernel_size"], prefix="")
    finally:
        for n, f in orig.items():
            setattr(R, n, f)
    H = sd["emb.weight"].shape[1]
    out["emb"] = (F.embedding(ids, sd["emb.weight"]) + F.embedding(tone, sd["tone_emb.weight"])
                  + F.embedding(language, sd["language_emb.weight"])) * math.sqrt(H) * mask
    out["proj"] = torch.cat([m, logs], 1).transpose(1, 2).contiguous()
    names = probe_names()
    assert set(names) == set(out), set(names) ^ set(out)
    return tuple(v.transpose(1, 2).contiguous() for v in (x, m, logs)), {n: out[n] for n in names}


def check(name, got, want, lengths, report, failures, loc_bound=TENC_LOCALISATION_BOUND):
    """One [B, T, C] tensor against the oracle's on its valid frames: whole tensor < 2e-4, every frame < FRAME_BOUND, localisation
    < TENC_LOCALISATION_BOUND, at most 1 % of the valid frames on the norm floor, every
    padding frame exactly zero (loc_bound: the localisation bound measured for other weights, tests/offdist_enc_cases.py).  Appends the figures to `report` and, on a failure, describe()'s line with the reasons to
    `failures`."""
    fe = masked_frame_errors(got, want, lengths)
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
    if not fe["padding_zero"]:
        why.append("padding frame %d of utterance %d is not zero" % (fe["first_nonzero"][1], fe["first_nonzero"][0]))
    if why:
        failures.append("%s  [%s]" % (describe(name, got, want, lengths), "; ".join(why)))
    return fe
