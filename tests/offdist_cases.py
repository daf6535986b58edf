"""Trained-like weight and input statistics for the denoiser's parity tests (plain helper module: no fixtures, no hooks).

synth.make_state_dict is PyTorch-default initialisation: norm gains 1 +- 0.1, norm biases +- 0.1, conv / linear biases
+- 1 / sqrt(fan_in), zero-mean unit-variance inputs.  In that regime a LayerNorm row has mean / sigma of about 0 and a GroupNorm
group likewise, so the cancellation in  rstd (x W' - mean u) + b'  (LayerNorm folded into the consumer GEMM, the raw rows stored as
two bf16 planes) and in the GroupNorm's folded per-column affine costs nothing.  make_state_dict_trained layers on top of it,
scaled by ONE `severity` knob, what a trained checkpoint has:

  norm gains    x 2^(s G z) (log-normal, z ~ N(0, 1)), a share of the channels multiplied up by 1 + s OUT, a few negative;
  norm biases   + s (NB z + NC c), c one number per layer (the common offset: |c| in [0.5, 1), either sign);
  other biases  + s (LB z + LC c) likewise - the common offset of a layer's bias is what gives the next LayerNorm a row mean and
                the next GroupNorm a group mean.  Two exceptions keep the nonlinearities in their working range: the GATE half of
                ff.net.0.proj.bias gets the spread but no common offset (GELU is neither 0 nor the identity), and
                time_emb_proj.bias has smaller constants of its own (the resnet blocks' `scale` is O(1), not O(10));
  inputs        x, cond, enc: per-channel scale 2^(s IS z) and offset s IO z, a few channels multiplied up by 1 + s OUT.

Everything is synth's integer hashing followed by exact float arithmetic (2^x is the piecewise-linear (1 + frac) 2^floor on a
1 / 16 grid: no libm), so (seed, severity) gives the same bits everywhere, and severity = 0 gives make_state_dict bit for bit
(every factor is exactly 1.0, every addend exactly 0.0; tests/test_offdist_reference.py asserts it).

One profile, PROFILES["trained"]: the largest severity of SEVERITY_GRID at which the reference alone stays in bounds on both shapes of
tests/test_gpu_offdist.py (tools/offdist_reference.py -> profiles/offdist_reference.txt has the figures that chose it)."""
import numpy as np

from diff_vits_amd import synth

GAIN_LOG2_STD = 0.5         # G: log2 of a norm gain ~ N(0, (s G)^2)
OUTLIER_SHARE = 1.0 / 64    # share of the norm channels (and input channels) multiplied up
OUTLIER_FACTOR = 3.5        # OUT: ... by 1 + s OUT
NEGATIVE_SHARE = 1.0 / 64   # share of the norm gains that change sign (severity > 0)
NORM_BIAS_STD = 1.0         # NB
NORM_BIAS_COMMON = 2.0      # NC
BIAS_STD = 1.0              # LB
BIAS_COMMON = 16.0          # LC
TEMB_BIAS_STD = 1.0         # time_emb_proj.bias (the resnet blocks' scale | shift): constants of its own, so that `scale` is O(1)
TEMB_BIAS_COMMON = 1.0      # ... and 1 + scale stays away from both 0 and scale
INPUT_LOG2_STD = 0.5        # IS
INPUT_OFFSET_STD = 4.0      # IO


def _exp2(x):
    """2^x, piecewise linear between the integers, x on a 1 / 16 grid: exact float arithmetic."""
    x = np.round(np.asarray(x, dtype=np.float64) * 16.0) / 16.0
    k = np.floor(x)
    return np.ldexp(1.0 + (x - k), k.astype(np.int64))


def _share(seed, name, n, share):
    """Boolean [n]: about `share` of the entries, hashed."""
    h = synth._stream(seed, name, n)[:, 0]
    return (h >> np.uint64(40)).astype(np.float64) / float(1 << 24) < share


def _common(seed, name):
    """One number per layer, |c| in [0.5, 1), either sign."""
    u = float(synth.uniform(seed, name, (1,))[0])
    return (0.5 + 0.5 * abs(u)) * (1.0 if u >= 0 else -1.0)


def make_state_dict_trained(shapes, seed=1234, severity=1.0):
    """make_state_dict(shapes, seed) with trained-like statistics layered on (module docstring)."""
    base = synth.make_state_dict(shapes, seed=seed)
    s = float(severity)
    out = {}
    for name, v in base.items():
        stem, _, leaf = name.rpartition(".")
        n = v.shape[0] if v.ndim else 1
        is_norm = ("norm" in stem.split(".")[-1]) and v.ndim == 1
        w = v.astype(np.float64)
        if is_norm and leaf == "weight":
            z = synth.normal(seed, name + "/gain", (n,)).astype(np.float64)
            f = _exp2(s * GAIN_LOG2_STD * z) * (1.0 + s * OUTLIER_FACTOR * _share(seed, name + "/outlier", n, OUTLIER_SHARE))
            if s > 0:
                f = np.where(_share(seed, name + "/negative", n, NEGATIVE_SHARE), -f, f)
            w = w * f
        elif leaf == "bias" and v.ndim == 1:
            std, com = (NORM_BIAS_STD, NORM_BIAS_COMMON) if is_norm else (BIAS_STD, BIAS_COMMON)
            if stem.endswith("time_emb_proj"):
                std, com = TEMB_BIAS_STD, TEMB_BIAS_COMMON
            z = synth.normal(seed, name + "/offset", (n,)).astype(np.float64)
            com = np.full(n, com * _common(seed, stem + "/common"))
            if stem.endswith("ff.net.0.proj"):
                com[n // 2:] = 0.0                       # the gate half of GEGLU: spread only
            w = w + s * (std * z + com)
        out[name] = w.astype(np.float32)
    return out


def make_inputs_trained(B, cx, cc, T, L, D, seed=61, severity=1.0):
    """x [B, cx, T], cond [B, cc, T], enc [B, L, D] as float32 arrays: synth.normal(seed, "x" | "c" | "e") - the layer-wise tests'
    inputs - with a per-channel scale, a per-channel offset and a few outlier channels."""
    s = float(severity)
    out = []
    for tag, shape, axis in (("x", (B, cx, T), 1), ("c", (B, cc, T), 1), ("e", (B, L, D), 2)):
        a = synth.normal(seed, tag, shape).astype(np.float64)
        n = shape[axis]
        scale = _exp2(s * INPUT_LOG2_STD * synth.normal(seed, tag + "/scale", (n,)).astype(np.float64))
        scale = scale * (1.0 + s * OUTLIER_FACTOR * _share(seed, tag + "/outlier", n, OUTLIER_SHARE))
        off = s * INPUT_OFFSET_STD * synth.normal(seed, tag + "/offset", (n,)).astype(np.float64)
        bc = (1, n, 1) if axis == 1 else (1, 1, n)
        out.append((a * scale.reshape(bc) + off.reshape(bc)).astype(np.float32))
    return tuple(out)


def timesteps(B):
    """Per-utterance timesteps: fractional, spread over the schedule (the time embedding's sinusoids are O(1) at all of them; with
    trained-like time_emb_proj biases the resnet blocks' `scale` is O(1), which regime_figures measures)."""
    return np.array([949.05 - 310.5 * (b % 3) - 17.25 * (b // 3) for b in range(B)], dtype=np.float32)


SEVERITY_GRID = (0.5, 1.0, 1.5, 2.0, 3.0, 4.0)
# name -> keyword arguments of make_state_dict_trained / make_inputs_trained
PROFILES = {
    "trained": dict(severity=1.0),
}


# ---- the regime, measured on the reference's own fp64 intermediates -----------------------------------------------------------
WIDTHS = (128, 256, 384, 512)


def _level_of(name, widths=WIDTHS):
    parts = name.split(".")
    if parts[0] == "mid_block":
        return len(widths) - 1
    i = int(parts[1])
    return i if parts[0] == "down_blocks" else len(widths) - 1 - i


def regime_figures(probes, groups=8):
    """From oracle_probes' dict (channels-last [B, T, C] tensors, fp64): the median over the rows of |mean| / sigma at the input
    of every LayerNorm (`proj_in` feeds norm1, `attn1` norm2, `attn2` norm3), and the median over (utterance, group) of
    |group mean| / group sigma at the input of every GroupNorm whose input is a probe (`conv1` feeds a resnet block's norm2,
    `resnets.j` the transformer's norm).  Returns {"ln": {name: (C, figure)}, "gn": {name: (level, figure)},
    "ln_by_width": {C: best}, "gn_by_level": {level: best}}."""
    ln, gn = {}, {}
    for name, v in probes.items():
        if v.dim() != 3 or name in ("emb", "conv_in"):
            continue
        a = v.detach().double().numpy()
        leaf = name.split(".")[-1]
        if leaf in ("proj_in", "attn1", "attn2"):
            r = np.abs(a.mean(-1)) / np.maximum(a.std(-1), 1e-300)
            ln[name] = (a.shape[-1], float(np.median(r)))
        is_resnet = name.split(".")[-2:-1] == ["resnets"]
        if leaf == "conv1" or (is_resnet and (name.replace("resnets", "attentions") + ".proj_in") in probes):
            Bn, Tn, C = a.shape
            g = a.reshape(Bn, Tn, groups, C // groups)
            r = np.abs(g.mean((1, 3))) / np.maximum(g.std((1, 3)), 1e-300)
            gn[name] = (_level_of(name), float(np.median(r)))
    by_w, by_l = {}, {}
    for c, f in ln.values():
        by_w[c] = max(by_w.get(c, 0.0), f)
    for lvl, f in gn.values():
        by_l[lvl] = max(by_l.get(lvl, 0.0), f)
    return {"ln": ln, "gn": gn, "ln_by_width": by_w, "gn_by_level": by_l}


REGIME_MIN = 3.0            # condition (c): median |mean| / sigma reached at one LayerNorm of every width, one GroupNorm per level


def regime_reached(fig, widths=WIDTHS):
    return (all(fig["ln_by_width"].get(c, 0.0) >= REGIME_MIN for c in widths) and
            all(fig["gn_by_level"].get(lvl, 0.0) >= REGIME_MIN for lvl in range(len(widths))))


def reference_margins(probes32, y32, probes64, y64):
    """Condition (a) / (b): the fp32 oracle against the fp64 oracle on every probe and y.  Returns (lines, worst) with
    worst = {"rel_l2", "frame", "ratio"} (the largest of each over the probes) and "floored_ok"."""
    from parity_metrics import frame_errors
    lines, worst = [], {"rel_l2": 0.0, "frame": 0.0, "ratio": 0.0, "floored_ok": True}
    items = [(n, probes32[n], probes64[n]) for n in probes64] + [("y", y32.permute(0, 2, 1), y64.permute(0, 2, 1))]
    for n, g, w in items:
        fe = frame_errors(g, w)
        ratio = fe["worst"] / max(fe["rel_l2"], 1e-300)
        lines.append("%-58s rel_l2 %.3e worst_frame %.3e ratio %5.2f floored %d/%d" % (n, fe["rel_l2"], fe["worst"], ratio, fe["floored"], fe["frames"]))
        worst["rel_l2"] = max(worst["rel_l2"], fe["rel_l2"])
        worst["frame"] = max(worst["frame"], fe["worst"])
        if fe["frames"] > 1:
            worst["ratio"] = max(worst["ratio"], ratio)
        worst["floored_ok"] = worst["floored_ok"] and fe["floored_ok"]
    return lines, worst


def margins_ok(worst):
    """(a): inside a third of each bound the layer-wise tests apply; (b): the floor guard."""
    from parity_metrics import FRAME_BOUND, LOCALISATION_BOUND
    return (worst["rel_l2"] < 2e-4 / 3 and worst["frame"] < FRAME_BOUND / 3 and worst["ratio"] < LOCALISATION_BOUND / 3 and
            worst["floored_ok"])


# ---- the shapes of tests/test_gpu_offdist.py, and one call that makes a case's weights and inputs --------------------------------
_FORCE = {"DVITS_CONV3_MIN_TILES": "1", "DVITS_QKV_SPLIT_MIN_WG": "1", "DVITS_FF_SPLIT_MIN_WG": "1"}
CASES = {
    # pitches 320 / 160 / 96 / 64: k_chain_ff, the 32-row forms of k_ff_split<256 | 512>, <384> refused (the merged GEMM)
    "padded-3x300": (3, 300, 77, dict(_FORCE)),
    # pitches 512 / 256 / 128 / 64, whole 64-row blocks on every level: k_ff_split<384>, k_qkv_split's head, tail and xa modes
    "blocks64-2x512": (2, 512, 40, dict(_FORCE)),
}


def case_tensors(kw, B, T, L, seed=1234, **profile):
    """(state dict, sample [B, Cin, T], t [B], enc [B, L, D], mask [B, L]) as torch tensors: trained-like weights and inputs of one
    profile, the ragged prompt mask of the layer-wise tests."""
    import torch
    from diff_vits_amd.unet1d.unet_1d_condition import UNet1DConditionModel
    with torch.device("meta"):
        shapes = {k: tuple(v.shape) for k, v in UNet1DConditionModel(**kw).state_dict().items()}
    sd = {k: torch.from_numpy(v) for k, v in make_state_dict_trained(shapes, seed=seed, **profile).items()}
    cx = kw["out_channels"]
    x, cond, enc = (torch.from_numpy(a) for a in make_inputs_trained(B, cx, kw["in_channels"] - cx, T, L, kw["cross_attention_dim"], **profile))
    mask = torch.ones(B, L, dtype=torch.bool)
    for b in range(B):
        mask[b, max(1, L - 3 * b):] = False
    return sd, torch.cat([x, cond], 1), torch.from_numpy(timesteps(B)), enc, mask


def oracle_pair(kw, sd, sample, t, enc, mask):
    """The oracle in fp32 and in fp64 on the same case: ((y32, probes32), (y64, probes64))."""
    import torch
    from parity_metrics import oracle_probes
    with torch.no_grad():
        r32 = oracle_probes(kw, sd, sample, t, enc, mask)
        r64 = oracle_probes(kw, {k: v.double() for k, v in sd.items()}, sample.double(), t.double(), enc.double(), mask)
    return r32, r64
