"""Trained-like weight and input statistics for the two encoder engines (plain helper module: no fixtures, no hooks): the text
encoder (dv_tenc_*, tests/tenc_cases.py) and the prompt encoder in both flavours (dv_penc_*, tests/prompt_cases.py).

tests/offdist_cases.py layers trained-like statistics on synth.make_state_dict for the denoiser; it knows a norm by "norm" in the
last stem component and by the leaves weight / bias.  That already covers the prompt encoder (layer_norm*.weight / .bias, the
biases of pre.conv, ffn_1.0, ffn_2 and out_proj.conv; its MultiheadAttention has no bias at all) and every conv bias of the text
encoder - conv_q / conv_k / conv_v included, so BIAS_COMMON reaches the attention logits there.  make_enc_state_dict_trained calls
it unchanged and adds, from the same hashed streams and the same exact arithmetic:

  *.gamma / *.beta    ChannelLayerNorm of the text encoder: the norm gain (log-normal, outliers, a few negative) / norm bias;
  emb*.weight         the three embedding tables [n, H]: per-channel scale 2^(s IS z), outliers, and a per-channel offset
                      s IO z / sqrt(H) (the tables are multiplied by sqrt(H): the offset is IO in the units of the sum);
  emb_rel_k / _v      a per-channel gain 2^(s (REL_LOG2_GAIN + G z)): trained tables are several times the initial +-0.1;
  ReLU biases         ffn_layers.N.conv_1.bias and ffn.ffn_1.0.bias get the spread but no common offset (as the GEGLU gate there);
  logit_gain          a power of two on the query projection (conv_q.weight and .bias; the q rows of in_proj_weight): attention
                      is made peaked independently of the rest.

Inputs: the speaker vector g and the prompt get make_inputs_trained's per-channel scale, offset and outliers.
severity = 0 and logit_gain = 1 give tc.state_dict() / pc.state_dict() and tc.inputs / pc.inputs bit for bit
(tests/test_offdist_enc_reference.py asserts it, and that the denoiser's trained profile is what it was).

PROFILES: per engine the largest (severity, logit gain) of GRID at which the fp32 oracle against the fp64 oracle stays inside a
third of every criterion of the GPU test on every probe of its cases (tools/offdist_enc_reference.py ->
profiles/offdist_enc_reference.txt has the figures that chose them and the regime they reach).

The second half restates one layer of either encoder in fp64 from the state-dict weights (tenc_layer_fp64, penc_layer_fp64).
They give the regime figures (row |mean| / sigma at every LayerNorm input, top-1 probability and max |logit| of every attention)
and carry the planted faults of tests/test_offdist_enc_reference.py (FAULTS)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from diff_vits_amd import synth

import offdist_cases as oc
import prompt_cases as pc
import tenc_cases as tc
from parity_metrics import FRAME_BOUND, masked_frame_errors

REL_LOG2_GAIN = 2.0         # emb_rel_k / emb_rel_v: the common part of the gain, 2^(s REL_LOG2_GAIN)

SEVERITIES = (0.5, 1.0, 1.5, 2.0)
LOGIT_GAINS = (1.0, 2.0, 4.0, 8.0)
GRID = [(s, g) for s in SEVERITIES for g in LOGIT_GAINS]          # ascending: the "largest" point is the last that qualifies

# engine -> keyword arguments of make_enc_state_dict_trained / the input makers (profiles/offdist_enc_reference.txt)
PROFILES = {
    "tenc": dict(severity=1.5, logit_gain=1.0),
    # NOT chosen by the rule: a second, milder text-encoder point whose softmax is peaked but not saturated (median top-1
    # probability 0.84 at layer 0, 0.04 - 0.13 elsewhere), so that an error in the logits still shows in the layer's output
    "tenc-mild": dict(severity=0.5, logit_gain=1.0),
    "penc": dict(severity=2.0, logit_gain=8.0),
}
# Largest localisation ratio (worst valid frame / whole tensor) the reference side shows against itself - the oracle in fp32
# against the oracle in fp64 - on THESE weights, every probe and output of every case below: profiles/offdist_enc_reference.txt
# (tools/offdist_enc_reference.py asserts the figures here are the ones it measures).  The bound for the HIP path is 3 x that: the
# rule of TENC_LOCALISATION_BOUND / PENC_LOCALISATION_BOUND.
LOCALISATION_REF_MAX = {"tenc": 7.64, "tenc-mild": 2.57, "penc": 2.90}
LOCALISATION_BOUND = {k: 3 * v for k, v in LOCALISATION_REF_MAX.items()}

TENC_CASES = ["3x75", "3x33"]                                      # each with and without g
PENC_CASES = ["D-3x75", "D-2x300", "P-16x99", "P-2x36"]            # each fused and with DVITS_FUSE_LN=0

REGIME_MIN = 3.0            # median row |mean| / sigma at a LayerNorm input of every layer
TOP1_MIN = 0.5              # median top-1 probability of at least one attention per engine, on a case with more than 32 keys


# ---- the generator ----------------------------------------------------------------------------------------------------------------
def _gain(seed, name, n, s, log2_mean=0.0):
    z = synth.normal(seed, name + "/gain", (n,)).astype(np.float64)
    return oc._exp2(s * (log2_mean + oc.GAIN_LOG2_STD * z))


def _norm_gain(seed, name, n, s):
    f = _gain(seed, name, n, s) * (1.0 + s * oc.OUTLIER_FACTOR * oc._share(seed, name + "/outlier", n, oc.OUTLIER_SHARE))
    if s > 0:
        f = np.where(oc._share(seed, name + "/negative", n, oc.NEGATIVE_SHARE), -f, f)
    return f


def _channel_affine(a, seed, tag, axis, s, offset_unit=1.0):
    """a x per-channel scale + per-channel offset (make_inputs_trained's arithmetic), channels on `axis`."""
    n = a.shape[axis]
    scale = oc._exp2(s * oc.INPUT_LOG2_STD * synth.normal(seed, tag + "/scale", (n,)).astype(np.float64))
    scale = scale * (1.0 + s * oc.OUTLIER_FACTOR * oc._share(seed, tag + "/outlier", n, oc.OUTLIER_SHARE))
    off = s * oc.INPUT_OFFSET_STD * offset_unit * synth.normal(seed, tag + "/offset", (n,)).astype(np.float64)
    bc = [1] * a.ndim
    bc[axis] = n
    return (a.astype(np.float64) * scale.reshape(bc) + off.reshape(bc)).astype(np.float32)


def make_enc_state_dict_trained(shapes, seed=1234, severity=1.0, logit_gain=1.0):
    """offdist_cases.make_state_dict_trained(shapes, seed, severity) with the encoders' own names treated as the module docstring
    says.  `shapes` carries the full reference names (enc_p. / prompt_encoder. / o_proj. in front)."""
    out = oc.make_state_dict_trained(shapes, seed=seed, severity=severity)
    base = synth.make_state_dict(shapes, seed=seed)
    s, lg = float(severity), float(logit_gain)
    assert lg > 0 and math.frexp(lg)[0] == 0.5, "the logit gain is a power of two"
    for name, v in list(out.items()):
        stem, _, leaf = name.rpartition(".")
        w = v.astype(np.float64)
        if leaf == "gamma" and v.ndim == 1:
            w = w * _norm_gain(seed, name, v.shape[0], s)
        elif leaf == "beta" and v.ndim == 1:
            z = synth.normal(seed, name + "/offset", v.shape).astype(np.float64)
            w = w + s * (oc.NORM_BIAS_STD * z + oc.NORM_BIAS_COMMON * oc._common(seed, stem + "/common"))
        elif leaf == "weight" and v.ndim == 2 and stem.split(".")[-1] in ("emb", "tone_emb", "language_emb"):
            H = v.shape[1]
            w = _channel_affine(v, seed, name, 1, s, offset_unit=2.0 ** -(int(math.log2(H)) // 2)).astype(np.float64)
        elif leaf in ("emb_rel_k", "emb_rel_v"):
            w = w * _gain(seed, name, v.shape[-1], s, REL_LOG2_GAIN)
        elif leaf == "bias" and stem.split(".")[-1] in ("conv_1", "0") and ".ffn" in stem:
            # the bias in front of the feed-forward's ReLU (ffn_layers.N.conv_1, ffn.ffn_1.0): the spread, no common offset - the
            # exception offdist_cases makes for the GEGLU gate (a common -16 s would switch the whole layer off, +16 s make it linear)
            z = synth.normal(seed, name + "/offset", v.shape).astype(np.float64)
            w = base[name].astype(np.float64) + s * oc.BIAS_STD * z
        if stem.endswith("conv_q"):
            w = w * lg
        elif leaf == "in_proj_weight":
            w = w.copy()
            w[: v.shape[0] // 3] *= lg
        out[name] = w.astype(np.float32)
    return out


def tenc_state_dict(seed=1234, **profile):
    from diff_vits_amd.model3 import TextEncoder
    with torch.device("meta"):
        shapes = {"enc_p." + k: tuple(v.shape) for k, v in TextEncoder(**tc.KW).state_dict().items()}
    return {k[len("enc_p."):]: torch.from_numpy(v) for k, v in make_enc_state_dict_trained(shapes, seed=seed, **profile).items()}


def penc_state_dict(flavour, **profile):
    from diff_vits_amd.model3 import PromptEncoder
    kw, prefix = pc.FLAVOURS[flavour]
    with torch.device("meta"):
        shapes = {prefix + k: tuple(v.shape) for k, v in PromptEncoder(p_dropout=0.2, backend="torch", **kw).state_dict().items()}
    return {k[len(prefix):]: torch.from_numpy(v) for k, v in make_enc_state_dict_trained(shapes, seed=1234, **profile).items()}


def tenc_inputs(B, T, lengths, severity=1.0, logit_gain=1.0):
    """tc.inputs with the speaker vector g [B, gin, 1] scaled and offset per channel."""
    ids, tone, lang, ln, g = tc.inputs(B, T, lengths)
    return ids, tone, lang, ln, torch.from_numpy(_channel_affine(g.numpy(), 1234, "te.g", 1, float(severity)))


def penc_inputs(flavour, B, L, lengths, severity=1.0, logit_gain=1.0):
    """pc.inputs with the prompt [B, C, L] scaled and offset per channel."""
    prompt, ln = pc.inputs(flavour, B, L, lengths)
    return torch.from_numpy(_channel_affine(prompt.numpy(), 1234, "pe.prompt", 1, float(severity))), ln


# ---- one layer of either encoder in fp64, with the regime figures and the planted faults ------------------------------------------
# "ln_var": LayerNorm variance as E[x^2] - mean^2 in fp32;  "k_lo": the lo plane of K dropped (K enters the scores as bf16(K));
# "p_flush": exp(s - max) below fp16's normal range (2^-14) flushed to zero before P V;  "stale_max": the band probabilities of the
# relative value term normalised with the running maximum of the moment their 32-key tile passed, not with the final one (text
# encoder only);  "gamma_sign": LayerNorm uses |gamma|.
FAULTS = ("ln_var", "k_lo", "p_flush", "stale_max", "gamma_sign")


def _valid(ln, T):
    return torch.arange(T)[None, :] < ln[:, None]


def _ln(x, gamma, beta, fault=None, stats=None, name=None, valid=None, eps=1e-5):
    if stats is not None:
        r = (x.mean(-1).abs() / x.std(-1, unbiased=False).clamp_min(1e-300))[valid]
        stats.setdefault("ln", {})[name] = float(r.median())
    if fault == "gamma_sign":
        gamma = gamma.abs()
    if fault == "ln_var":
        x32 = x.float()
        mean = x32.mean(-1, keepdim=True)
        var = ((x32 * x32).mean(-1, keepdim=True) - mean * mean).clamp_min(0.0)
        return ((x32 - mean) * torch.rsqrt(var + eps)).double() * gamma + beta
    return F.layer_norm(x, (x.shape[-1],), gamma, beta, eps)


def _bf16(v):
    return v.float().to(torch.bfloat16).double()


def _softmax_parts(scores, keymask, fault, stats, name, qvalid):
    """scores [B, h, Tq, Tk] fp64, keymask [B, Tk] -> (e = exp(s - max) with masked keys 0, l = its row sum, m = the row max)."""
    scores = scores.masked_fill(~keymask[:, None, None, :], -float("inf"))
    m = scores.amax(-1, keepdim=True)
    e = torch.exp(scores - m)
    l = e.sum(-1, keepdim=True)
    if stats is not None:
        top1 = (1.0 / l[..., 0]).transpose(1, 2)[qvalid]                     # [valid queries, heads]
        big = scores.masked_fill(~keymask[:, None, None, :], 0.0).abs().amax(-1).transpose(1, 2)[qvalid]
        stats.setdefault("attn", {})[name] = (float(top1.median()), float(big.median()), int(keymask.sum(-1).max()), float(big.max()))
    return e, l, m, scores


def tenc_layer_fp64(sd, i, x, ln, g=None, fault=None, stats=None):
    """Layer i of the text encoder on channels-last x [B, T, H] (the probe `emb` or `layer<i-1>`, masked) in fp64, as
    oracle.text_enc_ref computes it -> {"attn", "ln1", "ffn1", "out"} = the probes layerI.attn / .ln1 / .ffn1 / layerI."""
    W = lambda n: sd["encoder." + n].double()        # noqa: E731
    nh, w, ks = tc.KW["n_heads"], tc.WINDOW, tc.KW["kernel_size"]
    x = x.double()
    B, T, H = x.shape
    d = H // nh
    valid = _valid(ln, T)
    keep = valid.double()[:, :, None]
    if i == tc.COND_LAYER and g is not None:
        x = (x + F.linear(g.double().transpose(1, 2), W("spk_emb_linear.weight"), W("spk_emb_linear.bias"))) * keep
    pa = "attn_layers.%d." % i
    q, k, v = (F.linear(x, W(pa + "conv_%s.weight" % n)[:, :, 0], W(pa + "conv_%s.bias" % n)).view(B, T, nh, d).transpose(1, 2) for n in "qkv")
    q = q / math.sqrt(d)
    if fault == "k_lo":
        k = _bf16(k)
    ek, ev = W(pa + "emb_rel_k")[0], W(pa + "emb_rel_v")[0]
    ii, jj = torch.arange(T)[:, None], torch.arange(T)[None, :]
    off = jj - ii + w
    band = (off >= 0) & (off <= 2 * w)
    scores = q @ k.transpose(-1, -2) + (q @ ek.t()).gather(-1, off.clamp(0, 2 * w).expand(B, nh, T, T)) * band
    e, l, m, scores = _softmax_parts(scores, valid, fault, stats, "layer%d" % i, valid)
    ev_e = torch.where(e < 2.0 ** -14, torch.zeros_like(e), e) if fault == "p_flush" else e
    out = (ev_e @ v) / l
    kk = ii + torch.arange(2 * w + 1)[None, :] - w
    kvalid = (kk >= 0) & (kk < T)
    idx = kk.clamp(0, T - 1).expand(B, nh, T, 2 * w + 1)
    pband = e.gather(-1, idx) / l
    if fault == "stale_max":
        # running maximum after the 32-key tile that holds the band key: cummax over the tiles' maxima
        nt = -(-T // 32)
        tm = F.pad(scores, (0, nt * 32 - T), value=-float("inf")).view(B, nh, T, nt, 32).amax(-1).cummax(-1)[0]
        stale = tm.gather(-1, (idx // 32))
        pband = torch.exp(scores.gather(-1, idx) - stale) / l
    pband = pband * (kvalid & (kk < ln.view(B, 1, 1, 1)))
    out = (out + pband @ ev).transpose(1, 2).reshape(B, T, H)
    attn = (x + F.linear(out, W(pa + "conv_o.weight")[:, :, 0], W(pa + "conv_o.bias"))) * keep
    y1 = _ln(attn, W("norm_layers_1.%d.gamma" % i), W("norm_layers_1.%d.beta" % i), fault, stats, "layer%d.norm_1" % i, valid) * keep
    pf = "ffn_layers.%d." % i
    pad = ((ks - 1) // 2, ks // 2)
    conv = lambda a, n: F.conv1d(F.pad(a.transpose(1, 2), pad), W(pf + n + ".weight"), W(pf + n + ".bias")).transpose(1, 2)   # noqa: E731
    h = torch.relu(conv(y1, "conv_1")) * keep
    x2 = y1 + conv(h, "conv_2") * keep
    o = _ln(x2, W("norm_layers_2.%d.gamma" % i), W("norm_layers_2.%d.beta" % i), fault, stats, "layer%d.norm_2" % i, valid) * keep
    return {"attn": attn, "ln1": y1, "ffn1": h, "out": o}


def penc_layer_fp64(sd, i, x, ln, fault=None, stats=None, num_heads=8, kernel_size=9):
    """Layer i of the prompt encoder on x [B, L, C] (the probe `pre` or `layer<i-1>`) in fp64, as oracle.prompt_ref.enc_sa_layer
    computes it -> {"attn", "ffn1", "out"} = the probes layerI.attn / .ffn1 / layerI."""
    p = "layers.%d.op." % i
    W = lambda n: sd[p + n].double()        # noqa: E731
    x = x.double()
    B, L, C = x.shape
    d = C // num_heads
    valid = _valid(ln, L)
    keep = valid.double()[:, :, None]
    n1 = _ln(x, W("layer_norm1.weight"), W("layer_norm1.bias"), fault, stats, "layer%d.layer_norm1" % i, valid)
    q, k, v = (a.view(B, L, num_heads, d).transpose(1, 2) for a in F.linear(n1, W("self_attn.in_proj_weight")).chunk(3, -1))
    q = q * d ** -0.5
    if fault == "k_lo":
        k = _bf16(k)
    e, l, m, _ = _softmax_parts(q @ k.transpose(-1, -2), valid, fault, stats, "layer%d" % i, valid)
    if fault == "p_flush":
        e = torch.where(e < 2.0 ** -14, torch.zeros_like(e), e)
    o = ((e @ v) / l).transpose(1, 2).reshape(B, L, C)
    attn = (x + F.linear(o, W("self_attn.out_proj.weight"))) * keep
    n2 = _ln(attn, W("layer_norm2.weight"), W("layer_norm2.bias"), fault, stats, "layer%d.layer_norm2" % i, valid)
    first = (kernel_size - 1) // 2
    padded = F.pad(n2, (0, 0, first, kernel_size - 1 - first))
    res = 0
    for t in range(kernel_size):
        res = res + F.linear(padded[:, t:L + t] if t else n2, W("ffn.ffn_1.%d.weight" % t), W("ffn.ffn_1.0.bias") if t == 0 else None)
    h = F.relu(res * kernel_size ** -0.5)
    return {"attn": attn, "ffn1": h, "out": (attn + F.linear(h, W("ffn.ffn_2.weight"), W("ffn.ffn_2.bias"))) * keep}


def tenc_layers(sd, probes, ln, g, fault=None, stats=None):
    """Every layer restated from the fp64 oracle's own probe in front of it: {probe name: tensor}."""
    out, n = {}, tc.KW["n_layers"]
    for i in range(n):
        r = tenc_layer_fp64(sd, i, probes["emb"] if i == 0 else probes["layer%d" % (i - 1)], ln, g, fault, stats)
        out.update({"layer%d.attn" % i: r["attn"], "layer%d.ln1" % i: r["ln1"], "layer%d.ffn1" % i: r["ffn1"], "layer%d" % i: r["out"]})
    return out


def penc_layers(sd, probes, ln, n_layers, fault=None, stats=None):
    out = {}
    for i in range(n_layers):
        r = penc_layer_fp64(sd, i, probes["pre"] if i == 0 else probes["layer%d" % (i - 1)], ln, fault, stats)
        out.update({"layer%d.attn" % i: r["attn"], "layer%d.ffn1" % i: r["ffn1"], "layer%d" % i: r["out"]})
    return out


# ---- the oracle pair, the margins and the regime ------------------------------------------------------------------------------------
def tenc_pair(sd, ids, ln, tone, lang, g):
    """The text-encoder oracle in fp32 and in fp64: two {name: [B, T, C]} dicts, the probes and the outputs x, m, logs."""
    res = []
    with torch.no_grad():
        for dt in (torch.float32, torch.float64):
            (x, m, logs), pr = tc.oracle_probes(sd, ids, ln, tone, lang, g, dtype=dt)
            res.append(dict(pr, x=x, m=m, logs=logs))
    return res


def penc_pair(sd, prompt, ln, n_layers):
    from parity_metrics import prompt_oracle_probes
    res = []
    with torch.no_grad():
        for dt in (torch.float32, torch.float64):
            y, pr = prompt_oracle_probes({k: v.to(dt) for k, v in sd.items()}, prompt.to(dt), ln, n_layers)
            res.append(dict(pr, y=y))
    return res


def reference_margins(p32, p64, lengths):
    """The fp32 oracle against the fp64 oracle on the valid frames of every tensor: (lines, worst) with worst = {"rel_l2", "frame",
    "ratio", "floored"} - the largest of each; "floored" is the largest share of valid reference frames on the norm floor."""
    lines, worst = [], {"rel_l2": 0.0, "frame": 0.0, "ratio": 0.0, "floored": 0.0, "ratio_at": ""}
    for n, w in p64.items():
        fe = masked_frame_errors(p32[n], w, lengths)
        ratio = fe["worst"] / max(fe["rel_l2"], 1e-300)
        lines.append("%-14s rel_l2 %.3e worst_frame %.3e ratio %5.2f floored %d/%d" % (n, fe["rel_l2"], fe["worst"], ratio, fe["floored"], fe["frames"]))
        worst["rel_l2"] = max(worst["rel_l2"], fe["rel_l2"])
        worst["frame"] = max(worst["frame"], fe["worst"])
        worst["floored"] = max(worst["floored"], fe["floored"] / fe["frames"])
        if fe["frames"] > 1 and ratio > worst["ratio"]:
            worst["ratio"], worst["ratio_at"] = ratio, n
    return lines, worst


def margins_ok(worst):
    """Inside a third of the whole-tensor and the per-frame bound, and the floor cap itself (1 %).  The localisation bound is 3 x the
    ratio measured here, so the reference is inside a third of it by construction."""
    return worst["rel_l2"] < 2e-4 / 3 and worst["frame"] < FRAME_BOUND / 3 and worst["floored"] <= 0.01


def regime(stats_by_case):
    """stats_by_case: {case: stats of tenc_layers / penc_layers}, all cases of ONE model -> {"ln_per_layer": per layer the best median
    row |mean| / sigma over its LayerNorm inputs and the cases, "ln_min": the smallest of those, "top1": the best median top-1
    probability of an attention over the cases with more than 32 keys, "ln_ok" / "top1_ok" / "ok": REGIME_MIN / TOP1_MIN reached}."""
    per_layer, top1 = {}, 0.0
    for st in stats_by_case.values():
        for name, f in st["ln"].items():
            i = int(name.split(".")[0][len("layer"):])
            per_layer[i] = max(per_layer.get(i, 0.0), f)
        for name, (t1, _, keys, _) in st["attn"].items():
            if keys > 32:
                top1 = max(top1, t1)
    per_layer = [per_layer[i] for i in sorted(per_layer)]
    ln_ok, top1_ok = min(per_layer) >= REGIME_MIN, top1 >= TOP1_MIN
    return {"ln_min": min(per_layer), "ln_per_layer": per_layer, "top1": top1, "ln_ok": ln_ok, "top1_ok": top1_ok, "ok": ln_ok and top1_ok}


def regime_by_model(engine, stats_by_case):
    """The regime per MODEL: the text encoder is one; the prompt encoder's flavours D (4 layers) and P (6 layers) are two models with
    weights of their own, and each is asked for every one of its layers.  Case ids start with the flavour's letter."""
    if engine != "penc":
        return {engine: regime(stats_by_case)}
    return {"penc-" + fl: regime({c: st for c, st in stats_by_case.items() if c.startswith(fl + "-")}) for fl in ("D", "P")}
