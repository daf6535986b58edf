"""Vocoder parity cases (no test functions): the fp64 restatement of the published Vocos model (ConvNeXt-1D backbone, ISTFT
head) with every probe as a return value, its two-plane emulation and planted faults, a weight generator with trained-like
statistics, and the criteria tests/test_gpu_vocoder.py holds the HIP engine to (tests/test_vocoder_cpu.py shows on the CPU which
planted fault each criterion sees).

The restatement runs PER UTTERANCE on mel[b, :, :L_b] with torch.nn.functional and torch.istft in fp64: the definition of the
native path's ragged rule.  emulate=True rounds the operands of the GEMMs (embed, pwconv1, pwconv2 with gamma folded, head.out)
to two bf16 planes (parity_metrics._planes); emulate="bf16" to the hi plane alone.  The depthwise convolution, the LayerNorms
and everything after the head stay exact.
"""
import numpy as np
import torch
import torch.nn.functional as F

import parity_metrics as pm

N_FFT, HOP, BINS = 1024, 256, 513
CFG_FULL = dict(n_mels=100, dim=512, intermediate=1536, n_layers=8, n_fft=N_FFT, hop=HOP)
CFG_SMALL = dict(n_mels=100, dim=128, intermediate=384, n_layers=2, n_fft=N_FFT, hop=HOP)
# (B, T, lengths): a two-frame utterance, an odd length, ragged rows, rows that end one frame apart, rows shorter than the
# filter, more than one overlap-add run, a refused row
CASES = (
    (1, 2, [2]),
    (1, 37, [37]),
    (3, 64, [64, 33, 5]),
    (2, 100, [100, 99]),
    (4, 16, [16, 3, 2, 7]),
    (1, 300, [300]),
    (2, 8, [8, 0]),
)
FAULTS = ("halo", "env_T", "window_twice", "lost_lo", "eps", "clip_before_exp", "imag512")
# Largest localisation ratio (worst frame / whole tensor) of the fp32 restatement against fp64 over every probe of every case
# (profiles/vocoder_reference.txt); the HIP path is held to 3 x that, as parity_metrics.LOCALISATION_BOUND is argued
LOCALISATION_REF_MAX = 1.37
LOCALISATION_BOUND = 3 * LOCALISATION_REF_MAX
WHOLE_BOUND = 2e-4


def case_id(c):
    return "B%d-T%d" % (c[0], c[1])


def probe_names(n_layers):
    names = ["embed", "norm"]
    for i in range(n_layers):
        names += ["l%d.dwln" % i, "l%d.act" % i, "l%d.out" % i]
    return names + ["final", "head"]


def make_weights(cfg, seed=11):
    """A state dict (float32, the published names) with trained-like statistics: LayerNorm gains 1 +- 0.3 with biases, positive
    gamma in 0.05 .. 1, head magnitude rows x 2 with bias -2, phase rows x 3."""
    g = torch.Generator().manual_seed(seed)
    C, I, M, L = cfg["dim"], cfg["intermediate"], cfg["n_mels"], cfg["n_layers"]

    def n(*shape, s=1.0):
        return torch.randn(*shape, generator=g, dtype=torch.float64) * s

    def u(lo, hi, *shape):
        return lo + (hi - lo) * torch.rand(*shape, generator=g, dtype=torch.float64)

    sd = {"backbone.embed.weight": n(C, M, 7, s=(7 * M) ** -0.5), "backbone.embed.bias": n(C, s=0.1)}
    for p in ("backbone.norm.", "backbone.final_layer_norm."):
        sd[p + "weight"], sd[p + "bias"] = u(0.7, 1.3, C), n(C, s=0.1)
    for i in range(L):
        p = "backbone.convnext.%d." % i
        sd[p + "dwconv.weight"], sd[p + "dwconv.bias"] = n(C, 1, 7, s=7 ** -0.5), n(C, s=0.1)
        sd[p + "norm.weight"], sd[p + "norm.bias"] = u(0.7, 1.3, C), n(C, s=0.1)
        sd[p + "pwconv1.weight"], sd[p + "pwconv1.bias"] = n(I, C, s=C ** -0.5), n(I, s=0.1)
        sd[p + "pwconv2.weight"], sd[p + "pwconv2.bias"] = n(C, I, s=I ** -0.5), n(C, s=0.1)
        sd[p + "gamma"] = u(0.05, 1.0, C)
    W, b = n(N_FFT + 2, C, s=C ** -0.5), n(N_FFT + 2, s=0.1)
    W[:BINS] *= 2.0
    b[:BINS] = b[:BINS] - 2.0
    W[BINS:] *= 3.0
    sd["head.out.weight"], sd["head.out.bias"] = W, b
    sd["head.istft.window"] = torch.hann_window(N_FFT, periodic=True, dtype=torch.float64)
    return {k: v.to(torch.float32) for k, v in sd.items()}


def make_mel(B, T, lengths, seed=5, n_mels=100):
    """A denormalised log-mel-like input [B, n_mels, T] (float32): a smooth ramp over the bands plus noise.  Frames at or past a
    row's length hold LARGE values, so that a kernel that reads them is seen."""
    g = torch.Generator().manual_seed(seed + 1000 * B + T)
    mel = -5.0 + 2.0 * torch.randn(B, n_mels, T, generator=g, dtype=torch.float64) - torch.linspace(0, 4, n_mels, dtype=torch.float64)[None, :, None]
    for b, L in enumerate(lengths):
        L = min(max(int(L), 0), T)
        mel[b, :, L:] = 30.0 * torch.randn(n_mels, T - L, generator=g, dtype=torch.float64)
    return mel.to(torch.float32)


def _ln(x, g, b, eps):
    return F.layer_norm(x, (x.shape[-1],), g, b, eps)


def _conv7(xs, T, W, b, groups, halo):
    """The seven-tap convolution of every utterance xs[b] [1, C, L_b] on its own (zeros outside [0, L_b)); halo=True plants the
    fault of a kernel that reads its halo from the neighbouring rows of the row space m = b * T + t."""
    if not halo:
        return [F.conv1d(x, W, b, padding=3, groups=groups) for x in xs]
    cat = torch.cat([F.pad(x, (0, T - x.shape[-1])) for x in xs], dim=-1)
    y = F.conv1d(cat, W, b, padding=3, groups=groups)
    return [y[..., i * T:i * T + x.shape[-1]] for i, x in enumerate(xs)]


def istft_manual(S, window, n_env=None, window_twice=False, imag512=False):
    """torch.istft(center=True) of one utterance by hand: S complex [513, L] -> [(L - 1) * 256].  n_env: frames the envelope is
    taken for (None: L, the utterance's own; the "env_T" fault passes T); window_twice / imag512: planted faults (the window
    applied twice; the imaginary part of bin 512 entering the packed spectrum's bin 0, a constant -Im S[512] / 1024 per frame)."""
    L = S.shape[-1]
    frames = torch.fft.irfft(S.transpose(0, 1), n=N_FFT, dim=-1)
    if imag512:
        frames = frames - (S[BINS - 1].imag / N_FFT)[:, None]
    frames = frames * window
    if window_twice:
        frames = frames * window
    n_env = L if n_env is None else n_env
    y = frames.new_zeros(N_FFT + (max(L, n_env) - 1) * HOP)
    env = torch.zeros_like(y)
    w2 = window * window
    for f in range(L):
        y[f * HOP:f * HOP + N_FFT] += frames[f]
    for f in range(n_env):
        env[f * HOP:f * HOP + N_FFT] += w2
    lo, hi = N_FFT // 2, N_FFT // 2 + (L - 1) * HOP
    return y[lo:hi] / env[lo:hi]


def head_to_wave(logits, window, T=None, fault=None, manual=False):
    """One utterance's head logits [L, 1026] (any float dtype) -> waveform [(L - 1) * 256] in that dtype."""
    m, ph = logits[:, :BINS].transpose(0, 1), logits[:, BINS:].transpose(0, 1)
    mag = torch.exp(torch.clip(m, max=1e2)) if fault == "clip_before_exp" else torch.clip(torch.exp(m), max=1e2)
    S = torch.complex(mag * torch.cos(ph), mag * torch.sin(ph))
    if manual or fault in ("env_T", "window_twice", "imag512"):
        return istft_manual(S, window, n_env=T if fault == "env_T" else None, window_twice=fault == "window_twice", imag512=fault == "imag512")
    return torch.istft(S[None], N_FFT, hop_length=HOP, win_length=N_FFT, window=window, center=True)[0]


def reference(sd, cfg, mel, lengths=None, emulate=False, fault=None, dtype=torch.float64):
    """The restatement.  Returns a dict: every probe of probe_names() as [B, T, C] (zeros on padding rows), "wave"
    [B, (T - 1) * 256] and "samples" [B] (int64).  dtype=torch.float32 with emulate=False: the fp32 torch path."""
    B, _, T = mel.shape
    C, L = cfg["dim"], cfg["n_layers"]
    n = [T] * B if lengths is None else [int(v) for v in lengths]
    ok = [b for b in range(B) if 2 <= n[b] <= T]
    W = {k: v.detach().cpu().to(dtype) for k, v in sd.items()}
    op = (lambda v: pm._operand(v, emulate).to(dtype)) if emulate else (lambda v: v)
    eps = 1e-5 if fault == "eps" else 1e-6
    halo = fault == "halo"
    out = {"wave": torch.zeros(B, (T - 1) * HOP, dtype=dtype), "samples": torch.zeros(B, dtype=torch.int64)}

    def keep(name, xs, channels_first):
        full = torch.zeros(B, T, xs[0].shape[1] if channels_first else xs[0].shape[-1], dtype=dtype)
        for b, x in zip(ok, xs):
            full[b, :n[b]] = x[0].transpose(0, 1) if channels_first else x[0]
        out[name] = full

    xs = [mel[b:b + 1, :, :n[b]].detach().cpu().to(dtype) for b in ok]
    if not ok:
        for name in probe_names(L):
            out[name] = torch.zeros(B, T, {"act": cfg["intermediate"], "head": N_FFT + 2}.get(name.split(".")[-1], C), dtype=dtype)
        return out
    xs = _conv7([op(x) for x in xs], T, op(W["backbone.embed.weight"]), W["backbone.embed.bias"], 1, halo)
    keep("embed", xs, True)
    xs = [_ln(x.transpose(1, 2), W["backbone.norm.weight"], W["backbone.norm.bias"], eps).transpose(1, 2) for x in xs]
    keep("norm", xs, True)
    for i in range(L):
        p = "backbone.convnext.%d." % i
        ys = _conv7(xs, T, W[p + "dwconv.weight"], W[p + "dwconv.bias"], C, halo)
        ys = [_ln(y.transpose(1, 2), W[p + "norm.weight"], W[p + "norm.bias"], eps) for y in ys]
        keep("l%d.dwln" % i, ys, False)
        acts = [F.gelu(F.linear(op(y), op(W[p + "pwconv1.weight"]), W[p + "pwconv1.bias"])) for y in ys]
        keep("l%d.act" % i, acts, False)
        if emulate:      # the engine folds gamma into the fp32 weight (one rounding) before it splits it
            w2 = (W[p + "gamma"].float()[:, None] * W[p + "pwconv2.weight"].float()).to(dtype)
            b2 = (W[p + "gamma"].float() * W[p + "pwconv2.bias"].float()).to(dtype)
        else:
            w2, b2 = W[p + "gamma"][:, None] * W[p + "pwconv2.weight"], W[p + "gamma"] * W[p + "pwconv2.bias"]
        a_op = (lambda a: pm._planes(a, lo=False).to(dtype)) if fault == "lost_lo" else op
        xs = [x + F.linear(a_op(a), op(w2), b2).transpose(1, 2) for x, a in zip(xs, acts)]
        keep("l%d.out" % i, xs, True)
    fs = [_ln(x.transpose(1, 2), W["backbone.final_layer_norm.weight"], W["backbone.final_layer_norm.bias"], eps) for x in xs]
    keep("final", fs, False)
    hs = [F.linear(op(f), op(W["head.out.weight"]), W["head.out.bias"]) for f in fs]
    keep("head", hs, False)
    for b, h in zip(ok, hs):
        y = head_to_wave(h[0], W["head.istft.window"], T=T, fault=fault)
        out["wave"][b, :y.shape[0]] = y
        out["samples"][b] = y.shape[0]
    return out


def wave_blocks(wave, lengths, T):
    """wave [B, (T - 1) * 256] of the rows that hold an utterance -> ([B', T - 1, 256] blocks, their block counts L_b - 1)."""
    n = [int(v) for v in lengths]
    rows = [b for b in range(len(n)) if 2 <= n[b] <= T]
    w = torch.as_tensor(wave).detach().cpu().double()[rows].reshape(len(rows), T - 1, HOP)
    return w, [n[b] - 1 for b in rows]


def probe_failures(name, got, want, lengths, T):
    """The whole-engine criteria of one probe [B, T, C]: 2e-4 whole tensor, FRAME_BOUND on every valid frame, the localisation
    ratio, exact zeros on padding rows.  Returns the list of failures (empty: the probe passes) and the figures."""
    n = [int(v) for v in lengths]
    rows = [b for b in range(len(n)) if 2 <= n[b] <= T]
    g = torch.as_tensor(got).detach().cpu().double()
    fails = []
    dead = [b for b in range(len(n)) if b not in rows]
    if dead and float(g[dead].abs().max()) != 0.0:
        fails.append("%s: a refused row is not zero" % name)
    if not rows:
        return fails, {}
    fe = pm.masked_frame_errors(g[rows], torch.as_tensor(want).double()[rows], [n[b] for b in rows])
    loc = fe["worst"] / max(fe["rel_l2"], 1e-300)
    if not fe["padding_zero"]:
        fails.append("%s: padding frame %s is not zero" % (name, fe["first_nonzero"]))
    if not fe["rel_l2"] <= WHOLE_BOUND:
        fails.append("%s: whole tensor %.3e > %.1e" % (name, fe["rel_l2"], WHOLE_BOUND))
    if not fe["worst"] <= pm.FRAME_BOUND:
        fails.append("%s: worst frame %.3e at %s > %.1e" % (name, fe["worst"], fe["at"], pm.FRAME_BOUND))
    if fe["rel_l2"] > 1e-7 and not loc <= LOCALISATION_BOUND:
        fails.append("%s: localisation %.2f > %.2f (worst frame %.3e at %s, tensor %.3e)" % (name, loc, LOCALISATION_BOUND, fe["worst"], fe["at"], fe["rel_l2"]))
    return fails, {"rel_l2": fe["rel_l2"], "worst": fe["worst"], "loc": loc}


def wave_failures(got, emulated, want, lengths, T, mode=None):
    """The waveform per 256-sample block under isolated_bound(emulated, want); samples at or past n_b exactly zero."""
    fails = []
    g, nb = wave_blocks(got, lengths, T)
    e, _ = wave_blocks(emulated, lengths, T)
    w, _ = wave_blocks(want, lengths, T)
    full = torch.as_tensor(got).detach().cpu()
    for b, L in enumerate(int(v) for v in lengths):
        nvalid = (L - 1) * HOP if 2 <= L <= T else 0
        if float(full[b, nvalid:].abs().max()) != 0.0 if full[b, nvalid:].numel() else False:
            fails.append("wave: row %d holds non-zero samples at or past n_b = %d" % (b, nvalid))
    if not nb:
        return fails, {}
    bound = pm.isolated_bound(pm.split_valid(e, w, nb)["got"], pm.split_valid(e, w, nb)["want"], mode)
    fe = pm.masked_frame_errors(g, w, nb)
    if not fe["rel_l2"] <= bound:
        fails.append("wave: whole tensor %.3e > %.3e" % (fe["rel_l2"], bound))
    if not fe["worst"] <= bound:
        fails.append("wave: worst block %.3e at %s > %.3e" % (fe["worst"], fe["at"], bound))
    return fails, {"rel_l2": fe["rel_l2"], "worst": fe["worst"], "bound": bound}


def engine_failures(got, emulated, want, cfg, lengths, T, mode=None):
    """Every criterion of the whole-engine GPU test on a dict like reference()'s.  mode="bf16": the probes are held to
    isolated_bound against the one-plane emulation instead of the parity-mode figures."""
    fails = []
    for name in probe_names(cfg["n_layers"]):
        if mode == "bf16":
            f, _ = wave_like_probe(name, got[name], emulated[name], want[name], lengths, T)
        else:
            f, _ = probe_failures(name, got[name], want[name], lengths, T)
        fails += f
    f, _ = wave_failures(got["wave"], emulated["wave"], want["wave"], lengths, T, mode)
    fails += f
    n = [(int(v) - 1) * HOP if 2 <= int(v) <= T else 0 for v in lengths]
    if [int(v) for v in torch.as_tensor(got["samples"]).tolist()] != n:
        fails.append("samples: %s != %s" % (torch.as_tensor(got["samples"]).tolist(), n))
    return fails


def wave_like_probe(name, got, emulated, want, lengths, T):
    """bf16 fast mode: a probe per frame under isolated_bound(one-plane emulation, want, mode="bf16")."""
    n = [int(v) for v in lengths]
    rows = [b for b in range(len(n)) if 2 <= n[b] <= T]
    if not rows:
        return [], {}
    ln = [n[b] for b in rows]
    g, e, w = (torch.as_tensor(t).detach().cpu().double()[rows] for t in (got, emulated, want))
    sv = pm.split_valid(e, w, ln)
    bound = pm.isolated_bound(sv["got"], sv["want"], "bf16")
    fe = pm.masked_frame_errors(g, w, ln)
    fails = []
    if not fe["padding_zero"]:
        fails.append("%s: padding frame %s is not zero" % (name, fe["first_nonzero"]))
    if not fe["worst"] <= bound:
        fails.append("%s: worst frame %.3e at %s > %.3e (bf16)" % (name, fe["worst"], fe["at"], bound))
    return fails, {"worst": fe["worst"], "bound": bound}


def block_report(got, want, lengths, T):
    """Per-utterance figures of a waveform against `want`: the worst interior block, and the first / last two blocks (fewer than
    four frames overlap there) named separately.  Returns a list of (row, {"edge": worst, "interior": worst, "peak": |want| max})."""
    g, nb = wave_blocks(got, lengths, T)
    w, _ = wave_blocks(want, lengths, T)
    out = []
    for r, k in enumerate(nb):
        d = (g[r, :k] - w[r, :k]).norm(dim=-1).numpy()
        ref = float(w[r, :k].norm(dim=-1).pow(2).mean().sqrt())
        rel = d / max(ref, 1e-300)
        edge = np.zeros(k, dtype=bool)
        edge[:2] = True
        edge[-2:] = True
        out.append((r, {"edge": float(rel[edge].max()), "interior": float(rel[~edge].max()) if (~edge).any() else 0.0,
                        "per_block": rel, "peak": float(w[r, :k].abs().max()), "rms_block": ref}))
    return out
