"""Cases, seeded weights and the reference of the native posterior encoder's tests (dv_qenc_*, csrc/kernels_wn.hip, csrc/qenc.hip).
Shared by tests/test_qenc_cpu.py, tests/test_gpu_qenc_layerwise.py and tests/test_gpu_qenc.py.

THE REFERENCE is the package's own torch PosteriorEncoder on the CPU (tests/test_align_cpu.py::test_posterior_encoder_mirror pins
that module to the reference's golden), in float32 and in float64, with forward hooks: `pre` (masked), `layerN.acts` (the input of
res_skip_layers[N], masked), and from the output h of res_skip_layers[N] the module's own updates restated in its dtype and order,
`layerN.x` = (x + h[:, :H]) * mask and `layerN.skip` = skip + h[:, H:] (masked for the comparison: the module masks the sum once at
the end, the engine keeps padding rows at zero after every layer).  Probes are channels-last [B, T, C].

THE CASES are the smallest shapes that cross each edge of k_wn_layer (BM = 64 rows per tile, a two-row halo on each side).

THE WEIGHTS: PyTorch-default-like convolution weights w through synth.make_state_dict, stored the way weight_norm initialises
them: weight_v = w, weight_g = ||w|| per output channel.
"""
import numpy as np
import torch

from diff_vits_amd import synth
from diff_vits_amd.model3 import PosteriorEncoder

BM = 64
_REF = {}                    # what is computed once and shared: references, folded weights, the localisation bound
CFG = dict(in_channels=100, out_channels=128, hidden_channels=256, kernel_size=5, dilation_rate=1, n_layers=16, gin_channels=256)

# name: (T, lengths)
CASES = {
    "t1": (1, [1]),
    "t2": (2, [2]),                                  # the halo is longer than the utterance
    "t5": (5, [5]),
    "bm_minus_1": (BM - 1, [BM - 1]),
    "bm": (BM, [BM]),
    "bm_plus_1": (BM + 1, [BM + 1]),
    "two_bm_plus_1": (2 * BM + 1, [2 * BM + 1]),
    "ragged": (2 * BM + 2, [BM + 1, BM + 2, 2 * BM + 2]),   # utterances end 1 and 2 rows into a tile: the halo straddles the end
    "zero_between": (40, [40, 0, 33]),
    "batch4": (300, [300, 257, 192, 31]),
}


def probe_names(n_layers=CFG["n_layers"]):
    names = ["pre"]
    for i in range(n_layers):
        names += ["layer%d.acts" % i] + (["layer%d.x" % i] if i < n_layers - 1 else []) + ["layer%d.skip" % i]
    return names + ["proj"]


def make_weights(seed=4321):
    """{name relative to enc_q.: float32 array} for CFG."""
    c = CFG
    H, L = c["hidden_channels"], c["n_layers"]
    shapes = {"pre.weight": (H, c["in_channels"], 1), "pre.bias": (H,), "proj.weight": (2 * c["out_channels"], H, 1),
              "proj.bias": (2 * c["out_channels"],), "enc.cond_layer.weight": (2 * H * L, c["gin_channels"], 1),
              "enc.cond_layer.bias": (2 * H * L,)}
    for i in range(L):
        shapes["enc.in_layers.%d.weight" % i] = (2 * H, H, c["kernel_size"])
        shapes["enc.in_layers.%d.bias" % i] = (2 * H,)
        n2 = 2 * H if i < L - 1 else H
        shapes["enc.res_skip_layers.%d.weight" % i] = (n2, H, 1)
        shapes["enc.res_skip_layers.%d.bias" % i] = (n2,)
    raw = synth.make_state_dict(shapes, seed=seed)
    sd = {}
    for k, v in raw.items():
        if k.startswith("enc.") and k.endswith(".weight"):
            stem = k[:-len(".weight")]
            sd[stem + ".weight_v"] = v
            sd[stem + ".weight_g"] = np.sqrt((v.astype(np.float64) ** 2).sum((1, 2), keepdims=True)).astype(np.float32)
        else:
            sd[k] = v
    return sd


def make_module(sd=None, dtype=torch.float32, backend=None):
    m = PosteriorEncoder(CFG["in_channels"], CFG["out_channels"], CFG["hidden_channels"], CFG["kernel_size"], CFG["dilation_rate"],
                         CFG["n_layers"], CFG["gin_channels"], **({} if backend is None else {"backend": backend}))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in (sd or make_weights()).items()})
    return m.to(dtype).eval()


def make_inputs(name):
    """y [B, 100, T] (mel-like: unit scale), lengths int64 [B], g [B, 256], noise [B, 128, T] - float32 arrays."""
    T, lengths = CASES[name]
    B = len(lengths)
    return (synth.normal(55, name + ".y", (B, CFG["in_channels"], T)), np.array(lengths, np.int64),
            synth.normal(55, name + ".g", (B, CFG["gin_channels"]), std=0.5), synth.normal(55, name + ".noise", (B, CFG["out_channels"], T)))


def reference(module, y, lengths, g, noise):
    """-> ({probe name: [B, T, C]}, z, m, logs) of `module` (CPU, its dtype) on float32 inputs; g may be None."""
    dt = next(module.parameters()).dtype
    wn, H, L = module.enc, module.enc.hidden_channels, module.enc.n_layers
    yt, gt, nt = (None if a is None else torch.from_numpy(np.asarray(a)).to(dt) for a in (y, g, noise))
    lt = torch.from_numpy(np.asarray(lengths))
    mask = (torch.arange(yt.shape[2])[None, :] < lt[:, None]).to(dt).unsqueeze(1)
    acts, hs, taps = {}, {}, {}

    def tap(store, key):
        def hook(mod, inp, out):                                 # (returns None: the output is not replaced)
            store[key] = out
            acts[key] = inp[0]
        return hook

    hooks = [module.pre.register_forward_hook(tap(taps, "pre")), module.proj.register_forward_hook(tap(taps, "proj"))]
    hooks += [wn.res_skip_layers[i].register_forward_hook(tap(hs, i)) for i in range(L)]
    with torch.no_grad():
        z, m, logs, _ = module(yt, lt, None if gt is None else gt.unsqueeze(-1), noise=nt)
    for h in hooks:
        h.remove()
    cl = lambda t: (t * mask).transpose(1, 2).contiguous()       # noqa: E731
    out = {"pre": cl(taps["pre"]), "proj": cl(taps["proj"])}
    x = taps["pre"] * mask
    skip = torch.zeros_like(x)
    for i in range(L):
        out["layer%d.acts" % i] = cl(acts[i])
        if i < L - 1:
            x = (x + hs[i][:, :H]) * mask
            skip = skip + hs[i][:, H:]
            out["layer%d.x" % i] = cl(x)
        else:
            skip = skip + hs[i]
        out["layer%d.skip" % i] = cl(skip)
    return out, z, m, logs


def case_reference(name, with_g, dtype):
    """reference() of a case, computed once per (case, g, dtype) and shared; the caller must not modify it."""
    key = (name, with_g, dtype)
    if key not in _REF:
        if ("module", dtype) not in _REF:
            _REF[("module", dtype)] = make_module(dtype=dtype)
        y, lengths, g, noise = make_inputs(name)
        _REF[key] = reference(_REF[("module", dtype)], y, lengths, g if with_g else None, noise)
    return _REF[key]


def valid_rows(lengths):
    """Indices of the utterances that hold at least one frame (parity_metrics takes lengths >= 1)."""
    return [b for b, n in enumerate(lengths) if n >= 1]


# ---- the documented arithmetic of the engine, restated on the host (csrc/kernels_wn.hip, csrc/qenc.hip) ---------------------------
# emulate=False: the forward in float64 from the float32 parameters (the restatement; test_qenc_cpu.py holds it against the torch
# module in float64).  emulate=True: what the kernels are documented to do - weight norm folded in float32; every contraction
# operand as two bf16 planes (hi = bf16(v), lo = bf16(v - hi)), the three products hi*hi + hi*lo + lo*hi accumulated in float32;
# bias, conditioning, residual and skip updates in float32; tanh / sigmoid by the kernel's expf forms in float32.  What the
# device's expf and division may add to those forms is the header's stated error WN_ACT_ERR per gated activation; it enters the
# acts bound below as a term of its own.  `fault` plants what the kernel could get wrong (FAULTS).
WN_ACT_ERR = 4.5e-7          # |error of tanh(a) * sigmoid(b)| the header of csrc/kernels_wn.hip states for its two forms
FAULTS = ("halo_across_utterances", "gate_pairs_shifted", "cond_wrong_layer", "last_layer_half", "acts_lost_lo", "x_in_place")


def _bf16(v32):
    u = v32.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32)


def _planes32(v):
    v32 = np.ascontiguousarray(v, np.float32)
    hi = _bf16(v32)
    return hi, _bf16(v32 - hi)


def _mm(x, W, emulate, lo=True):
    """x [..., K] times W [N, K]^T."""
    if not emulate:
        return np.asarray(x, np.float64) @ np.asarray(W, np.float64).T
    xh, xl = _planes32(x)
    wh, wl = _planes32(W)
    out = xh @ wh.T + xh @ wl.T
    return (out + xl @ wh.T) if lo else out


def folded(sd, stem, emulate):
    """weight_g * weight_v / ||weight_v|| (float32 as k_wn_fold, or float64), computed once per weight set and shared."""
    key = ("fold", id(sd), stem, emulate)
    if key not in _REF:
        _REF[key] = _fold(sd, stem, emulate)
    return _REF[key]


def _fold(sd, stem, emulate):
    v, g = sd[stem + ".weight_v"], sd[stem + ".weight_g"]
    if emulate:
        n = np.sqrt((v * v).sum((1, 2), keepdims=True, dtype=np.float32))
        return (v * (g / n)).astype(np.float32)
    v, g = v.astype(np.float64), g.astype(np.float64)
    return v * (g / np.sqrt((v * v).sum((1, 2), keepdims=True)))


def _shifted(x, s, flat):
    """x [B, T, H] (padding rows zero) read at frame t + s; zeros beyond the utterance - or (flat: the halo fault) whatever row
    m + s of the flattened row space holds."""
    B, T, H = x.shape
    src = x.reshape(1, B * T, H) if flat else x
    out = np.zeros_like(src)
    n = src.shape[1]
    if s >= 0:
        out[:, :n - s] = src[:, s:]
    else:
        out[:, -s:] = src[:, :n + s]
    return out.reshape(B, T, H)


def gated(x, lengths, W5, b1, cond, emulate, fault=None, x_new=None):
    """Steps 1-4 of k_wn_layer for the layer input x [B, T, H] (padding rows zero): the gated activations [B, T, H], masked.
    W5 [2H, H, 5] folded, b1 [2H], cond [B, 2H] or None.  x_new: this layer's correct output, for the x_in_place fault - a tile's
    upper halo then holds rows its neighbour has already overwritten."""
    B, T, H = x.shape
    dt = np.float32 if emulate else np.float64
    mask = (np.arange(T)[None, :] < np.asarray(lengths)[:, None]).astype(dt)[:, :, None]
    a = np.zeros((B, T, 2 * H), dt)
    for k in range(5):
        xs = _shifted(x, k - 2, fault == "halo_across_utterances")
        if fault == "x_in_place" and k < 2:
            t = np.arange(T)
            stale = (t >= BM) & ((t % BM) + k - 2 < 0)           # rows whose tap k reads the previous tile
            xs = xs.copy()
            xs[:, stale] = _shifted(x_new, k - 2, False)[:, stale]
        a = a + _mm(xs, W5[:, :, k], emulate).astype(dt)
    a = a + b1.astype(dt)
    if cond is not None:
        a = a + cond.astype(dt)[:, None, :]
    ta, sb = a[..., :H], a[..., H:]
    if fault == "gate_pairs_shifted":
        sb = np.roll(sb, -1, axis=-1)
    if emulate:
        e = np.exp(np.float32(-2.0) * np.abs(ta))
        th = np.copysign((np.float32(1) - e) / (np.float32(1) + e), ta)
        with np.errstate(over="ignore"):
            sg = np.float32(1) / (np.float32(1) + np.exp(-sb))
    else:
        th, sg = np.tanh(ta), 1.0 / (1.0 + np.exp(-sb))
    return (th * sg * mask).astype(dt)


def emulate_forward(sd, y, lengths, g, noise, emulate=True, fault=None):
    """-> ({probe: [B, T, C] float64}, z, m, logs [B, C, T] float64) of the whole engine."""
    c = CFG
    H, L, C = c["hidden_channels"], c["n_layers"], c["out_channels"]
    dt = np.float32 if emulate else np.float64
    B, _, T = y.shape
    mask = (np.arange(T)[None, :] < np.asarray(lengths)[:, None]).astype(dt)[:, :, None]
    cond = None
    if g is not None:
        wc = folded(sd, "enc.cond_layer", emulate)[:, :, 0]
        cond = (g.astype(dt) @ wc.astype(dt).T + sd["enc.cond_layer.bias"].astype(dt)).astype(dt)     # exact fp32 dots in the kernel
    x = ((_mm(np.swapaxes(y, 1, 2), sd["pre.weight"][:, :, 0], emulate).astype(dt) + sd["pre.bias"].astype(dt)) * mask).astype(dt)
    out = {"pre": x}
    skip = np.zeros_like(x)
    for i in range(L):
        W5, b1 = folded(sd, "enc.in_layers.%d" % i, emulate), sd["enc.in_layers.%d.bias" % i]
        W1, b2 = folded(sd, "enc.res_skip_layers.%d" % i, emulate)[:, :, 0], sd["enc.res_skip_layers.%d.bias" % i]
        j = (i + 1) % L if fault == "cond_wrong_layer" else i
        cs = None if cond is None else cond[:, 2 * H * j:2 * H * (j + 1)]
        last = i == L - 1

        def rest(acts):
            h = (_mm(acts, W1, emulate, lo=fault != "acts_lost_lo").astype(dt) + b2.astype(dt)).astype(dt)
            if last:
                if fault == "last_layer_half":
                    h = h * (np.arange(H) < H // 2)
                return None, (skip + h * mask).astype(dt)
            return ((x + h[..., :H]) * mask).astype(dt), (skip + h[..., H:] * mask).astype(dt)

        acts = gated(x, lengths, W5, b1, cs, emulate, None if fault == "x_in_place" else fault)
        if fault == "x_in_place" and not last:
            acts = gated(x, lengths, W5, b1, cs, emulate, fault, x_new=rest(acts)[0])
        out["layer%d.acts" % i] = acts
        xn, skip = rest(acts)
        if not last:
            x = xn
            out["layer%d.x" % i] = x
        out["layer%d.skip" % i] = skip
    st = ((_mm(skip, sd["proj.weight"][:, :, 0], emulate).astype(dt) + sd["proj.bias"].astype(dt)) * mask).astype(dt)
    out["proj"] = st
    m, logs = np.swapaxes(st[..., :C], 1, 2), np.swapaxes(st[..., C:], 1, 2)
    z = ((m + noise.astype(dt) * np.exp(logs)) * np.swapaxes(mask, 1, 2)).astype(dt)
    return {k: v.astype(np.float64) for k, v in out.items()}, z.astype(np.float64), m.astype(np.float64), logs.astype(np.float64)


def acts_in_isolation(sd, layer, x_in, lengths, g, emulate):
    """The gated activations of `layer` from ITS OWN input x_in [B, T, H] (a probe: `pre` or `layer{N-1}.x`), float64 array."""
    H = CFG["hidden_channels"]
    cs = None
    if g is not None:
        dt = np.float32 if emulate else np.float64
        wc = folded(sd, "enc.cond_layer", emulate)[2 * H * layer:2 * H * (layer + 1), :, 0]
        cs = g.astype(dt) @ wc.astype(dt).T + sd["enc.cond_layer.bias"][2 * H * layer:2 * H * (layer + 1)].astype(dt)
    x = np.asarray(x_in, np.float32 if emulate else np.float64)
    return gated(x, lengths, folded(sd, "enc.in_layers.%d" % layer, emulate), sd["enc.in_layers.%d.bias" % layer], cs, emulate).astype(np.float64)


def acts_errors(got, want, lengths):
    """Per-frame errors of gated activations over the valid frames, relative to max(||want frame||, parity_metrics' floor):
    (worst frame of got, the share WN_ACT_ERR can have of a frame: WN_ACT_ERR * sqrt(H) over the smallest denominator)."""
    import parity_metrics as pm
    rows = valid_rows(lengths)
    n = [lengths[b] for b in rows]
    sv = pm.split_valid(np.asarray(got)[rows], np.asarray(want)[rows], n)
    fe = pm.frame_errors(sv["got"], sv["want"])
    wn = np.sqrt((sv["want"] ** 2).sum(-1))
    floor = pm.FLOOR_FRACTION * np.sqrt((wn * wn).mean())
    return fe["worst"], WN_ACT_ERR * np.sqrt(got.shape[-1]) / max(float(np.maximum(wn, floor).min()), 1e-300)


def acts_bound(emulated, want, lengths):
    """Per-frame bound for `layerN.acts` against the float64 activations of the same layer input: twice the worst frame of the
    host emulation of the documented arithmetic (the device accumulates the same products in another order; the factor as
    parity_metrics.isolated_bound argues it), plus what WN_ACT_ERR can add to a frame, plus 2^-16 (isolated_bound's own term)."""
    worst, transcendental = acts_errors(emulated, want, lengths)
    return 2.0 * worst + transcendental + 2.0 ** -16


def localisation_bound():
    """3 x the largest localisation ratio of the float32 reference against the float64 one: every probe and z / m / logs of every
    case, with g and without, valid frames.  -> (bound, lines of the report, largest whole-tensor figure, largest frame figure)."""
    import parity_metrics as pm
    if "loc" not in _REF:
        lines, worst, wt, wf = [], 0.0, 0.0, 0.0
        for name, (T, lengths) in CASES.items():
            rows = valid_rows(lengths)
            n = [lengths[b] for b in rows]
            for with_g in (True, False):
                r32, r64 = case_reference(name, with_g, torch.float32), case_reference(name, with_g, torch.float64)
                pairs = [(k, r32[0][k], r64[0][k]) for k in probe_names()]
                pairs += [(k, a.transpose(1, 2), b.transpose(1, 2)) for k, a, b in zip(("z", "m", "logs"), r32[1:], r64[1:])]
                for k, a, b in pairs:
                    sv = pm.split_valid(a[rows], b[rows], n)
                    fe = pm.frame_errors(sv["got"], sv["want"])
                    loc = fe["worst"] / max(fe["rel_l2"], 1e-300)
                    worst, wt, wf = max(worst, loc), max(wt, fe["rel_l2"]), max(wf, fe["worst"])
                    lines.append("%-36s tensor %.3e  worst frame %.3e  localisation %.2f"
                                 % ("%s/%s %s" % (name, "g" if with_g else "-", k), fe["rel_l2"], fe["worst"], loc))
        _REF["loc"] = (3 * worst, lines, wt, wf)
    return _REF["loc"]
