"""Parity metrics that localise an error, and the oracle's named intermediates.

A whole-tensor relative L2 is one number over up to 10^6 values; the failure modes of tiled kernels are local - one row block,
one column slice, the frame next to a padding row, one head.  These helpers report the error per frame and per tile-shaped
block, and how much worse the worst frame is than the tensor as a whole (tests/test_parity_metrics.py plants such faults and
shows which criterion sees them).  Plain helper module: no fixtures, no pytest hooks.
"""
import numpy as np
import torch

FLOOR_FRACTION = 0.1        # denominators are floored at this fraction of the rms frame (block) norm of the reference
MAX_FLOORED = 0.01          # at most this share of the frames may sit on that floor (else the metric says little)
FRAME_BOUND = 1e-3          # the project's budget for the denoiser output (BASELINE.json north_star), asked of every frame
# Largest localisation ratio the reference side shows against itself (oracle fp32 vs oracle fp64, every probe, config 1 at
# B = 1, T = 256 and B = 2, T = 100: profiles/parity_localisation_ref.txt), and the bound for the HIP path: 3 x that (the
# split-bf16 / fp16-P noise is not distributed exactly like fp32 rounding, and the maximum over 8 k frames sits further out
# than the maximum over 256)
LOCALISATION_REF_MAX = 1.67
LOCALISATION_BOUND = 3 * LOCALISATION_REF_MAX
# The prompt encoder has a constant of its own: its reference side (oracle.prompt_ref fp32 vs fp64 on every case of
# tests/prompt_cases.py, valid frames, profiles/parity_localisation_penc_ref.txt) reaches 2.01 at layer0.attn of the o_proj flavour
# at B = 8, L = 1024 - above the denoiser's 1.67, the maximum being taken over 3 k - 8 k frames of softmax outputs over up to
# 1024 keys (every other probe of every case stays at or below 1.59).  Same 3 x margin, same reasons.
PENC_LOCALISATION_REF_MAX = 2.01
PENC_LOCALISATION_BOUND = 3 * PENC_LOCALISATION_REF_MAX


def _f64(a):
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().to(torch.float64).numpy()
    return np.asarray(a, dtype=np.float64)


def frame_errors(got, want):
    """Per-frame relative error of channels-last [B, T, C] tensors, in fp64:
    ||got[b,t] - want[b,t]|| / max(||want[b,t]||, floor), floor = 0.1 x the rms frame norm of `want`.
    Returns a dict: worst (the largest per-frame error), at = its (b, t), rel_l2 (whole tensor), floored (frames whose own norm
    is below the floor), frames, floored_ok (floored <= 1 % of the frames), per_frame ([B, T] array)."""
    g, w = _f64(got), _f64(want)
    assert g.shape == w.shape and g.ndim == 3, (g.shape, w.shape)
    wn = np.sqrt((w * w).sum(-1))
    dn = np.sqrt(((g - w) ** 2).sum(-1))
    floor = FLOOR_FRACTION * np.sqrt((wn * wn).mean())
    per = dn / np.maximum(np.maximum(wn, floor), 1e-300)
    i = int(np.argmax(per))
    floored = int((wn < floor).sum())
    return {"worst": float(per.flat[i]), "at": tuple(int(v) for v in np.unravel_index(i, per.shape)),
            "rel_l2": float(np.sqrt((dn * dn).sum()) / max(np.sqrt((wn * wn).sum()), 1e-300)),
            "floored": floored, "frames": int(per.size), "floored_ok": floored <= MAX_FLOORED * per.size, "per_frame": per}


def block_errors(got, want, rows, cols, lengths=None):
    """Relative L2 per rows x cols block of [B, T, C] tensors; the row blocks are laid out per utterance from its first frame (as
    the kernels' row tiles are), the last block of an utterance / of the channels may be short.  Denominators are floored like
    frame_errors'.  With `lengths` ([B]) only the first lengths[b] frames of utterance b count: its last block ends there, and
    the blocks behind it enter neither the maximum nor the floor.
    Returns a dict: worst, utterance, rows (r0, r1), cols (c0, c1) - half-open ranges of the worst block."""
    g, w = _f64(got), _f64(want)
    assert g.shape == w.shape and g.ndim == 3, (g.shape, w.shape)
    B, T, C = w.shape
    n = np.full(B, T) if lengths is None else np.asarray(lengths).astype(np.int64).reshape(B)
    assert n.min() >= 1 and n.max() <= T, n
    rows, cols = min(rows, T), min(cols, C)
    nr, nc = -(-T // rows), -(-C // cols)
    pad = ((0, 0), (0, nr * rows - T), (0, nc * cols - C))
    valid = (np.arange(T)[None, :] < n[:, None])[:, :, None]
    d2 = np.pad((g - w) ** 2 * valid, pad).reshape(B, nr, rows, nc, cols).sum((2, 4))
    w2 = np.pad(w * w * valid, pad).reshape(B, nr, rows, nc, cols).sum((2, 4))
    live = np.broadcast_to((np.arange(nr)[None, :] * rows < n[:, None])[:, :, None], w2.shape)   # blocks with a valid frame
    floor2 = FLOOR_FRACTION ** 2 * w2[live].mean()
    per = np.where(live, np.sqrt(d2 / np.maximum(np.maximum(w2, floor2), 1e-300)), 0.0)
    b, r, c = (int(v) for v in np.unravel_index(int(np.argmax(per)), per.shape))
    return {"worst": float(per[b, r, c]), "utterance": b, "rows": (r * rows, min((r + 1) * rows, int(n[b]))),
            "cols": (c * cols, min((c + 1) * cols, C))}


def split_valid(got, want, lengths):
    """A [B, L, C] pair of a ragged batch (utterance b holds lengths[b] valid frames, then padding that is exactly zero by
    contract) -> a dict:
    got, want - the valid frames, utterance after utterance, as [1, sum(lengths), C] fp64 arrays: what frame_errors and
      localisation take (under frame_errors the zero padding frames would all sit on the norm floor and break its 1 % cap);
    where - [sum(lengths), 2] int array, the (utterance, frame) of every row of those;
    padding_zero - every padding frame of `got` is exactly 0.0;  first_nonzero - the (utterance, frame) of the first one
      that is not, or None."""
    g, w = _f64(got), _f64(want)
    assert g.shape == w.shape and g.ndim == 3, (g.shape, w.shape)
    B, L, C = w.shape
    n = np.asarray(lengths).astype(np.int64).reshape(B)
    assert n.min() >= 1 and n.max() <= L, n
    valid = np.arange(L)[None, :] < n[:, None]
    where = np.argwhere(valid)                                   # row-major: utterance after utterance, frames ascending
    bad = np.argwhere(~valid & (g != 0.0).any(-1))
    return {"got": g[valid][None], "want": w[valid][None], "where": where, "padding_zero": bad.shape[0] == 0,
            "first_nonzero": tuple(int(v) for v in bad[0]) if bad.shape[0] else None}


def masked_frame_errors(got, want, lengths):
    """frame_errors over the valid frames of a ragged batch (split_valid): the floor, its 1 % cap, the whole-tensor figure and
    the worst frame all come from valid frames only; `at` and `per_frame` ([B, L], 0 on padding) are in (utterance, frame)
    coordinates; padding_zero / first_nonzero are split_valid's."""
    sv = split_valid(got, want, lengths)
    fe = frame_errors(sv["got"], sv["want"])
    per = np.zeros(tuple(np.asarray(want).shape[:2]))
    per[sv["where"][:, 0], sv["where"][:, 1]] = fe["per_frame"][0]
    fe.update(at=tuple(int(v) for v in sv["where"][fe["at"][1]]), per_frame=per, padding_zero=sv["padding_zero"],
              first_nonzero=sv["first_nonzero"])
    return fe


def localisation(got, want):
    """Worst-frame error / whole-tensor error.  Rounding noise spread over the tensor gives a small ratio (the tail of a
    distribution over the frames); a fault confined to a few frames gives a large one."""
    fe = frame_errors(got, want)
    return fe["worst"] / max(fe["rel_l2"], 1e-300)


TILE_GEOMETRIES = ((32, 1 << 30), (64, 64), (128, 128))   # 32 rows x all channels (row-block chains), conv / split tiles, GEMM tiles


def describe(name, got, want, lengths=None):
    """One line that says where `got` is furthest from `want`: worst frame, worst block of each tile geometry, whole tensor
    (with `lengths`: over the valid frames of a ragged batch)."""
    fe = frame_errors(got, want) if lengths is None else masked_frame_errors(got, want, lengths)
    parts = ["%s: tensor %.2e, worst frame %.2e at utterance %d frame %d (x%.1f)" %
             (name, fe["rel_l2"], fe["worst"], fe["at"][0], fe["at"][1], fe["worst"] / max(fe["rel_l2"], 1e-300))]
    for rows, cols in TILE_GEOMETRIES:
        be = block_errors(got, want, rows, cols, lengths)
        parts.append("rows %d..%d of utterance %d, columns %d..%d, %.2e" %
                     (be["rows"][0], be["rows"][1] - 1, be["utterance"], be["cols"][0], be["cols"][1] - 1, be["worst"]))
    return "; ".join(parts)


def expected_probes(model):
    """Names of every intermediate the engine registers with DVITS_KEEP_INTERMEDIATES=1, from the module tree, in no particular
    order: emb, conv_in, every resnet and its conv1, every transformer with proj_in / attn1 / attn2 / ff, every resampler."""
    names = ["emb", "conv_in"]
    for n, _ in model.named_modules():
        parts = n.split(".")
        if len(parts) < 2 or not parts[-1].isdigit():
            continue
        kind = parts[-2]
        if kind == "resnets":
            names += [n, n + ".conv1"]
        elif kind == "attentions":
            tb = n + ".transformer_blocks.0."
            names += [n, n + ".proj_in", tb + "attn1", tb + "attn2", tb + "ff"]
        elif kind in ("downsamplers", "upsamplers"):
            names.append(n)
    return names


def one_plane(v):
    """The operand-rounding hook of the bf16 fast mode: v as ONE bf16 plane, in v's own dtype."""
    return v.to(torch.float32).to(torch.bfloat16).to(v.dtype)


class _RoundedOps:
    """`base` (torch.nn.functional, or torch) with every contraction operand passed through `hook` first: linear, conv1d, matmul,
    and scaled_dot_product_attention restated as its two products - q d^-1/2 and k rounded, the mask added to the logits, exp(s - max)
    and v rounded, the denominator from the unrounded exponentials.  Everything else is `base`'s own: torch.einsum among it, so the
    two small products of the pooled text embedding (oracle/unet_ref.py text_time_embedding) keep their operands unrounded."""

    def __init__(self, base, hook):
        self._base, self._hook = base, hook

    def __getattr__(self, name):
        return getattr(self._base, name)

    def linear(self, x, w, b=None):
        return self._base.linear(self._hook(x), self._hook(w), b)

    def conv1d(self, x, w, b=None, **kwargs):
        return self._base.conv1d(self._hook(x), self._hook(w), b, **kwargs)

    def matmul(self, a, b):
        return self._base.matmul(self._hook(a), self._hook(b))

    def scaled_dot_product_attention(self, q, k, v, attn_mask=None, dropout_p=0.0, is_causal=False):
        assert dropout_p == 0.0 and not is_causal
        s = self._hook(q * q.shape[-1] ** -0.5) @ self._hook(k).transpose(-1, -2)
        if attn_mask is not None:
            s = s + attn_mask
        pr = torch.exp(s - s.amax(-1, keepdim=True))
        return (self._hook(pr) @ self._hook(v)) / pr.sum(-1, keepdim=True)


def _hooked(R, hook):
    """Module attributes of the oracle module R to swap while `hook` is on: {name: replacement}."""
    return {} if hook is None else {n: _RoundedOps(getattr(R, n), hook) for n in ("F", "torch") if hasattr(R, n)}


def oracle_probes(kw, sd, sample, t, enc, mask_t, round_operand=None):
    """Named intermediates of the oracle, keyed like the engine's probes (channels-last), in schedule order.  round_operand: a hook
    applied to both operands of every F.linear / F.conv1d / attention product of the forward, the einsum pair of the pooled text
    embedding excepted (one_plane: a whole-forward emulation
    of the bf16 fast mode); None (the default) leaves the oracle as it is."""
    from conftest import oracle_cfg
    from oracle import unet_ref as R
    out = {}
    swapped = {n: getattr(R, n) for n in _hooked(R, round_operand)}
    for n, v in _hooked(R, round_operand).items():
        setattr(R, n, v)
    F = R.F
    orig = {n: getattr(R, n) for n in ("resnet_block", "transformer_1d", "downsample", "upsample", "transformer_block",
                                       "attention")}

    def tap(name, v):
        out[name] = v.permute(0, 2, 1).contiguous() if v.dim() == 3 else v

    def resnet_block(sdd, p, cfg, x, emb):
        g, eps = cfg["norm_num_groups"], cfg["norm_eps"]
        h = F.conv1d(F.silu(F.group_norm(x, g, sdd[p + "norm1.weight"], sdd[p + "norm1.bias"], eps)),
                     sdd[p + "conv1.weight"], sdd[p + "conv1.bias"], padding=1)
        tap(p + "conv1", h)
        y = orig["resnet_block"](sdd, p, cfg, x, emb)
        tap(p[:-1], y)
        return y

    def transformer_1d(sdd, p, cfg, x, e, b):
        h = F.group_norm(x, cfg["norm_num_groups"], sdd[p + "norm.weight"], sdd[p + "norm.bias"], 1e-6)
        h = F.conv1d(h, sdd[p + "proj_in.weight"], sdd[p + "proj_in.bias"])
        tap(p + "proj_in", h)
        y = orig["transformer_1d"](sdd, p, cfg, x, e, b)
        tap(p[:-1], y)
        return y

    def transformer_block(sdd, p, heads, x, e, b):
        C = x.shape[-1]
        n = F.layer_norm(x, (C,), sdd[p + "norm1.weight"], sdd[p + "norm1.bias"], 1e-5)
        x1 = orig["attention"](sdd, p + "attn1.", heads, n) + x
        out[p + "attn1"] = x1
        n = F.layer_norm(x1, (C,), sdd[p + "norm2.weight"], sdd[p + "norm2.bias"], 1e-5)
        x2 = orig["attention"](sdd, p + "attn2.", heads, n, e, b) + x1
        out[p + "attn2"] = x2
        y = orig["transformer_block"](sdd, p, heads, x, e, b)
        out[p + "ff"] = y
        return y

    def downsample(sdd, p, x):
        y = orig["downsample"](sdd, p, x)
        tap(p[:-1], y)
        return y

    def upsample(sdd, p, x, size=None):
        y = orig["upsample"](sdd, p, x, size)
        tap(p[:-1], y)
        return y

    R.resnet_block, R.transformer_1d, R.transformer_block, R.downsample, R.upsample = (
        resnet_block, transformer_1d, transformer_block, downsample, upsample)
    try:
        pr = {}
        y = R.unet_forward(sd, oracle_cfg(kw), sample, t, enc, mask_t, probes=pr)
    finally:
        for n, f in list(orig.items()) + list(swapped.items()):
            setattr(R, n, f)
    out["emb"] = pr["emb"][:, None, :]
    tap("conv_in", pr["conv_in"])
    return y, out


def prompt_probe_names(n_layers):
    """Names of the prompt encoder's intermediates (dv_penc_probe, include/dvits_hip.h), in schedule order."""
    names = ["pre"]
    for i in range(n_layers):
        names += ["layer%d.attn" % i, "layer%d.ffn1" % i, "layer%d" % i]
    return names + ["out_proj"]


def prompt_oracle_probes(sd, prompt, lengths, n_layers, num_heads=8, round_operand=None):
    """oracle.prompt_ref.prompt_encoder with its named intermediates, keyed like the engine's probes: (y [B, L, C_out], dict of
    [B, L, C]).  `pre` and `layerN` are the oracle's own probes; `layerN.attn` (after self-attention + residual + mask),
    `layerN.ffn1` (relu(k^-1/2 x the nine taps' sum), 4H wide, padding frames NOT masked) and `out_proj` (the masked out_proj
    ConvLayer, before the last LayerNorm) are taken by wrapping enc_sa_layer / ffn / conv_layer, which the oracle calls through
    its module globals; the wrappers call the original functions for what they return, so the oracle computes what it always
    computes.  round_operand: oracle_probes' hook, here on every F.linear and torch.matmul (the k = 1 ConvTBC and both attention
    products: q d^-1/2, k, the normalised probabilities and v are each rounded)."""
    from oracle import prompt_ref as R
    out = {}
    swapped = {n: getattr(R, n) for n in _hooked(R, round_operand)}
    for n, v in _hooked(R, round_operand).items():
        setattr(R, n, v)
    F = R.F
    orig = {n: getattr(R, n) for n in ("enc_sa_layer", "ffn", "conv_layer")}
    keep = R.sequence_mask(lengths, prompt.shape[2]).to(prompt.dtype)[:, :, None]      # [B, L, 1]

    def index(p):
        return int(p.split("layers.")[1].split(".")[0])

    def bt(v):                                                  # [L, B, C] -> [B, L, C]
        return v.permute(1, 0, 2).contiguous()

    def enc_sa_layer(sdd, p, x, pad_mask, num_heads=8, kernel_size=9):
        n = F.layer_norm(x, (x.shape[-1],), sdd[p + "layer_norm1.weight"], sdd[p + "layer_norm1.bias"], 1e-5)
        x2 = (x + R.self_attention(sdd, p + "self_attn.", n, pad_mask, num_heads)) * keep.transpose(0, 1)
        out["layer%d.attn" % index(p)] = bt(x2)
        return orig["enc_sa_layer"](sdd, p, x, pad_mask, num_heads, kernel_size)

    def ffn(sdd, p, x, kernel_size=9):
        T = x.shape[0]
        first = (kernel_size - 1) // 2
        padded = F.pad(x, (0, 0, 0, 0, first, kernel_size - 1 - first))
        res = 0
        for i in range(kernel_size):
            res = res + F.linear(padded[i:T + i] if i else x, sdd[p + "ffn_1.%d.weight" % i], sdd[p + "ffn_1.0.bias"] if i == 0 else None)
        out["layer%d.ffn1" % index(p)] = bt(F.relu(res * kernel_size ** -0.5))
        return orig["ffn"](sdd, p, x, kernel_size)

    def conv_layer(sdd, p, x, pad_mask=None):
        y = orig["conv_layer"](sdd, p, x, pad_mask)
        if p.endswith("out_proj."):
            out["out_proj"] = bt(y) * keep
        return y

    R.enc_sa_layer, R.ffn, R.conv_layer = enc_sa_layer, ffn, conv_layer
    try:
        pr = {}
        y = R.prompt_encoder(sd, prompt, lengths, n_layers, num_heads, probes=pr)
    finally:
        for n, f in list(orig.items()) + list(swapped.items()):
            setattr(R, n, f)
    out.update(pr)
    names = prompt_probe_names(n_layers)
    assert set(names) == set(out), set(names) ^ set(out)
    return y.permute(0, 2, 1).contiguous(), {n: out[n] for n in names}


# ---- the one-launch feed-forward in isolation (tests/test_gpu_tapped_schedule.py, tests/test_ff_tail_reference.py) --------------
FF_TAIL_BOUND = 1e-4        # whole tensor and every frame: test_conv3's bound for the same split-bf16 contraction


def ff_tail_fp64(sd, p, h3, x, drop_ff=False, swap_geglu=False, emulate=False, fault=None):
    """What k_chain_ff / k_ff_split compute for the Transformer2DModel with prefix `p` ("....attentions.0."), restated in fp64 from
    the UNMERGED state-dict weights:  proj_out(h3 + ff.net.2(GEGLU(ff.net.0(LN3(h3))))) + x,  h3 = the block after its cross
    attention, x = the transformer's input, both channels-last [B, T, C].  `drop_ff` / `swap_geglu` plant a fault (the
    feed-forward term left out; the value and gate halves of GEGLU exchanged) for the tests that show the bound has teeth;
    `emulate` / `fault` are ln_linear's (below)."""
    import torch.nn.functional as F
    tb = p + "transformer_blocks.0."
    W = lambda n: sd[n].detach().cpu().to(torch.float64)    # noqa: E731
    h3, x = torch.as_tensor(h3).to(torch.float64), torch.as_tensor(x).to(torch.float64)
    C = h3.shape[-1]
    hg = ln_linear(h3, W(tb + "norm3.weight"), W(tb + "norm3.bias"), W(tb + "ff.net.0.proj.weight"), W(tb + "ff.net.0.proj.bias"),
                   emulate, fault)
    a, gate = hg.chunk(2, dim=-1)
    if swap_geglu:
        a, gate = gate, a
    ff = _linear(a * F.gelu(gate), W(tb + "ff.net.2.weight"), W(tb + "ff.net.2.bias"), emulate)
    h4 = h3 if drop_ff else h3 + ff
    return _linear(h4, W(p + "proj_out.weight")[:, :, 0], W(p + "proj_out.bias"), emulate) + x


def seam_figures(per_frame, rows):
    """Worst per-frame error of a [B, T] array, reported apart as test_conv3 does: the first frame, the last frame, the frames at
    the seams of `rows`-high row blocks (multiples of `rows` and the frames just before them), every other frame."""
    T = per_frame.shape[1]
    seams = sorted({t for t in range(T) if t % rows in (0, rows - 1)} - {0, T - 1})
    inner = sorted(set(range(T)) - set(seams) - {0, T - 1})
    return {"first": float(per_frame[:, 0].max()), "last": float(per_frame[:, T - 1].max()),
            "seams": float(per_frame[:, seams].max()) if seams else 0.0, "inner": float(per_frame[:, inner].max()) if inner else 0.0}


# ---- the folded-normalisation launches in isolation (tests/test_gpu_offdist.py, tests/test_offdist_reference.py) ----------------
# Each restatement below computes one stretch of the schedule between two taps in fp64 from the UNMERGED state-dict weights.  With
# emulate=True it does the arithmetic the kernels are documented to do instead (csrc/kernels_qkv.hip, kernels_chain.hip,
# kernels_ffsplit.hip, gnx_device.h): every contraction operand held as two bf16 planes (hi = bf16(v), lo = bf16(v - hi)), the
# products summed exactly (fp64 here); a LayerNorm folded into its consumer - gamma and beta in the packed weights, the RAW row in
# the planes, mean and rstd (from the fp32 row) applied afterwards as  rstd (x W' - mean u) + b' ; a GroupNorm as one affine
# a x + b per (utterance, channel), applied before the planes are stored; the attention logits in fp32, exp(s - max) rounded to
# ONE fp16 plane before P V (tests/test_gpu_ops.py test_attention_frag).  The emulation is what sets the per-frame bound of the
# GPU test (isolated_bound): it carries the cancellation of  x W' - mean u  at a large row mean that a fixed bound would have to
# guess.  `fault` plants what a kernel could get wrong only in this regime (FAULTS).
#
# emulate="bf16" is the fast mode (precision="bf16": the plain schedule, DESIGN.md "Precision"): every contraction operand ONE bf16
# plane - the raw LayerNorm row, the gamma-folded weight W gamma (folded first, then rounded, as the packer does), the GroupNorm
# affine's result, q, k, v; q is multiplied by fp32(d^-1/2 log2 e) BEFORE it is rounded (attn_tile.h keeps the scores in the log2
# domain and scales the query, not the logit), the logits and the mask are added in fp32, and exp2(s - max) is rounded to ONE bf16
# plane before P V while the denominator sums the unrounded values.  Two faults belong to this mode: "mask_tail" - the mask bias
# left off the keys of the last 32-key sub-tile; "p_fp16" - P rounded to fp16 where bf16 is documented.
FAULTS = ("lost_lo", "mean_from_bf16", "beta_sign", "tscale", "skip_stats")
BF16_FAULTS = ("mean_from_bf16", "beta_sign", "tscale", "skip_stats", "mask_tail", "p_fp16")
BF16_FLOOR = 2.0 ** -9      # half an ulp of an 8-bit significand: what one bf16 plane can hold of an operand at all
LOG2E = 1.44269504088896340736


def _planes(v, lo=True):
    """What two bf16 planes hold of the fp32 tensor v, as fp64 (lo=False: the hi plane alone)."""
    v32 = torch.as_tensor(v).to(torch.float32)
    hi = v32.to(torch.bfloat16).float()
    if not lo:
        return hi.double()
    return hi.double() + (v32 - hi).to(torch.bfloat16).double()


def _operand(v, emulate):
    """What a contraction holds of the operand v: v itself, its two bf16 planes (emulate=True), its hi plane alone ("bf16")."""
    return _planes(v, lo=emulate != "bf16") if emulate else v


def _linear(x, W, b, emulate):
    import torch.nn.functional as F
    return F.linear(_operand(x, emulate), _operand(W, emulate), b)


def ln_linear(x, gamma, beta, W, b, emulate=False, fault=None, eps=1e-5, stats=None, acc32=False):
    """linear(LayerNorm(x) gamma + beta; W, b) in fp64, or (emulate / fault) in the folded form described above.  Faults:
    "lost_lo" - the raw row enters the contraction as its hi plane alone; "mean_from_bf16" - the row mean is taken from the
    bf16-rounded row, not from the fp32 row; "beta_sign" - beta folded into b' with the wrong sign.
    stats = (mean, rstd) per row: the folded form finishes with THESE (what the consumer combined from the producer's fp32
    partials: tests/norm_cases.py) instead of the fp64 statistics of the row.  acc32: u, b' and the contraction are rounded to
    float32 and the finish rstd * (acc - mean * u) + b' runs in float32, as the epilogue does."""
    import torch.nn.functional as F
    x = torch.as_tensor(x).double()
    if not emulate and stats is None and fault not in ("lost_lo", "mean_from_bf16", "beta_sign"):
        return F.linear(F.layer_norm(x, (x.shape[-1],), gamma, beta, eps), W, b)
    x32 = x.float().double()
    mean = x32.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x32 - mean) ** 2).mean(-1, keepdim=True) + eps)
    if stats is not None:
        mean, rstd = (torch.as_tensor(s).double().reshape(-1, 1) for s in stats)
    if fault == "mean_from_bf16":
        mean = _planes(x, lo=False).mean(-1, keepdim=True)
    Wf = _planes(W * gamma[None, :], lo=emulate != "bf16")
    bf = (-1.0 if fault == "beta_sign" else 1.0) * (W @ beta) + (0.0 if b is None else b)
    xp = _planes(x, lo=fault != "lost_lo" and emulate != "bf16")
    assert not (acc32 and emulate == "bf16")
    if acc32:    # the three products of the split-bf16 contraction (hi hi + hi lo + lo hi; lo lo is never formed), float32 accumulation
        u32, b32 = (W * gamma[None, :]).sum(-1).float(), bf.float()
        xh, wh = _planes(x, lo=False).float(), _planes(W * gamma[None, :], lo=False).float()
        xl, wl = (xp.float() - xh) if fault != "lost_lo" else torch.zeros_like(xh), Wf.float() - wh
        acc = xh @ wh.t() + xh @ wl.t() + xl @ wh.t()
        return (rstd.float() * (acc - mean.float() * u32) + b32).double()
    return rstd * (xp @ Wf.t() - mean * Wf.sum(-1)) + bf


def _sdpa(q, k, v, heads, bias, emulate, fault=None):
    import math
    B, Tq, C = q.shape
    d = C // heads
    q, k, v = (a.reshape(B, -1, heads, d).transpose(1, 2) for a in (q, k, v))
    if fault == "mask_tail" and bias is not None:
        Tk = k.shape[-2]
        bias = bias.clone()
        bias[..., (Tk - 1) // 32 * 32:] = 0.0
    if emulate == "bf16":
        qs = torch.tensor(1.0 / math.sqrt(d), dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
        s = (_planes(q.float() * qs, lo=False) @ _planes(k, lo=False).transpose(-1, -2)).float()
        if bias is not None:
            s = s + (bias.float() * torch.tensor(LOG2E, dtype=torch.float32))[:, None]
        s = s.double()
        pr = torch.exp2(s - s.amax(-1, keepdim=True))
        p1 = pr.half().double() if fault == "p_fp16" else pr.float().to(torch.bfloat16).double()
        o = (p1 @ _planes(v, lo=False)) / pr.sum(-1, keepdim=True)
        return o.transpose(1, 2).reshape(B, Tq, C)
    s = q @ k.transpose(-1, -2) / math.sqrt(d)
    if emulate:
        s = s.float() if bias is None else s.float() + bias.float()[:, None]
        s = s.double()
    elif bias is not None:
        s = s + bias[:, None]
    pr = torch.exp(s - s.amax(-1, keepdim=True))
    o = ((pr.half().double() if emulate else pr) @ v) / pr.sum(-1, keepdim=True)
    return o.transpose(1, 2).reshape(B, Tq, C)


def sdpa_fp64(q, k, v, heads, bias=None, emulate=False, fault=None):
    """softmax(q k^T d^-1/2 + bias) v on [B, T, heads d] tensors, bias additive [B, Tk] or None, in fp64 - or as the documented
    arithmetic does it (emulate / fault: above)."""
    q, k, v = (torch.as_tensor(a).double() for a in (q, k, v))
    return _sdpa(q, k, v, heads, None if bias is None else torch.as_tensor(bias).double()[:, None, :], emulate, fault)


def attn_chain_fp64(sd, tb, which, x, heads, enc=None, mask=None, emulate=False, fault=None):
    """`which` = "attn1": norm1 -> self attention -> to_out + x (x = the tapped proj_in, result = the tapped attn1);
    "attn2": norm2 -> cross attention over enc [B, L, D] under the boolean mask [B, L] -> to_out + x (attn1 -> attn2).
    tb = "....transformer_blocks.0."."""
    import torch.nn.functional as F
    W = lambda n: sd[n].detach().cpu().to(torch.float64)    # noqa: E731
    x = torch.as_tensor(x).double()
    g, b, a = W(tb + "norm%s.weight" % which[-1]), W(tb + "norm%s.bias" % which[-1]), tb + which + "."
    q = ln_linear(x, g, b, W(a + "to_q.weight"), None, emulate, fault)
    if enc is None:
        k, v, bias = ln_linear(x, g, b, W(a + "to_k.weight"), None, emulate, fault), ln_linear(x, g, b, W(a + "to_v.weight"), None, emulate, fault), None
    else:
        e = torch.as_tensor(enc).double()
        k, v = _linear(e, W(a + "to_k.weight"), None, emulate), _linear(e, W(a + "to_v.weight"), None, emulate)
        bias = None if mask is None else ((1.0 - torch.as_tensor(mask).double()) * -10000.0)[:, None, :]
    o = _sdpa(q, k, v, heads, bias, emulate, fault)
    return _linear(o, W(a + "to_out.0.weight"), W(a + "to_out.0.bias"), emulate) + x


def _group_affine(x, groups, gamma, beta, eps, stats_from=None):
    """GroupNorm of channels-last x [B, T, C] as the per-(utterance, channel) affine (a, b): y = a x + b.  stats_from: a [C] index
    array - channel c takes the statistics of the group of channel stats_from[c] (a planted fault)."""
    B, T, C = x.shape
    xg = x.reshape(B, T, groups, C // groups)
    mean = xg.mean((1, 3))
    rstd = 1.0 / torch.sqrt(((xg - mean[:, None, :, None]) ** 2).mean((1, 3)) + eps)
    idx = torch.arange(C) if stats_from is None else torch.as_tensor(stats_from)
    grp = idx // (C // groups)
    a = rstd[:, grp] * gamma[None, :]
    return a[:, None, :], (beta[None, :] - mean[:, grp] * a)[:, None, :]


def _conv(h, W, b, emulate, stride=1):
    import torch.nn.functional as F
    return F.conv1d(_operand(h, emulate).permute(0, 2, 1), _operand(W, emulate), b, stride=stride,
                    padding=W.shape[-1] // 2).permute(0, 2, 1)


def proj_in_fp64(sd, p, x, groups, emulate=False):
    """The first stretch of the block head: GroupNorm (eps 1e-6) -> proj_in, x = the transformer's input (the tapped resnet block),
    result = the tapped proj_in.  p = "....attentions.i."."""
    W = lambda n: sd[n].detach().cpu().to(torch.float64)    # noqa: E731
    x = torch.as_tensor(x).double()
    a, b = _group_affine(x, groups, W(p + "norm.weight"), W(p + "norm.bias"), 1e-6)
    return _conv(a * x + b, W(p + "proj_in.weight"), W(p + "proj_in.bias"), emulate)


def resnet_fp64(sd, p, x, emb, groups, skip=None, eps=1e-5, emulate=False, fault=None):
    """A ResnetBlock2D from its input tap to its output tap: norm1 + SiLU -> conv1 -> norm2 (1 + scale) + shift + SiLU -> conv2 +
    shortcut.  x [B, T, C] channels-last, emb [B, 1, E] or [B, E] (the tapped `emb`), skip: the second half of an up-path block's
    concatenated input.  Faults: "tscale" - 1 + scale replaced by scale; "skip_stats" - the skip half's channels take the group
    statistics of the h half's channels at the same offset (the concatenated GroupNorm indexed without the skip's channel base)."""
    import torch.nn.functional as F
    W = lambda n: sd[n].detach().cpu().to(torch.float64)    # noqa: E731
    x = torch.as_tensor(x).double()
    C1 = x.shape[-1]
    if skip is not None:
        x = torch.cat([x, torch.as_tensor(skip).double()], -1)
    C = x.shape[-1]
    stats_from = None
    if fault == "skip_stats":
        assert skip is not None
        stats_from = torch.cat([torch.arange(C1), torch.arange(C - C1)])
    a, b = _group_affine(x, groups, W(p + "norm1.weight"), W(p + "norm1.bias"), eps, stats_from)
    h = _conv(F.silu(a * x + b), W(p + "conv1.weight"), W(p + "conv1.bias"), emulate)
    t = F.linear(F.silu(torch.as_tensor(emb).double().reshape(x.shape[0], -1)), W(p + "time_emb_proj.weight"), W(p + "time_emb_proj.bias"))
    scale, shift = t.chunk(2, -1)
    a, b = _group_affine(h, groups, W(p + "norm2.weight"), W(p + "norm2.bias"), eps)
    m = (scale if fault == "tscale" else 1.0 + scale)[:, None, :]
    h = _conv(F.silu((a * m) * h + (b * m + shift[:, None, :])), W(p + "conv2.weight"), W(p + "conv2.bias"), emulate)
    if (p + "conv_shortcut.weight") in sd:
        x = _conv(x, W(p + "conv_shortcut.weight"), W(p + "conv_shortcut.bias"), emulate)
    return x + h


def isolated_bound(emulated, want, mode=None):
    """Bound for one launch (or one stretch between taps) in isolation, whole tensor and every frame: FF_TAIL_BOUND, or - where the
    inputs make the documented arithmetic itself cost more - 2 x the worst frame of its host emulation + 2^-16 (the factor 2 and
    the 2^-16 as tests/test_gpu_ops.py test_attention_frag argues them).  mode="bf16": the same form for the one-plane fast mode,
    2 x the worst frame of the emulate="bf16" restatement + 2^-9 (BF16_FLOOR: with a single valid key the emulation is exact);
    FF_TAIL_BOUND is a parity-mode figure and does not enter."""
    if mode == "bf16":
        return 2.0 * frame_errors(emulated, want)["worst"] + BF16_FLOOR
    assert mode is None, mode
    return max(FF_TAIL_BOUND, 2.0 * frame_errors(emulated, want)["worst"] + 2.0 ** -16)


def conv_in_fp64(sd, sample, emulate=False):
    """conv_in: sample [B, T, Cin] channels-last -> the tapped conv_in."""
    W = lambda n: sd[n].detach().cpu().to(torch.float64)    # noqa: E731
    return _conv(torch.as_tensor(sample).double(), W("conv_in.weight"), W("conv_in.bias"), emulate)


def resample_fp64(sd, p, x, size=None, emulate=False):
    """Downsample2D (p = "....downsamplers.0.": Conv1d k 3, stride 2, padding 1) or Upsample2D (p = "....upsamplers.0.": nearest to
    `size` frames - twice the input's when None - then Conv1d k 3, padding 1), x channels-last = the tapped input."""
    import torch.nn.functional as F
    W = lambda n: sd[n].detach().cpu().to(torch.float64)    # noqa: E731
    x = torch.as_tensor(x).double()
    if "downsamplers" in p:
        return _conv(x, W(p + "conv.weight"), W(p + "conv.bias"), emulate, stride=2)
    x = F.interpolate(x.permute(0, 2, 1), size=2 * x.shape[1] if size is None else size, mode="nearest").permute(0, 2, 1)
    return _conv(x, W(p + "conv.weight"), W(p + "conv.bias"), emulate)


def conv_out_fp64(sd, x, groups, eps=1e-5, emulate=False):
    """conv_norm_out -> SiLU -> conv_out: x = the tapped last transformer (up_blocks.3.attentions.2), result = the output y, channels-last."""
    import torch.nn.functional as F
    W = lambda n: sd[n].detach().cpu().to(torch.float64)    # noqa: E731
    x = torch.as_tensor(x).double()
    a, b = _group_affine(x, groups, W("conv_norm_out.weight"), W("conv_norm_out.bias"), eps)
    return _conv(F.silu(a * x + b), W("conv_out.weight"), W("conv_out.bias"), emulate)


def resnet_input_taps(n_levels=4, layers=2):
    """{resnet block name: (tap of its input, tap of the concatenated skip or None)} for the layout of oracle.unet_ref.unet_forward:
    down = (CrossAttn x (n - 1), Down), mid, up = (Up, CrossAttn x (n - 1))."""
    out, skips, h = {}, ["conv_in"], "conv_in"
    for i in range(n_levels):
        for j in range(layers):
            out["down_blocks.%d.resnets.%d" % (i, j)] = (h, None)
            h = "down_blocks.%d.%s.%d" % (i, "attentions" if i < n_levels - 1 else "resnets", j)
            skips.append(h)
        if i < n_levels - 1:
            h = "down_blocks.%d.downsamplers.0" % i
            skips.append(h)
    out["mid_block.resnets.0"] = (h, None)
    out["mid_block.resnets.1"] = ("mid_block.attentions.0", None)
    h = "mid_block.resnets.1"
    for i in range(n_levels):
        for j in range(layers + 1):
            out["up_blocks.%d.resnets.%d" % (i, j)] = (h, skips.pop())
            h = "up_blocks.%d.%s.%d" % (i, "attentions" if i > 0 else "resnets", j)
        if i < n_levels - 1:
            h = "up_blocks.%d.upsamplers.0" % i
    assert not skips
    return out
