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


def block_errors(got, want, rows, cols):
    """Relative L2 per rows x cols block of [B, T, C] tensors; the row blocks are laid out per utterance from its first frame (as
    the kernels' row tiles are), the last block of an utterance / of the channels may be short.  Denominators are floored like
    frame_errors'.  Returns a dict: worst, utterance, rows (r0, r1), cols (c0, c1) - half-open ranges of the worst block."""
    g, w = _f64(got), _f64(want)
    assert g.shape == w.shape and g.ndim == 3, (g.shape, w.shape)
    B, T, C = w.shape
    rows, cols = min(rows, T), min(cols, C)
    nr, nc = -(-T // rows), -(-C // cols)
    pad = ((0, 0), (0, nr * rows - T), (0, nc * cols - C))
    d2 = np.pad((g - w) ** 2, pad).reshape(B, nr, rows, nc, cols).sum((2, 4))
    w2 = np.pad(w * w, pad).reshape(B, nr, rows, nc, cols).sum((2, 4))
    floor2 = FLOOR_FRACTION ** 2 * w2.mean()
    per = np.sqrt(d2 / np.maximum(np.maximum(w2, floor2), 1e-300))
    b, r, c = (int(v) for v in np.unravel_index(int(np.argmax(per)), per.shape))
    return {"worst": float(per[b, r, c]), "utterance": b, "rows": (r * rows, min((r + 1) * rows, T)),
            "cols": (c * cols, min((c + 1) * cols, C))}


def localisation(got, want):
    """Worst-frame error / whole-tensor error.  Rounding noise spread over the tensor gives a small ratio (the tail of a
    distribution over the frames); a fault confined to a few frames gives a large one."""
    fe = frame_errors(got, want)
    return fe["worst"] / max(fe["rel_l2"], 1e-300)


TILE_GEOMETRIES = ((32, 1 << 30), (64, 64), (128, 128))   # 32 rows x all channels (row-block chains), conv / split tiles, GEMM tiles


def describe(name, got, want):
    """One line that says where `got` is furthest from `want`: worst frame, worst block of each tile geometry, whole tensor."""
    fe = frame_errors(got, want)
    parts = ["%s: tensor %.2e, worst frame %.2e at utterance %d frame %d (x%.1f)" %
             (name, fe["rel_l2"], fe["worst"], fe["at"][0], fe["at"][1], fe["worst"] / max(fe["rel_l2"], 1e-300))]
    for rows, cols in TILE_GEOMETRIES:
        be = block_errors(got, want, rows, cols)
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


def oracle_probes(kw, sd, sample, t, enc, mask_t):
    """Named intermediates of the oracle, keyed like the engine's probes (channels-last), in schedule order."""
    import torch.nn.functional as F
    from conftest import oracle_cfg
    from oracle import unet_ref as R
    out = {}
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
        for n, f in orig.items():
            setattr(R, n, f)
    out["emb"] = pr["emb"][:, None, :]
    tap("conv_in", pr["conv_in"])
    return y, out
