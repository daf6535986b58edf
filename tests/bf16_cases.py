"""The cases of the bf16 fast-mode parity tests (tests/test_bf16_reference.py on the CPU, tests/test_gpu_bf16_mode.py on the GPU):
the attention shapes that reach every k_attention<DP, NW, 1> instantiation, the three denoiser shapes with their inputs, and the
list of stretches between two taps with their fp64 / one-plane restatements (tests/parity_metrics.py).  Plain helper module: no
fixtures, no hooks."""
import numpy as np
import torch

from conftest import UNET_CASES
from parity_metrics import (attn_chain_fp64, conv_in_fp64, conv_out_fp64, ff_tail_fp64, proj_in_fp64, resample_fp64, resnet_fp64,
                            resnet_input_taps)

KW = UNET_CASES["cfg1"][0]
# (B, T, L): levels 100 / 50 / 25 / 13 in padded row spaces; levels with fewer rows than one tile; whole tiles
SHAPES = [(2, 100, 20), (1, 37, 20), (3, 64, 33)]
XF_BLOCKS = ([(i, "down_blocks.%d.attentions.%d." % (i, j)) for i in range(3) for j in range(2)] + [(3, "mid_block.attentions.0.")] +
             [(3 - i, "up_blocks.%d.attentions.%d." % (i, j)) for i in range(1, 4) for j in range(3)])


# ---------------------------------------------------------------------------------------------------------------- attention
def plain_instantiation(B, H, Tq, Tk, d):
    """(DP, NW) of the k_attention<DP, NW, NSPLIT> launch_attention picks (csrc/kernels_attn.hip): the head width padded to a
    multiple of 16; 8 waves per workgroup from 1100 (utterance, head, 32-query block) jobs, 4 from 64, 2 from 16, else 1."""
    waves = B * H * -(-Tq // 32)
    return -(-d // 16) * 16, 8 if waves >= 1100 else (4 if waves >= 64 else (2 if waves >= 16 else 1))


# (B, H, Tq, Tk, d, mask, logit scale); the mask kinds are those of ATTN_FRAG_SHAPES (tests/test_gpu_ops.py)
ATTN_PLAIN_SHAPES = [
    (1, 1, 1, 1, 4, None, 1), (1, 8, 31, 31, 16, "ragged", 1), (1, 2, 33, 32, 32, None, 1), (1, 4, 33, 97, 48, "all", 1),
    (1, 8, 1, 161, 64, "one", 8),                                                                       # 1 wave
    (2, 8, 31, 33, 8, "ragged", 1), (2, 8, 33, 64, 12, "tile", 1), (1, 8, 96, 65, 32, "ragged", 8), (2, 4, 100, 97, 48, "one", 1),
    (1, 8, 64, 161, 64, None, 1),                                                                       # 2 waves
    (2, 8, 300, 33, 16, "all", 1), (2, 8, 300, 161, 24, "tile", 1), (2, 8, 300, 65, 48, None, 1), (2, 8, 128, 1, 64, None, 1),  # 4 waves
    (2, 8, 2240, 97, 16, "ragged", 1), (2, 8, 2240, 31, 32, "one", 1), (2, 8, 2240, 64, 40, None, 1), (2, 8, 2240, 161, 64, "ragged", 8),  # 8 waves
]


def attention_case(B, H, Tq, Tk, d, mask, qs):
    """q [B, Tq, H d] x the logit scale, k, v [B, Tk, H d], each rounded to bf16 first (so one plane holds k and v exactly), and the
    additive key bias [B, Tk] or None, as numpy float32."""
    from diff_vits_amd import synth

    def bf16(a):
        return torch.from_numpy(a).to(torch.bfloat16).float().numpy()
    q = bf16(synth.normal(99, "q", (B, Tq, H * d)) * np.float32(qs))
    k, v = bf16(synth.normal(99, "k", (B, Tk, H * d))), bf16(synth.normal(99, "v", (B, Tk, H * d)))
    bias = None
    if mask is not None:
        bias = np.zeros((B, Tk), dtype=np.float32)
        for b in range(B):
            if mask == "ragged":
                bias[b, max(1, Tk - 7 * (b + 1)):] = -10000.0
            elif mask == "one":
                bias[b] = -10000.0
                bias[b, (5 * b + 3) % Tk] = 0.0
            elif mask == "all":
                bias[b, (0 if b == 0 else max(1, Tk - 9)):] = -10000.0
            elif mask == "tile":
                bias[b, max(1, (Tk - 1) // 32 * 32 - 32 * b):] = -10000.0
    return q, k, v, bias


# ---------------------------------------------------------------------------------------------------------------- the denoiser
def state_dict():
    from diff_vits_amd import synth
    from diff_vits_amd.unet1d.unet_1d_condition import UNet1DConditionModel
    with torch.device("meta"):
        shapes = {k: tuple(v.shape) for k, v in UNet1DConditionModel(**KW).state_dict().items()}
    return {k: torch.from_numpy(v) for k, v in synth.make_state_dict(shapes, seed=1234).items()}


def inputs(B, T, L):
    """sample [B, 208, T], t [B], enc [B, L, 128], the ragged prompt mask [B, L] (mask[b, max(1, L - 7 b):] = False)."""
    from diff_vits_amd import synth
    cx = KW["out_channels"]
    x = torch.from_numpy(synth.normal(61, "x", (B, cx, T)))
    cond = torch.from_numpy(synth.normal(61, "c", (B, KW["in_channels"] - cx, T)))
    enc = torch.from_numpy(synth.normal(61, "e", (B, L, KW["cross_attention_dim"])))
    mask = torch.ones(B, L, dtype=torch.bool)
    for b in range(B):
        mask[b, max(1, L - 7 * b):] = False
    t = torch.tensor([949.05 - 51.5 * b for b in range(B)])
    return torch.cat([x, cond], 1), t, enc, mask


def levels(T, n=4):
    out = [T]
    for _ in range(n - 1):
        out.append((out[-1] - 1) // 2 + 1)
    return out


def stretches(sd, taps, sample, enc, mask, y, T):
    """Every stretch of the schedule between two taps that parity_metrics restates: a list of (name, kind, output tensor
    [B, T', C], fn) with fn(emulate, fault=None) -> the restatement evaluated on `taps`' own inputs.  taps: {probe name: [B, T', C]}
    (the engine's, or the oracle's); sample [B, Cin, T], y [B, Cout, T] channels-first."""
    heads, groups = KW["attention_head_dim"], KW["norm_num_groups"]
    Ts = levels(T)
    cl = lambda v: torch.as_tensor(v).permute(0, 2, 1).contiguous()    # noqa: E731
    out = [("conv_in", "conv", taps["conv_in"], lambda e, fault=None: conv_in_fp64(sd, cl(sample), emulate=e))]
    res_in = resnet_input_taps()
    for name, (xin, skip) in res_in.items():
        out.append((name, "resnet" + ("+skip" if skip else ""), taps[name],
                    lambda e, fault=None, name=name, xin=xin, skip=skip: resnet_fp64(
                        sd, name + ".", taps[xin], taps["emb"], groups, skip=None if skip is None else taps[skip], emulate=e, fault=fault)))
    for _, p in XF_BLOCKS:
        tb = p + "transformer_blocks.0."
        x = taps[p.replace("attentions", "resnets")[:-1]]
        h, h1, h3 = taps[p + "proj_in"], taps[tb + "attn1"], taps[tb + "attn2"]
        out.append((p + "proj_in", "GN+proj", h, lambda e, fault=None, p=p, x=x: proj_in_fp64(sd, p, x, groups, emulate=e)))
        out.append((tb + "attn1", "attn1", h1, lambda e, fault=None, tb=tb, h=h: attn_chain_fp64(sd, tb, "attn1", h, heads, emulate=e, fault=fault)))
        out.append((tb + "attn2", "attn2", h3, lambda e, fault=None, tb=tb, h1=h1: attn_chain_fp64(sd, tb, "attn2", h1, heads, enc, mask,
                                                                                                   emulate=e, fault=fault)))
        out.append((p[:-1], "ff", taps[p[:-1]], lambda e, fault=None, p=p, h3=h3, x=x: ff_tail_fp64(sd, p, h3, x, emulate=e, fault=fault)))
    for i in range(3):
        p = "down_blocks.%d.downsamplers.0." % i
        out.append((p[:-1], "down", taps[p[:-1]], lambda e, fault=None, p=p, i=i: resample_fp64(sd, p, taps["down_blocks.%d.attentions.1" % i],
                                                                                                emulate=e)))
        p = "up_blocks.%d.upsamplers.0." % i
        src = "up_blocks.0.resnets.2" if i == 0 else "up_blocks.%d.attentions.2" % i
        out.append((p[:-1], "up", taps[p[:-1]], lambda e, fault=None, p=p, src=src, i=i: resample_fp64(sd, p, taps[src], size=Ts[2 - i], emulate=e)))
    out.append(("conv_out", "GN+conv", cl(y), lambda e, fault=None: conv_out_fp64(sd, taps["up_blocks.3.attentions.2"], groups, emulate=e)))
    return out
