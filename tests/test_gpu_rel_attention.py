"""GPU: k_rel_attention alone (dv_op_rel_attention, csrc/kernels_relattn.hip) against the attention core of
oracle.text_enc_ref.rel_attention - what sits between the q / k / v projections and conv_o - restated here in fp64 torch.

Criteria on the valid rows (tests/parity_metrics.py): every frame < FRAME_BOUND = 1e-3 and whole-tensor relative L2 < 2e-4; rows of
an utterance behind its length are exactly zero.  Shapes: head dims 32 / 64 / 128 at window 4 and B = 3 with T = 1, 5 (every
offset of the window exists exactly once), 9, 31, 32, 33 (either side of the 32-key tile), 75 (ragged 75 / 40 / 9) and 300; windows
1 and 8 at T = 33; and T = 512, the longest the kernel accepts (the launcher refuses longer ones: checked without a launch).

The kernel's own edges (EDGE_CASES: d = 32 / 128, T = 33 / 75, window 4), each also under a per-row bound in the manner of
tests/test_gpu_ops.py test_attention_frag - 2 x the worst row of a host emulation of the documented arithmetic + 2^-16: a logit
gain of 4 and 8 on q; one dominant key (+12 in natural units through q and k) in the first or the last key tile, inside the band
of some queries and outside that of others; a common offset c u on every key (c = 0, 4, 16), which the softmax ignores and K Q^T pays for.
DVITS_PARITY_REPORT=<file> appends their figures (profiles/offdist_enc_parity.txt)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from parity_metrics import FRAME_BOUND, masked_frame_errors

pytestmark = pytest.mark.gpu

H = 2
LENGTHS = {1: [1, 1, 1], 5: [5, 3, 1], 9: [9, 8, 4], 31: [31, 17, 2], 32: [32, 31, 1], 33: [33, 32, 31], 75: [75, 40, 9],
           300: [300, 257, 33], 512: [512, 480, 65]}
CASES = [(d, T, 4) for d in (32, 64, 128) for T in (1, 5, 9, 31, 32, 33, 75, 300)] + [(128, 33, 1), (128, 33, 8), (128, 512, 4)]


def core_fp64(q, k, v, ek, ev, lengths, window):
    """q, k, v [B, T, H, d]; ek, ev [2w+1, d] -> [B, T, H*d], rows >= lengths[b] zero (oracle.text_enc_ref.rel_attention :28-48)."""
    q, k, v, ek, ev = (a.double() for a in (q, k, v, ek, ev))
    B, T, Hn, d = q.shape
    q, k, v = (a.permute(0, 2, 1, 3) for a in (q, k, v))
    q = q / math.sqrt(d)
    keep = (torch.arange(T)[None, :] < lengths[:, None]).double()
    attn_mask = (keep[:, :, None] * keep[:, None, :])[:, None]
    scores = q @ k.transpose(-2, -1)
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    off = j - i + window
    band = (off >= 0) & (off <= 2 * window)
    scores = scores + (q @ ek.t()).gather(-1, off.clamp(0, 2 * window).expand(B, Hn, T, T)) * band
    scores = scores.masked_fill(attn_mask == 0, -1e4)
    p = torch.softmax(scores, -1)
    out = p @ v
    jj = i + torch.arange(2 * window + 1)[None, :] - window
    valid = (jj >= 0) & (jj < T)
    out = out + (p.gather(-1, jj.clamp(0, T - 1).expand(B, Hn, T, 2 * window + 1)) * valid) @ ev
    return out.permute(0, 2, 1, 3).reshape(B, T, Hn * d) * keep[:, :, None]


def _tensors(d, T, window):
    from diff_vits_amd import synth
    tag = "ra.%d.%d.%d." % (d, T, window)
    q, k, v = (torch.from_numpy(synth.normal(1234, tag + n, (3, T, H, d))) for n in "qkv")
    ek, ev = (torch.from_numpy(synth.normal(1234, tag + n, (2 * window + 1, d), std=d ** -0.5)) for n in ("ek", "ev"))
    return q, k, v, ek, ev, torch.tensor(LENGTHS[T], dtype=torch.int64)


def _run(q, k, v, ek, ev, lengths, window):
    from diff_vits_amd import _lib
    B, T, Hn, d = q.shape
    dq, dk, dv, dek, dev, dl = (a.cuda().contiguous() for a in (q, k, v, ek, ev, lengths))
    o = torch.full((B, T, Hn * d), float("nan"), device="cuda")
    _lib.check(_lib.lib().dv_op_rel_attention(_lib.ptr(dq), _lib.ptr(dk), _lib.ptr(dv), _lib.ptr(dek), _lib.ptr(dev), _lib.ptr(dl),
                                              _lib.ptr(o), B, Hn, T, d, window, _lib.stream_ptr()), "dv_op_rel_attention")
    torch.cuda.synchronize()
    return o.cpu()


@pytest.mark.parametrize("d,T,window", CASES, ids=["d%d-T%d-w%d" % c for c in CASES])
def test_rel_attention_against_fp64_core(d, T, window):
    q, k, v, ek, ev, lengths = _tensors(d, T, window)
    want = core_fp64(q, k, v, ek, ev, lengths, window)
    got = _run(q, k, v, ek, ev, lengths, window)
    assert bool(torch.isfinite(got).all()), "rows the kernel did not write"
    fe = masked_frame_errors(got, want, lengths.tolist())
    print("d=%d T=%d w=%d: rel_l2 %.3e worst frame %.3e at %s" % (d, T, window, fe["rel_l2"], fe["worst"], fe["at"]))
    assert fe["padding_zero"], "row %s behind its utterance's length is not zero" % (fe["first_nonzero"],)
    assert fe["worst"] < FRAME_BOUND, (fe["worst"], fe["at"])
    assert fe["rel_l2"] < 2e-4, fe["rel_l2"]


def test_band_terms_matter_and_offsets_map_one_to_one():
    """T = 5, window 4: every offset -4 .. 4 exists exactly once per (first query, last query) pair.  With E_k or E_v zeroed the
    result moves by far more than the bound - the comparison above does exercise both band terms - and a reversed E_k table
    is told from the right one."""
    d, T, window = 128, 5, 4
    q, k, v, ek, ev, lengths = _tensors(d, T, window)
    lengths = torch.tensor([5, 5, 5])
    got = _run(q, k, v, ek, ev, lengths, window)
    for other in ((torch.zeros_like(ek), ev), (ek, torch.zeros_like(ev)), (ek.flip(0), ev), (ek, ev.flip(0))):
        wrong = core_fp64(q, k, v, other[0], other[1], lengths, window)
        assert masked_frame_errors(got, wrong, lengths.tolist())["worst"] > 10 * FRAME_BOUND


def test_refuses_what_it_was_not_tested_for():
    from diff_vits_amd import _lib
    L = _lib.lib()
    a = torch.zeros(16, device="cuda")
    ln = torch.ones(1, dtype=torch.int64, device="cuda")
    args = lambda T, d, w: (_lib.ptr(a),) * 5 + (_lib.ptr(ln), _lib.ptr(a), 1, 1, T, d, w, _lib.stream_ptr())     # noqa: E731
    for T, d, w, word in ((513, 128, 4, b"T = 513"), (8, 48, 4, b"d = 48"), (8, 128, 17, b"window = 17"), (0, 128, 4, b"T = 0")):
        assert L.dv_op_rel_attention(*args(T, d, w)) == -1
        assert word in L.dv_last_error(), L.dv_last_error()


# ---- the kernel's own edges ----------------------------------------------------------------------------------------------------------
EDGE_CASES = [(d, T) for d in (32, 128) for T in (33, 75)]
EDGE_IDS = ["d%d-T%d" % c for c in EDGE_CASES]
WINDOW = 4


def _planes32(a):
    """The two bf16 planes of a float32 tensor, as float32."""
    hi = a.to(torch.bfloat16).float()
    return hi, (a - hi).to(torch.bfloat16).float()


def core_emulated(q, k, v, ek, ev, lengths, window, planes=False):
    """core_fp64 with the arithmetic csrc/kernels_relattn.hip documents: the logits in fp32 (planes=True: q d^-1/2 and k each kept
    to two bf16 planes, the lo x lo product dropped, the three products accumulated in fp32), the band logits in fp32, exp(s - max)
    rounded to ONE fp16 plane before P V, the band probabilities from the same scores with the final maximum and sum."""
    B, T, Hn, d = q.shape
    qs = (q.double() / math.sqrt(d)).float().permute(0, 2, 1, 3)
    kf = k.float().permute(0, 2, 1, 3)
    if planes:
        (qh, ql), (kh, kl) = _planes32(qs), _planes32(kf)
        s32 = qh @ kl.transpose(-1, -2) + ql @ kh.transpose(-1, -2) + qh @ kh.transpose(-1, -2)
    else:
        s32 = (qs.double() @ kf.double().transpose(-1, -2)).float()
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    off = j - i + window
    band = (off >= 0) & (off <= 2 * window)
    rel = (qs.double() @ ek.double().t()).float()
    s32 = s32 + rel.gather(-1, off.clamp(0, 2 * window).expand(B, Hn, T, T)) * band
    keep = torch.arange(T)[None, :] < lengths[:, None]
    s = s32.double().masked_fill(~keep[:, None, None, :], -float("inf"))
    e = torch.exp(s - s.amax(-1, keepdim=True))
    l = e.sum(-1, keepdim=True)
    out = (e.half().double() @ v.double().permute(0, 2, 1, 3)) / l
    jj = i + torch.arange(2 * window + 1)[None, :] - window
    pb = e.gather(-1, jj.clamp(0, T - 1).expand(B, Hn, T, 2 * window + 1)) / l * ((jj >= 0) & (jj < T))
    out = out + pb @ ev.double()
    return out.permute(0, 2, 1, 3).reshape(B, T, Hn * d) * keep.double()[:, :, None]


def _edge(label, q, k, v, ek, ev, lengths, planes=False):
    """Runs the kernel and applies the three criteria; returns (fe, row bound, the emulation's own worst row)."""
    want = core_fp64(q, k, v, ek, ev, lengths, WINDOW)
    emu = masked_frame_errors(core_emulated(q, k, v, ek, ev, lengths, WINDOW, planes), want, lengths.tolist())
    bound = 2.0 * emu["worst"] + 2.0 ** -16
    got = _run(q, k, v, ek, ev, lengths, WINDOW)
    assert bool(torch.isfinite(got).all()), "rows the kernel did not write"
    fe = masked_frame_errors(got, want, lengths.tolist())
    line = "%-34s rel_l2 %.3e worst row %.3e at %s; emulation worst row %.3e, row bound %.3e; FRAME_BOUND %.0e" % (
        label, fe["rel_l2"], fe["worst"], fe["at"], emu["worst"], bound, FRAME_BOUND)
    print(line)
    path = os.environ.get("DVITS_PARITY_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")
    assert fe["padding_zero"], "row %s behind its utterance's length is not zero" % (fe["first_nonzero"],)
    assert fe["worst"] < FRAME_BOUND, (fe["worst"], fe["at"])
    assert fe["rel_l2"] < 2e-4, fe["rel_l2"]
    assert fe["worst"] < bound, (fe["worst"], bound, fe["at"])
    return fe, bound, emu["worst"]


@pytest.mark.parametrize("gain", [4, 8])
@pytest.mark.parametrize("d,T", EDGE_CASES, ids=EDGE_IDS)
def test_logit_gain_on_q(d, T, gain):
    """q x 4 and q x 8: logits of std 4 and 8, the other keys' weights in or near fp16's subnormal range relative to the running
    maximum.  The emulation forms the logits in fp32 and rounds exp(s - max) to fp16 before P V."""
    q, k, v, ek, ev, lengths = _tensors(d, T, WINDOW)
    _edge("rel_attention d=%d T=%d q x %d" % (d, T, gain), q * float(gain), k, v, ek, ev, lengths)


@pytest.mark.parametrize("where", ["first-tile", "last-tile"])
@pytest.mark.parametrize("d,T", EDGE_CASES, ids=EDGE_IDS)
def test_dominant_key(d, T, where):
    """One key of every utterance - key 2 (the first 32-key tile: the running maximum rises at once) or the utterance's last key,
    length - 1, which lies in its last tile (length - 1) // 32 (the maximum rises after every other key was weighted against a
    smaller one; at T = 33 that is key 32, alone in utterance 0's second tile - the utterances of 32 and 31 tokens have one tile)
    - carries +12 in natural units on every query's logit,
    through q and k: q += a u and k[key] += a u with a^2 d^-1/2 = 12, u a unit vector.  The key is inside the band of the queries
    within 4 tokens of it and outside the band of all others."""
    from diff_vits_amd import synth
    q, k, v, ek, ev, lengths = _tensors(d, T, WINDOW)
    u = torch.from_numpy(synth.normal(1234, "ra.dominant.u.%d" % d, (d,))).double()
    u = (u / u.norm()).float()
    a = math.sqrt(12.0 * math.sqrt(d))
    q, k = q + a * u, k.clone()
    for b, n in enumerate(lengths.tolist()):
        k[b, 2 if where == "first-tile" else n - 1] += a * u
    want = core_fp64(q, k, v, ek, ev, lengths, WINDOW)
    if where == "last-tile":
        assert (lengths.max().item() - 1) // 32 >= 1                                   # the longest utterance's key is past tile 0
    plain = core_fp64(q, _tensors(d, T, WINDOW)[1], v, ek, ev, lengths, WINDOW)
    assert masked_frame_errors(plain, want, lengths.tolist())["rel_l2"] > 0.5          # the key does dominate
    _edge("rel_attention d=%d T=%d dominant %s" % (d, T, where), q, k, v, ek, ev, lengths)


@pytest.mark.parametrize("c", [0, 4, 16])
@pytest.mark.parametrize("d,T", EDGE_CASES, ids=EDGE_IDS)
def test_common_key_offset(d, T, c):
    """k + c u on every key, u a fixed unit-scale channel vector (what a common offset in conv_k.bias does): q . c u is one number
    per query, the softmax does not see it - asserted on the fp64 reference first - but K Q^T is formed from two bf16 planes per
    operand and three of the four cross products, about 16 significand bits relative to sum |q_c k_c|, which grows with c.  The
    emulation keeps each operand to two bf16 planes, drops lo x lo and accumulates in fp32.  c = 0 is the same tensors without the
    offset: the baseline the other two rows are read against."""
    from diff_vits_amd import synth
    q, k, v, ek, ev, lengths = _tensors(d, T, WINDOW)
    u = torch.from_numpy(synth.normal(1234, "ra.offset.u.%d" % d, (d,)))
    kc = (k.double() + float(c) * u.double()).float()
    base = core_fp64(q, k, v, ek, ev, lengths, WINDOW)
    moved = masked_frame_errors(core_fp64(q, kc, v, ek, ev, lengths, WINDOW), base, lengths.tolist())
    assert moved["worst"] < 1e-5, moved["worst"]          # (the fp32 rounding of k + c u: 2^-24 c on a logit's operands)
    _edge("rel_attention d=%d T=%d k + %d u" % (d, T, c), q, kc, v, ek, ev, lengths, planes=True)
