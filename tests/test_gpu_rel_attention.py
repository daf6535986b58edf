"""GPU: k_rel_attention alone (dv_op_rel_attention, csrc/kernels_relattn.hip) against the attention core of
oracle.text_enc_ref.rel_attention - what sits between the q / k / v projections and conv_o - restated here in fp64 torch.

Criteria on the valid rows (tests/parity_metrics.py): every frame < FRAME_BOUND = 1e-3 and whole-tensor relative L2 < 2e-4; rows of
an utterance behind its length are exactly zero.  Shapes: head dims 32 / 64 / 128 at window 4 and B = 3 with T = 1, 5 (every
offset of the window exists exactly once), 9, 31, 32, 33 (either side of the 32-key tile), 75 (ragged 75 / 40 / 9) and 300; windows
1 and 8 at T = 33; and T = 512, the longest the kernel accepts (the launcher refuses longer ones: checked without a launch)."""
import ctypes as C
import math

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
