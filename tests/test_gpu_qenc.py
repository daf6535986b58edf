"""Native posterior encoder on the reference's golden (tests/golden/align_forward.npz): z / m_q / logs_q against the reference's
tensors under the bounds of tests/test_gpu_qenc_layerwise.py, and a fully native VITS.align - text encoder, posterior encoder,
scores and search on the HIP engines - returning the golden path.

Path identity is guaranteed only while 2 * Ty * (largest deviation of the native scores from the golden neg_cent) stays below the
fixture's smallest decision margin (align_cases.search_ref): the test computes and prints both figures; if the condition holds it
asserts the golden integers, otherwise equality with the restated search on the run's own scores (as tests/test_gpu_align.py)."""
import numpy as np
import pytest
import torch

import align_cases as A
import parity_metrics as pm
from conftest import rel_l2

pytestmark = pytest.mark.gpu

TENSOR_BOUND, FRAME_BOUND = 2e-4, pm.FRAME_BOUND


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def case(gold):
    from test_align_cpu import align_case, align_mirror
    g, sd, y, noise = align_case(gold)
    native = align_mirror(g, sd, posterior_backend="hip", text_encoder_backend="hip").cuda()
    torch_route = align_mirror(g, sd).cuda()
    args = [_dev(a) for a in (g["text"], g["x_lengths"], y, g["y_lengths"], g["tone"], g["language"])]
    return g, native, torch_route, args, _dev(noise)


def _within(label, got, want, lengths):
    """got / want channels-first [B, C, T]; valid frames within the bounds, padding of `got` exactly zero."""
    fe = pm.masked_frame_errors(got.transpose(1, 2), np.swapaxes(np.asarray(want), 1, 2), lengths)
    print("%s: tensor %.3e, worst frame %.3e" % (label, fe["rel_l2"], fe["worst"]))
    assert fe["padding_zero"], fe["first_nonzero"]
    assert fe["rel_l2"] < TENSOR_BOUND and fe["worst"] < FRAME_BOUND, label


def test_posterior_on_the_golden(case):
    g, native, torch_route, args, noise = case
    y, yl = args[2], args[3]
    with torch.no_grad():
        gg = native.ref_enc(y.transpose(1, 2)).unsqueeze(-1)
        before = native.native_posterior_calls
        z, m, logs, mask = native.enc_q(y, yl, gg, noise=noise)
        assert native.native_posterior_calls == before + 1
        zt, mt, lt, mask_t = torch_route.enc_q(y, yl, gg, noise=noise)
    torch.cuda.synchronize()
    assert torch.equal(mask, mask_t) and torch_route.native_posterior_calls == 0
    for k, a, t in (("z", z, zt), ("m_q", m, mt), ("logs_q", logs, lt)):
        _within("native vs golden " + k, a, g[k], g["y_lengths"])
        _within("native vs torch route " + k, a, t.cpu().numpy(), g["y_lengths"])


def test_fully_native_align_returns_the_golden_path(case):
    from test_align_cpu import golden_path
    g, native, torch_route, args, noise = case
    calls = (native.native_posterior_calls, native.native_align_calls)
    dur, tok, scores = native.align(*args, noise=noise, align_backend="hip", return_scores=True)
    torch.cuda.synchronize()
    assert (native.native_posterior_calls, native.native_align_calls) == (calls[0] + 1, calls[1] + 1)
    s = scores.cpu().numpy()
    dev = max(float(np.abs(s[b, :ty, :tx].astype(np.float64) - g["neg_cent"][b, :ty, :tx]).max())
              for b, (ty, tx) in enumerate(zip(g["y_lengths"], g["x_lengths"])))
    margin = A.search_ref(g["neg_cent"], g["y_lengths"], g["x_lengths"])[2]
    need = 2 * int(g["Ty"]) * dev
    print("fully native align: largest score deviation %.3e, 2 * Ty * deviation = %.3e, smallest golden margin %.3g" % (dev, need, margin))
    if need < margin:
        gd, gt = golden_path(g)
        assert np.array_equal(dur.cpu().numpy(), gd) and np.array_equal(tok.cpu().numpy(), gt)
    else:
        wd, wt, _ = A.search_ref(s, g["y_lengths"], g["x_lengths"])
        assert np.array_equal(dur.cpu().numpy(), wd) and np.array_equal(tok.cpu().numpy(), wt)
    # the default route is untouched and agrees: its scores within 1e-5 of the native ones (tests/test_gpu_align.py's figure for
    # scores), its path identical where the margin condition guarantees that
    d2, t2, s2 = torch_route.align(*args, noise=noise, return_scores=True)
    s2 = s2.cpu().numpy()
    for b, (ty, tx) in enumerate(zip(g["y_lengths"], g["x_lengths"])):
        assert rel_l2(s[b, :ty, :tx], s2[b, :ty, :tx]) < 1e-5, b
    if need < margin:
        assert torch.equal(d2, dur) and torch.equal(t2, tok)
    assert torch_route.native_posterior_calls == 0 and torch_route.native_align_calls == 0
