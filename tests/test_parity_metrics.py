"""CPU: faults of the kind a tiled kernel makes, planted in an oracle tensor of the bench shape, pass the whole-tensor
relative-L2 bar of the GPU tests (2e-4) and are caught - and located - by the per-frame, per-block and localisation metrics of
tests/parity_metrics.py.  Every case carries the rounding noise of a correct kernel as well (3e-5 relative per element, the
level the HIP path shows against the oracle), so the metrics are shown to separate a fault from noise, not from nothing."""
import numpy as np
import pytest
import torch

from conftest import UNET_CASES
from parity_metrics import (FRAME_BOUND, LOCALISATION_BOUND, block_errors, describe, expected_probes, frame_errors, localisation,
                            oracle_probes)

B, T, L = 8, 1024, 32            # the benchmark's batch and length (the prompt length does not matter here)
OLD_BAR = 2e-4                   # whole-tensor relative L2 of the layer-wise GPU tests
NOISE = 3e-5


@pytest.fixture(scope="module")
def oracle():
    from diff_vits_amd import synth
    from diff_vits_amd.unet1d.unet_1d_condition import UNet1DConditionModel
    kw = UNET_CASES["cfg1"][0]
    with torch.device("meta"):
        model = UNet1DConditionModel(**kw)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(shapes, seed=1234).items()}
    x, cond, enc, mask = (torch.from_numpy(a) for a in synth.make_inputs(B, 80, T, L, seed=11, ragged_mask=True))
    with torch.no_grad():
        y, probes = oracle_probes(kw, sd, torch.cat([x, cond], 1), torch.linspace(900.0, 20.0, B), enc, mask)
    return model, sd, probes


def _noisy(want, seed=5):
    g = torch.Generator().manual_seed(seed)
    return want.double() * (1.0 + NOISE * torch.randn(want.shape, generator=g, dtype=torch.float64))


def test_probe_list_comes_from_the_module_tree(oracle):
    model, _, probes = oracle
    names = expected_probes(model)
    assert len(names) == 2 + 22 * 2 + 16 * 5 + 6 and len(set(names)) == len(names)
    assert set(names) == set(probes)


def test_rounding_noise_alone_passes_every_criterion(oracle):
    want = oracle[2]["down_blocks.0.resnets.0.conv1"]
    assert tuple(want.shape) == (B, T, 128)
    got = _noisy(want)
    fe = frame_errors(got, want)
    assert fe["floored_ok"] and fe["rel_l2"] < OLD_BAR and fe["worst"] < FRAME_BOUND
    assert localisation(got, want) < LOCALISATION_BOUND / 2, localisation(got, want)


def test_lost_lo_plane_in_one_tile(oracle):
    """(a) one 64 x 64 tile of a [8192, 128] tensor whose values were re-rounded to bf16 (the epilogue dropped the `lo` plane)."""
    want = oracle[2]["down_blocks.0.resnets.0.conv1"]
    got = _noisy(want)
    got[2, 192:256, 64:128] = want[2, 192:256, 64:128].to(torch.bfloat16).double()
    fe = frame_errors(got, want)
    assert fe["rel_l2"] < OLD_BAR, fe["rel_l2"]                      # the gap: the old criterion passes
    ratio = localisation(got, want)
    assert ratio > LOCALISATION_BOUND, (ratio, describe("(a)", got, want))
    assert fe["at"][0] == 2 and 192 <= fe["at"][1] < 256
    be = block_errors(got, want, 64, 64)
    assert (be["utterance"], be["rows"], be["cols"]) == (2, (192, 256), (64, 128)), be
    assert be["worst"] > 8 * fe["rel_l2"]
    assert "rows 192..255 of utterance 2, columns 64..127" in describe("(a)", got, want)


def test_halo_of_the_last_frame_read_from_the_next_row(oracle):
    """(b) the last frame of each utterance computed with the row behind it as its right conv halo instead of zeros; that row
    holds leftovers of 1 % of a real frame's magnitude (what a producer's GroupNorm makes of a padding row)."""
    model, sd, probes = oracle
    want = probes["down_blocks.0.resnets.0.conv1"]
    w = sd["down_blocks.0.resnets.0.conv1.weight"].double()           # [Cout, Cin, 3]
    x = probes["conv_in"].double()                                    # a tensor of the conv's input width
    g = sd["down_blocks.0.resnets.0.norm1.weight"].double()
    xin = torch.nn.functional.silu(torch.nn.functional.group_norm(x.permute(0, 2, 1), 8, g,
                                                                  sd["down_blocks.0.resnets.0.norm1.bias"].double(), 1e-5))
    got = _noisy(want)
    for b in range(B):
        leftovers = 0.01 * xin[(b + 1) % B, :, 0]                     # the next row of the flat [B * T] row space
        got[b, T - 1] += w[:, :, 2] @ leftovers
    fe = frame_errors(got, want)
    assert fe["rel_l2"] < OLD_BAR, fe["rel_l2"]
    assert fe["worst"] > FRAME_BOUND and fe["at"][1] == T - 1, fe["worst"]
    assert localisation(got, want) > LOCALISATION_BOUND
    worst = np.argsort(fe["per_frame"].ravel())[-B:]
    assert sorted(int(i) % T for i in worst) == [T - 1] * B           # the eight worst frames: the last one of every utterance
    be = block_errors(got, want, 32, 1 << 30)
    assert be["rows"] == (T - 32, T), be


def test_one_head_of_one_row_block_scaled(oracle):
    """(c) one head's 16 columns of one 32-row block scaled by 1 + 2^-10 (a wrong softmax denominator in one wave)."""
    want = oracle[2]["down_blocks.0.attentions.0.transformer_blocks.0.attn1"]
    assert tuple(want.shape) == (B, T, 128)
    got = _noisy(want)
    got[5, 640:672, 48:64] = want[5, 640:672, 48:64].double() * (1.0 + 2.0 ** -10)
    fe = frame_errors(got, want)
    assert fe["rel_l2"] < OLD_BAR / 4, fe["rel_l2"]
    ratio = localisation(got, want)
    assert ratio > LOCALISATION_BOUND, (ratio, describe("(c)", got, want))
    assert fe["at"][0] == 5 and 640 <= fe["at"][1] < 672
    be = block_errors(got, want, 32, 16)
    assert (be["utterance"], be["rows"], be["cols"]) == (5, (640, 672), (48, 64)), be
    be = block_errors(got, want, 32, 1 << 30)
    assert (be["utterance"], be["rows"]) == (5, (640, 672)), be


def test_every_probe_of_the_bench_shape_keeps_off_the_floor(oracle):
    """Condition of the per-frame metric: at most 1 % of a probe's frames may have a norm below the floor."""
    bad = {n: (fe["floored"], fe["frames"]) for n, v in oracle[2].items() for fe in [frame_errors(v, v)] if not fe["floored_ok"]}
    assert not bad, bad
