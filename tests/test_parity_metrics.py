"""CPU: faults of the kind a tiled kernel makes, planted in an oracle tensor of the bench shape, pass the whole-tensor
relative-L2 bar of the GPU tests (2e-4) and are caught - and located - by the per-frame, per-block and localisation metrics of
tests/parity_metrics.py.  The second half plants the prompt encoder's faults (ragged batch, masked tensors) in oracle tensors of
its B = 3 / L = 75 case; three of the four cannot be diluted below the whole-tensor bar at that size and say so.  Every case carries the rounding noise of a correct kernel as well (3e-5 relative per element, the
level the HIP path shows against the oracle), so the metrics are shown to separate a fault from noise, not from nothing."""
import numpy as np
import pytest
import torch

from conftest import UNET_CASES
from parity_metrics import (FRAME_BOUND, LOCALISATION_BOUND, PENC_LOCALISATION_BOUND, block_errors, describe, expected_probes,
                            frame_errors, localisation, masked_frame_errors, oracle_probes, prompt_oracle_probes,
                            prompt_probe_names, split_valid)

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


# ---- the prompt encoder: masked tensors of a ragged batch (tests/test_gpu_prompt_layerwise.py) ---------------------------------
@pytest.fixture(scope="module")
def penc():
    """Oracle tensors of the B = 3 / L = 75 case (lengths 75, 1, 50; flavour D), fp64 weights for the faults' own arithmetic."""
    import prompt_cases as pc
    from oracle import prompt_ref
    name, flavour, pB, pL, lengths = pc.case("D-3x75")
    sd = pc.state_dict(flavour)
    prompt, ln = pc.inputs(flavour, pB, pL, lengths)
    with torch.no_grad():
        y, probes = prompt_oracle_probes(sd, prompt, ln, 4)
        plain = prompt_ref.prompt_encoder(sd, prompt, ln, 4)
    assert torch.equal(plain.permute(0, 2, 1), y)                    # the wrappers change nothing the oracle computes
    pad = ~prompt_ref.sequence_mask(ln, pL)
    return {k: v.double() for k, v in sd.items()}, probes, lengths, pad, pc


def _penc_check(pc, name, got, want, lengths, masked=True):
    report, failures = [], []
    fe = pc.check(name, got, want, lengths, report, failures, masked)
    return fe, "".join(failures)


def test_prompt_oracle_probes_equal_the_goldens_and_restore_the_oracle(gold):
    """The oracle's probes of the golden case (D, B = 2, L = 40) through prompt_oracle_probes: the five the goldens carry within
    1e-6, the new ones with the right shapes, padding exactly zero where the schedule masks; oracle.prompt_ref is left as found."""
    import prompt_cases as pc
    from oracle import prompt_ref
    before = (prompt_ref.enc_sa_layer, prompt_ref.ffn, prompt_ref.conv_layer)
    name, flavour, pB, pL, lengths = pc.case("D-2x40")
    g = gold("prompt_cfg.npz")
    prompt, ln = pc.inputs(flavour, pB, pL, lengths)
    with torch.no_grad():
        y, probes = prompt_oracle_probes(pc.state_dict(flavour), prompt, ln, 4)
    assert (prompt_ref.enc_sa_layer, prompt_ref.ffn, prompt_ref.conv_layer) == before
    assert list(probes) == prompt_probe_names(4) and len(probes) == 1 + 3 * 4 + 1
    rel = lambda a, b: float(np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b))    # noqa: E731
    assert rel(y.permute(0, 2, 1).numpy(), g["enc"]) < 1e-6
    for k in ["pre"] + ["layer%d" % i for i in range(4)]:
        assert rel(probes[k].numpy(), g["probe_" + k]) < 1e-6, k
    for k, v in probes.items():
        assert tuple(v.shape) == (pB, pL, 512 if k.endswith(".ffn1") else 128), k
        sv = split_valid(v, v, lengths)
        assert sv["padding_zero"] == (not k.endswith(".ffn1")), k
        assert sv["got"].shape == (1, 67, v.shape[2]) and [tuple(r) for r in sv["where"][[0, 39, 40, 66]]] == [(0, 0), (0, 39), (1, 0), (1, 26)]
    # the last valid frame of the first utterance and the first of the next are neighbours in the concatenation
    fe = masked_frame_errors(probes["layer1"] * 1.0001, probes["layer1"], lengths)
    assert fe["frames"] == 67 and fe["floored"] == 0 and abs(fe["rel_l2"] - 1e-4) < 1e-6 and fe["per_frame"].shape == (pB, pL)
    assert np.all(fe["per_frame"][1, 27:] == 0)


def test_rounding_noise_alone_passes_every_prompt_criterion(penc):
    sd, probes, lengths, pad, pc = penc
    for k, want in probes.items():
        fe, why = _penc_check(pc, k, _noisy(want), want, lengths, masked=not k.endswith(".ffn1"))
        assert not why and fe["floored"] == 0, why


def test_penc_taps_read_across_the_utterance_boundary(penc):
    """(a) the last four valid frames of utterance 0 (length 75 = L) take taps 5..8 (offsets +1..+4) of layer 1's feed-forward
    from the next rows of the flat [B * L] row space - the first frames of utterance 1 - instead of zeros.
    At this size the fault cannot pass the whole-tensor bar: four frames of 126 valid ones, each wrong by tens of per cent, leave
    5.7e-2 on layer1.ffn1 and 2.8e-2 on layer1.  Kept as a plain detection test: the per-frame criteria name the frames."""
    import torch.nn.functional as F
    sd, probes, lengths, pad, pc = penc
    p, L_ = "layers.1.op.", 75
    x2 = probes["layer1.attn"].double()
    n2 = F.layer_norm(x2, (128,), sd[p + "layer_norm2.weight"], sd[p + "layer_norm2.bias"], 1e-5)
    flat, xt = n2.reshape(-1, 128), n2.permute(1, 0, 2)
    padded, res = F.pad(xt, (0, 0, 0, 0, 4, 4)), 0
    for i in range(9):
        res = res + F.linear(padded[i:L_ + i] if i else xt, sd[p + "ffn.ffn_1.%d.weight" % i], sd[p + "ffn.ffn_1.0.bias"] if i == 0 else None)
    res = res.permute(1, 0, 2).clone()
    assert torch.allclose(F.relu(res / 3.0), probes["layer1.ffn1"].double(), atol=1e-5)      # the fault starts from the oracle's sum
    for t in range(71, 75):
        for i in range(5, 9):
            if t + i - 4 >= L_:
                res[0, t] += F.linear(flat[t + i - 4], sd[p + "ffn.ffn_1.%d.weight" % i])
    h = F.relu(res / 3.0)
    got = _noisy(probes["layer1.ffn1"])
    got[0, 71:75] = h[0, 71:75]
    fe, why = _penc_check(pc, "(a) layer1.ffn1", got, probes["layer1.ffn1"], lengths, masked=False)
    assert fe["at"] == (0, 74) and fe["worst"] > FRAME_BOUND and "utterance 0 frame 74" in why and "rows 64..74 of utterance 0" in why, why
    assert sorted(int(i) for i in np.argsort(fe["per_frame"][0])[-4:]) == [71, 72, 73, 74]
    keep = (~pad).double()[:, :, None]
    out = (x2 + F.linear(h, sd[p + "ffn.ffn_2.weight"], sd[p + "ffn.ffn_2.bias"])) * keep
    got = _noisy(probes["layer1"])
    got[0, 71:75] = out[0, 71:75]
    fe, why = _penc_check(pc, "(a) layer1", got, probes["layer1"], lengths)
    assert fe["at"] == (0, 74) and fe["worst"] > FRAME_BOUND and fe["worst"] / fe["rel_l2"] > PENC_LOCALISATION_BOUND, why
    assert fe["rel_l2"] > OLD_BAR            # (see the docstring: not diluted at this size)


def test_penc_row_mask_dropped_on_one_row_block(penc):
    """(b) the epilogue of layer 1's ffn_2 GEMM leaves the keep mask out for rows 32..63 of utterance 2 (length 50): frames 50..63
    hold x2 + ffn_2(h) of padding rows instead of zeros.  The valid frames are untouched - whole tensor, every frame and the
    localisation ratio pass - and only the padding criterion sees it, with the first such frame."""
    import torch.nn.functional as F
    sd, probes, lengths, pad, pc = penc
    p = "layers.1.op."
    unmasked = probes["layer1.attn"].double() + F.linear(probes["layer1.ffn1"].double(), sd[p + "ffn.ffn_2.weight"], sd[p + "ffn.ffn_2.bias"])
    got = _noisy(probes["layer1"])
    got[2, 50:64] = unmasked[2, 50:64]
    fe, why = _penc_check(pc, "(b) layer1", got, probes["layer1"], lengths)
    assert fe["rel_l2"] < OLD_BAR and fe["worst"] < FRAME_BOUND and fe["worst"] / fe["rel_l2"] < PENC_LOCALISATION_BOUND
    assert not fe["padding_zero"] and fe["first_nonzero"] == (2, 50)
    assert why.endswith("[padding frame 50 of utterance 2 is not zero]"), why


def test_penc_lost_lo_plane_in_one_tile_of_ffn1(penc):
    """(c) one 64 x 64 tile of layer1.ffn1 ([3, 75, 512]) re-rounded to bf16.
    At this size the fault cannot pass the whole-tensor bar: the tile is 64 of 126 valid frames x 1 / 8 of the columns, which leaves
    4.2e-4 on the tensor.  Kept as a plain detection test, and what detects it is the 64 x 64 block metric (1.7e-3 in exactly that
    tile, 4 x the tensor), which describe() puts into every failure message; one frame carries 7.6e-4, below FRAME_BOUND, and the
    ratio is 1.8: on a 512-wide tensor a fault in 64 columns of 64 rows is NOT caught by the per-frame criteria alone."""
    sd, probes, lengths, pad, pc = penc
    want = probes["layer1.ffn1"]
    got = _noisy(want)
    got[0, 0:64, 64:128] = want[0, 0:64, 64:128].to(torch.bfloat16).double()
    fe, why = _penc_check(pc, "(c) layer1.ffn1", got, want, lengths, masked=False)
    assert OLD_BAR < fe["rel_l2"] < 3 * OLD_BAR and "whole tensor" in why
    be = block_errors(got, want, 64, 64, lengths)
    assert (be["utterance"], be["rows"], be["cols"]) == (0, (0, 64), (64, 128)), be
    assert be["worst"] > FRAME_BOUND and be["worst"] > 3.5 * fe["rel_l2"]
    assert "rows 0..63 of utterance 0, columns 64..127" in why


def test_penc_key_bias_off_by_one_key(penc):
    """(d) utterance 2 (length 50) attends its first padded key (key 50) in layer 1's self-attention.
    At this size the fault cannot pass the whole-tensor bar: every one of the utterance's 50 frames (of 126) moves by 1 - 2 %, which
    leaves 8.4e-3 on the tensor.  Kept as a plain detection test: every frame of utterance 2 and none of the others is over
    FRAME_BOUND, and the message names the utterance."""
    import torch.nn.functional as F
    from oracle import prompt_ref
    sd, probes, lengths, pad, pc = penc
    p = "layers.1.op."
    x = probes["layer0"].double().permute(1, 0, 2)
    n1 = F.layer_norm(x, (128,), sd[p + "layer_norm1.weight"], sd[p + "layer_norm1.bias"], 1e-5)
    same = ((x + prompt_ref.self_attention(sd, p + "self_attn.", n1, pad, 8)).permute(1, 0, 2)) * (~pad).double()[:, :, None]
    assert frame_errors(same, probes["layer1.attn"])["rel_l2"] < 1e-6                         # the fault starts from the oracle's tensor
    pad2 = pad.clone()
    pad2[2, 50] = False
    wrong = ((x + prompt_ref.self_attention(sd, p + "self_attn.", n1, pad2, 8)).permute(1, 0, 2)) * (~pad).double()[:, :, None]
    got = _noisy(probes["layer1.attn"])
    got[2] = wrong[2]
    fe, why = _penc_check(pc, "(d) layer1.attn", got, probes["layer1.attn"], lengths)
    assert fe["rel_l2"] > OLD_BAR and fe["padding_zero"]
    assert np.all(fe["per_frame"][2, :50] > FRAME_BOUND) and np.all(fe["per_frame"][[0, 1]] < FRAME_BOUND)
    assert fe["at"][0] == 2 and "of utterance 2" in why and "a frame at" in why, why
