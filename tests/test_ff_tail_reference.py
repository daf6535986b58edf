"""CPU: the isolated check of the one-launch feed-forward (tests/test_gpu_tapped_schedule.py) has teeth.

That check feeds the engine's own taps of h3 (`...attn2`) and of the transformer's input x through parity_metrics.ff_tail_fp64 and
compares the result with the tapped `attentions.i` under FF_TAIL_BOUND = 1e-4 (whole tensor and every frame).  Here the same
restatement is (1) compared with oracle.unet_ref's own transformer block on the same h3 and x, and (2) given the faults a
column-split row-block kernel makes; each must move the worst frame above 10 x the bound ON THE FULL OUTPUT - the residual x
does not dilute them below it, so the GPU test compares the full output and not `got - x`."""
import numpy as np
import pytest
import torch

from conftest import UNET_CASES
from parity_metrics import FF_TAIL_BOUND, ff_tail_fp64, frame_errors, oracle_probes, seam_figures

B, T, L = 2, 100, 20
BLOCKS = ["down_blocks.0.attentions.1.", "up_blocks.2.attentions.0.", "down_blocks.2.attentions.0.", "mid_block.attentions.0."]   # C = 128, 256, 384, 512
NOISE = 1e-5                # the level SURVEY section 7 measures for one split-bf16 contraction


def _input_of(p):
    """The tensor a transformer reads: the resnet block before it (down_blocks.i.resnets.j -> attentions.j; mid: resnets.0)."""
    return p.replace("attentions", "resnets")[:-1]


@pytest.fixture(scope="module")
def oracle():
    from diff_vits_amd import synth
    from diff_vits_amd.unet1d.unet_1d_condition import UNet1DConditionModel
    kw = UNET_CASES["cfg1"][0]
    with torch.device("meta"):
        shapes = {k: tuple(v.shape) for k, v in UNet1DConditionModel(**kw).state_dict().items()}
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(shapes, seed=1234).items()}
    x, cond, enc, mask = (torch.from_numpy(a) for a in synth.make_inputs(B, 80, T, L, seed=11, ragged_mask=True))
    with torch.no_grad():
        _, probes = oracle_probes(kw, sd, torch.cat([x, cond], 1), torch.tensor([949.05, 311.0]), enc, mask)
    return sd, probes


def _tensors(oracle, p):
    sd, probes = oracle
    return sd, probes[p + "transformer_blocks.0.attn2"], probes[_input_of(p)], probes[p[:-1]]


@pytest.mark.parametrize("p", BLOCKS[:2], ids=["C128", "C256"])
def test_restatement_agrees_with_the_oracle_block(oracle, p):
    """The oracle's block ran in fp32 on exactly this h3 and x (they are its own intermediates): 1e-6, whole tensor and per frame."""
    sd, h3, x, out = _tensors(oracle, p)
    fe = frame_errors(out, ff_tail_fp64(sd, p, h3, x))
    assert fe["floored_ok"] and fe["rel_l2"] < 1e-6 and fe["worst"] < 1e-6, fe


def _noisy(want):
    g = torch.Generator().manual_seed(5)
    return want * (1.0 + NOISE * torch.randn(want.shape, generator=g, dtype=torch.float64))


@pytest.mark.parametrize("p", BLOCKS, ids=["C128", "C256", "C384", "C512"])
def test_planted_faults_exceed_ten_times_the_bound(oracle, p):
    sd, h3, x, _ = _tensors(oracle, p)
    want = ff_tail_fp64(sd, p, h3, x)
    Tn, C = want.shape[1:]
    fe = frame_errors(_noisy(want), want)
    assert fe["rel_l2"] < FF_TAIL_BOUND and fe["worst"] < FF_TAIL_BOUND, fe          # a correct kernel's noise passes
    faults = {"feed-forward term dropped": ff_tail_fp64(sd, p, h3, x, drop_ff=True),
              "GEGLU halves swapped": ff_tail_fp64(sd, p, h3, x, swap_geglu=True)}
    # one 32-row x 64-column tile holds the neighbouring workgroup's column strip (rows of the last, partly filled row block)
    r0 = (Tn - 1) // 32 * 32
    tile = _noisy(want)
    tile[1, r0:r0 + 32, 0:64] = want[1, r0:r0 + 32, 64:128]
    faults["tile from the neighbouring strip"] = tile
    # one padding row's garbage (3e4, as test_conv3 plants it) added into the last valid frame
    leak = _noisy(want)
    leak[0, Tn - 1] += torch.from_numpy(3.0e4 * np.random.default_rng(7).standard_normal(C))
    faults["padding row leaked"] = leak
    for name, got in faults.items():
        fe = frame_errors(got, want)
        print("%s C=%d: tensor %.2e worst frame %.2e at %s" % (name, C, fe["rel_l2"], fe["worst"], fe["at"]))
        assert fe["worst"] > 10 * FF_TAIL_BOUND, (name, fe["worst"])
    fe = frame_errors(faults["tile from the neighbouring strip"], want)
    assert fe["at"][0] == 1 and r0 <= fe["at"][1] < r0 + 32
    fe = frame_errors(faults["padding row leaked"], want)
    assert fe["at"] == (0, Tn - 1)
    assert seam_figures(fe["per_frame"], 32)["last"] == fe["worst"]


def test_seam_figures_split_the_frames():
    per = np.zeros((2, 100))
    per[0, 0], per[1, 99], per[0, 31], per[1, 64], per[0, 50] = 1, 2, 3, 4, 5
    assert seam_figures(per, 32) == {"first": 1.0, "last": 2.0, "seams": 4.0, "inner": 5.0}
    assert seam_figures(per, 64)["seams"] == 4.0 and seam_figures(per, 64)["inner"] == 5.0
