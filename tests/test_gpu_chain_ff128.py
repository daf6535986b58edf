"""GPU: the C = 128 transformer blocks with the cross-attention chain and the feed-forward chain in ONE launch (k_chain_xa_ff,
kernels_chain.hip) against the two launches it replaces (DVITS_CHAIN_MERGE_FF128=0: k_chain2<1, 0, true> then k_chain_ff).

The merged launch keeps h3, its split planes and its LayerNorm row partials in LDS and changes no arithmetic, so everything
here is compared BIT FOR BIT: two engines in one process on the same weights and inputs, every tap of the production plan
(DVITS_KEEP_INTERMEDIATES=tap - with `1` the plan has no one-launch feed-forward at all, see tests/test_gpu_tapped_schedule.py)
and the output.  The plans are asserted from eng.profile_forward; no hand-over may have timed out.  One forward is also held
against the oracle at the bound of tests/test_gpu_midblock_split.py (rel-L2 < 2e-4).

Shapes (cfg1: levels of T, T/2, T/4, T/8 frames at C = 128, 256, 384, 512 - the C = 128 level carries the kernel):
  2 x 64, L = 24    exactly 128 rows (the chain_min_rows edge), a prompt shorter than one 32-key tile
  2 x 100, L = 33   row pitch 128 with a short last row block; a second key tile that holds one valid key
  3 x 96, L = 70    ragged key mask: one utterance with a single valid key, one with all keys valid"""
import os

import numpy as np
import pytest
import torch

from conftest import UNET_CASES, oracle_cfg, rel_l2

pytestmark = pytest.mark.gpu

KW = UNET_CASES["cfg1"][0]
KNOB = "DVITS_CHAIN_MERGE_FF128"
MERGED = " after to_out+res+LN+to_q+xattn+to_out+res "
SHAPES = {"2x64-min-rows": (2, 64, 24), "2x100-padded": (2, 100, 33), "3x96-ragged": (3, 96, 70)}


@pytest.fixture(scope="module")
def weights():
    from diff_vits_amd import synth
    from diff_vits_amd.unet1d.unet_1d_condition import UNet1DConditionModel
    with torch.device("meta"):
        shapes = {k: tuple(v.shape) for k, v in UNet1DConditionModel(**KW).state_dict().items()}
    return {k: torch.from_numpy(v) for k, v in synth.make_state_dict(shapes, seed=808).items()}


def _inputs(B, T, L):
    from diff_vits_amd import synth
    x, cond, enc, _ = (torch.from_numpy(v) for v in synth.make_inputs(B, 80, T, L, seed=81))
    mask = torch.ones(B, L, dtype=torch.bool)
    if B == 3:                                      # ragged: one valid key / all keys / a tile and a half
        mask[0, 1:] = False
        mask[2, 48:] = False
    t = torch.linspace(949.05, 37.0, B)
    return x, cond, enc, mask, t


def _run(sd, B, T, L, knob, env=None, runs=1):
    """One engine on the tapped production plan: outputs of `runs` forwards, every tap, the plan rows, the hand-over status."""
    from diff_vits_amd.unet1d.unet_1d_condition import UNet1DConditionModel
    x, cond, enc, mask, t = _inputs(B, T, L)
    env = dict(env or {})
    env[KNOB] = knob
    env["DVITS_KEEP_INTERMEDIATES"] = "tap"
    os.environ.update(env)
    try:
        m = UNet1DConditionModel(backend="hip", **KW).eval()
        m.load_state_dict(sd)
        m = m.cuda()
        sample = torch.cat([x, cond], 1).cuda()
        with torch.no_grad():
            m(sample, t.cuda(), enc.cuda(), encoder_attention_mask=mask.cuda())       # (prepares the engine)
        eng = m.hip_engine()
        rows = [(r[0], r[3]) for r in eng.profile_forward(x.cuda(), cond.cuda(), t.cuda())]
        names = [d.split(" ")[0] for k, d in rows if k == "probe"]
        ys, taps = [], []
        for _ in range(runs):
            with torch.no_grad():
                ys.append(m(sample, t.cuda(), enc.cuda(), encoder_attention_mask=mask.cuda()).sample.cpu())
            torch.cuda.synchronize()
            taps.append({n: eng.probe(n).clone() for n in names})
        out = {"y": ys, "taps": taps, "rows": rows, "handover": eng.handover_status(), "downgraded": eng.handover_downgraded,
               "launches": eng.stats()[0], "flops": eng.stats()[1]}
        del m, eng
        return out
    finally:
        for k in env:
            os.environ.pop(k, None)


def _c128(rows):
    """The C = 128 blocks' launches of a plan: merged, the separate cross-attention chains, the separate k_chain_ff launches."""
    chain = [d for k, d in rows if k == "chain" and " C=128 " in d + " "]
    return {"merged": [d for d in chain if MERGED in d],
            "xa": [d for d in chain if d.startswith("to_out+res+LN+to_q+xattn+to_out+res M=")],
            "ff": [d for d in chain if d.startswith("LN+GEGLU+ffproj+res") and MERGED not in d]}


def _assert_same_bits(on, off):
    assert on["handover"][1] == 0 and off["handover"][1] == 0, (on["handover"], off["handover"])
    assert not on["downgraded"] and not off["downgraded"]
    p_on, p_off = _c128(on["rows"]), _c128(off["rows"])
    assert len(p_on["merged"]) == 5 and not p_on["xa"] and not p_on["ff"], p_on
    assert not p_off["merged"] and len(p_off["xa"]) == 5 and len(p_off["ff"]) == 5, p_off
    # the merged launch ends as the k_chain_ff launch it replaces does (GroupNorm finished in the launch or not, fp32 kept or not)
    assert [d.split(" ")[0] for d in p_on["merged"]] == [d.split(" ")[0] for d in p_off["ff"]], (p_on["merged"], p_off["ff"])
    assert off["launches"] - on["launches"] == 5 and on["flops"] == off["flops"], (on["launches"], off["launches"], on["flops"], off["flops"])
    t_on, t_off = on["taps"][0], off["taps"][0]
    assert set(t_on) == set(t_off) and len(t_on) >= 40, set(t_on) ^ set(t_off)
    assert sum(1 for n in t_on if n.endswith("transformer_blocks.0.attn2")) == 16      # h3 of every block, the merged ones included
    moved = [n for n in t_on if not np.array_equal(t_on[n].numpy(), t_off[n].numpy())]
    assert not moved, "taps that differ between one launch and two: %s" % moved[:8]
    assert np.array_equal(on["y"][0].numpy(), off["y"][0].numpy())
    assert np.isfinite(on["y"][0].numpy()).all()


@pytest.fixture(scope="module")
def small(weights):
    """2 x 64, L = 24 on the merged plan, run twice: shared by the bit-identity, repeatability and oracle tests."""
    return _run(weights, 2, 64, 24, "1", runs=2)


@pytest.mark.parametrize("shape", list(SHAPES), ids=list(SHAPES))
def test_one_launch_equals_two_bit_for_bit(weights, small, shape):
    B, T, L = SHAPES[shape]
    on = small if shape == "2x64-min-rows" else _run(weights, B, T, L, "1")
    off = _run(weights, B, T, L, "0")
    _assert_same_bits(on, off)


def test_both_endings_of_the_launch(weights):
    """A block whose consumer's GroupNorm is finished inside the launch ("+gnx": exchange words, the consumer's planes) and one
    whose output leaves as fp32 rows and block statistics alone: the default plan holds both kinds, DVITS_GNX_FF=0 makes every
    block the second kind.  Each plan against its own two-launch schedule."""
    B, T, L = 2, 128, 24
    on, off = _run(weights, B, T, L, "1"), _run(weights, B, T, L, "0")
    kinds = [d.split(" ")[0] for d in _c128(on["rows"])["merged"]]
    assert any("+gnx" in k for k in kinds) and "LN+GEGLU+ffproj+res" in kinds, kinds
    _assert_same_bits(on, off)
    env = {"DVITS_GNX_FF": "0"}
    on, off = _run(weights, B, T, L, "1", env), _run(weights, B, T, L, "0", env)
    kinds = [d.split(" ")[0] for d in _c128(on["rows"])["merged"]]
    assert kinds == ["LN+GEGLU+ffproj+res"] * 5, kinds
    _assert_same_bits(on, off)


def test_merged_schedule_repeats_bit_for_bit(small):
    assert len(_c128(small["rows"])["merged"]) == 5
    assert np.array_equal(small["y"][0].numpy(), small["y"][1].numpy())
    a, b = small["taps"]
    assert set(a) == set(b)
    assert not [n for n in a if not np.array_equal(a[n].numpy(), b[n].numpy())]


def test_merged_forward_against_the_oracle(weights, small):
    from oracle import unet_ref
    B, T, L = 2, 64, 24
    x, cond, enc, mask, t = _inputs(B, T, L)
    with torch.no_grad():
        y_ref = unet_ref.unet_forward(weights, oracle_cfg(KW), torch.cat([x, cond], 1), t, enc, mask)
    got = small["y"][0].numpy()
    err = rel_l2(got, y_ref.numpy())
    print("merged C = 128 chains, B=%d T=%d L=%d: rel-L2 vs oracle %.3e" % (B, T, L, err))
    assert np.isfinite(got).all()
    assert err < 2e-4, err
