"""GPU: the C = 512 transformer block (the mid block: 8 heads of d = 64) on the column-split launches of 32-row blocks -
k_qkv_split<512, 0> (GroupNorm -> proj_in -> LN1 -> q | K fragments | V^T fragments) and k_qkv_split<512, 1> (attn1.to_out +
residual -> LN2 -> attn2.to_q), kernels_qkv.hip - with its self attention on k_attention_frag<64, ...>.

Checked here: the UNet output against the oracle at the tolerance of the engine's golden tests (2e-4 relative,
tests/test_gpu_unet.py) with the plan asserted from eng.profile_forward (a silent fall-back to one launch per GEMM proves
nothing), a level whose frame count is no multiple of the row block, a ragged prompt mask, the 64-row geometry of C <= 384
unchanged bit for bit (against the parent commit's recorded output with DVITS_QKV_SPLIT_MAX_C=384, and probe by probe between
the two schedules), bit-repeatable results, no hand-over timed out."""
import os

import numpy as np
import pytest
import torch

from conftest import UNET_CASES, oracle_cfg, rel_l2
from parity_metrics import expected_probes

pytestmark = pytest.mark.gpu

KW = UNET_CASES["cfg1"][0]          # block_out_channels (128, 256, 384, 512): the production denoiser


@pytest.fixture(scope="module")
def weights():
    from diff_vits_amd import synth
    from diff_vits_amd.unet1d.unet_1d_condition import UNet1DConditionModel
    with torch.device("meta"):
        shapes = {k: tuple(v.shape) for k, v in UNet1DConditionModel(**KW).state_dict().items()}
    return {k: torch.from_numpy(v) for k, v in synth.make_state_dict(shapes, seed=707).items()}


def _inputs(B, T, L, seed):
    from diff_vits_amd import synth
    x, cond, enc, mask = (torch.from_numpy(v) for v in synth.make_inputs(B, 80, T, L, seed=seed, ragged_mask=True))
    if B > 1:
        mask[B - 1, max(1, L - 5):] = False         # (the last utterance is one of the two the oracle checks: ragged for any B)
    t = torch.linspace(949.05, 37.0, B)
    return x, cond, enc, mask, t


def _model(sd):
    from diff_vits_amd.unet1d.unet_1d_condition import UNet1DConditionModel
    m = UNet1DConditionModel(backend="hip", **KW).eval()
    m.load_state_dict(sd)
    return m.cuda()


def _forward(m, x, cond, enc, mask, t):
    with torch.no_grad():
        y = m(torch.cat([x, cond], 1).cuda(), t.cuda(), enc.cuda(), encoder_attention_mask=mask.cuda()).sample
    torch.cuda.synchronize()
    return y


def _mid_plan(rows):
    """The C = 512 block's launches on the schedule, from the engine's per-operation table (kind, flops, ms, description)."""
    d = [r[3] for r in rows]
    return {
        "head": sum(1 for s in d if "q|Kfrag|Vfrag [8 wg / 32 rows]" in s and "C=512" in s),
        "tail": sum(1 for s in d if s.startswith("to_out+res+LN+to_q [8 wg / 32 rows]") and "C=512" in s),
        "attn64_frag": sum(1 for r in rows if r[0] == "attn" and " d=64 " in r[3] and r[3].endswith(" frag")),
        "attn64_converting": sum(1 for r in rows if r[0] == "attn" and " d=64 " in r[3] and not r[3].endswith(" frag")),
    }


SPLIT_PLAN = {"head": 1, "tail": 1, "attn64_frag": 2, "attn64_converting": 0}      # (self + cross attention on fragments)
PARENT_PLAN = {"head": 0, "tail": 0, "attn64_frag": 1, "attn64_converting": 1}


# (4, 1024): the mid level has 128 frames - 16 row blocks of 32, 128 workgroups: one round, admitted by the planner's own
#   thresholds, whole multiples of 8 row blocks (h handed over through the XCD's L2), four 32-key tiles of self attention
#   shared between the two wave halves of a query block;
# (3, 1000): 125 frames at the mid level - a padded row space of pitch 128, three padding rows in every utterance's last row
#   block and last key tile; 12 row blocks (96 workgroups, the planner's minimum): no multiple of 8, h goes through memory
@pytest.mark.parametrize("B,T,L", [(4, 1024, 40), (3, 1000, 33)], ids=["4x1024-xcd-local", "3x1000-padded-through-memory"])
def test_mid_block_on_the_split_launches_matches_the_oracle(weights, B, T, L):
    from oracle import unet_ref
    x, cond, enc, mask, t = _inputs(B, T, L, seed=71)
    m = _model(weights)
    y = _forward(m, x, cond, enc, mask, t)
    y2 = _forward(m, x, cond, enc, mask, t)
    eng = m.hip_engine()
    n_ops, bad = eng.handover_status()
    assert bad == 0 and n_ops > 0 and not eng.handover_downgraded, (n_ops, bad)
    assert torch.equal(y, y2), "two runs on the same inputs differ: arrival order entered the arithmetic"
    plan = _mid_plan(eng.profile_forward(x.cuda(), cond.cuda(), t.cuda()))
    assert plan == SPLIT_PLAN, plan
    assert eng.handover_status()[1] == 0
    pick = sorted({0, B - 1})                                # (utterances are independent through the denoiser)
    with torch.no_grad():
        y_ref = unet_ref.unet_forward(weights, oracle_cfg(KW), torch.cat([x, cond], 1)[pick], t[pick], enc[pick], mask[pick])
    got = y.cpu()[pick].numpy()
    err = rel_l2(got, y_ref.numpy())
    print("B=%d T=%d L=%d: rel-L2 vs oracle %.3e" % (B, T, L, err))
    assert np.isfinite(got).all()
    assert err < 2e-4, err


FIX_B, FIX_T, FIX_L, FIX_SEED = 8, 256, 24, 72      # levels of 256 / 128 / 64 / 32 frames: 8 row blocks at C = 384 and at C = 512
FIX_ENV = {"DVITS_QKV_SPLIT_MIN_WG": "1"}           # (the split launches forced at this small size, 64-row geometry included)


def test_knob_off_is_the_parent_schedule_bit_for_bit(weights, gold):
    """DVITS_QKV_SPLIT_MAX_C=384: the C = 512 block is back on one launch per GEMM and the converting self attention, and the
    output equals, bit for bit, what the parent commit (before the 32-row geometry existed) computed on the same inputs with
    its C = 384 / 256 blocks on the 64-row split launches: tests/golden/unet_midsplit_parent.npz, utterances 0 and 7."""
    x, cond, enc, mask, t = _inputs(FIX_B, FIX_T, FIX_L, seed=FIX_SEED)
    os.environ.update(FIX_ENV)
    os.environ["DVITS_QKV_SPLIT_MAX_C"] = "384"
    try:
        m = _model(weights)
        y = _forward(m, x, cond, enc, mask, t)
        eng = m.hip_engine()
        rows = eng.profile_forward(x.cuda(), cond.cuda(), t.cuda())
        bad = eng.handover_status()[1]
    finally:
        os.environ.pop("DVITS_QKV_SPLIT_MAX_C", None)
        for k in FIX_ENV:
            os.environ.pop(k, None)
    assert bad == 0
    assert _mid_plan(rows) == PARENT_PLAN, _mid_plan(rows)
    assert sum(1 for r in rows if r[0] == "chain" and "wg / 64 rows" in r[3] and "C=384" in r[3]) >= 10, [r[3] for r in rows if r[0] == "chain"]
    want = gold("unet_midsplit_parent.npz")["y"]
    got = y.cpu().numpy()[[0, FIX_B - 1]]
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(got, want), "max |diff| %.3e" % float(np.abs(got - want).max())


def test_c384_and_below_are_bit_identical_with_the_knob_on():
    """Two engines in one process, DVITS_QKV_SPLIT_MAX_C=384 and the default, with every intermediate kept: every probe in
    front of the C = 512 block - the down path (proj_in = h of the C <= 384 heads, attn1 = what their q / K / V fragments give,
    attn2, ff) and the mid block's first resnet - is bit-identical; the block's own probes and the output move by float32
    rounding only (same operands, same split-bf16 products; LayerNorm statistics from the fp32 rows instead of block partials,
    another summation order); the new launches repeat bit for bit."""
    from diff_vits_amd import synth
    from diff_vits_amd.unet1d.unet_1d_condition import UNet1DConditionModel
    with torch.device("meta"):
        meta = UNet1DConditionModel(**KW)
    shapes = {k: tuple(v.shape) for k, v in meta.state_dict().items()}
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(shapes, seed=707).items()}
    names = expected_probes(meta)
    before = [n for n in names if n in ("emb", "conv_in") or n.startswith("down_blocks.") or n.startswith("mid_block.resnets.0")]
    mid = [n for n in names if n.startswith("mid_block.attentions.0")]
    assert len(before) >= 40 and len(mid) == 5, (len(before), mid)
    x, cond, enc, mask, t = _inputs(FIX_B, FIX_T, FIX_L, seed=FIX_SEED)
    got, ys, plans = {}, {}, {}
    os.environ.update(FIX_ENV)
    os.environ["DVITS_KEEP_INTERMEDIATES"] = "1"
    try:
        for knob in ("384", "512"):
            os.environ["DVITS_QKV_SPLIT_MAX_C"] = knob
            m = _model(sd)
            ys[knob] = _forward(m, x, cond, enc, mask, t).cpu()
            eng = m.hip_engine()
            got[knob] = {n: eng.probe(n) for n in before + mid}
            if knob == "512":
                y2 = _forward(m, x, cond, enc, mask, t).cpu()
                assert torch.equal(y2, ys[knob])
                for n in mid:
                    assert torch.equal(eng.probe(n), got[knob][n]), "%s differs between two runs" % n
            assert eng.handover_status()[1] == 0 and not eng.handover_downgraded
            plans[knob] = _mid_plan(eng.profile_forward(x.cuda(), cond.cuda(), t.cuda()))
            del m, eng
    finally:
        os.environ.pop("DVITS_QKV_SPLIT_MAX_C", None)
        os.environ.pop("DVITS_KEEP_INTERMEDIATES", None)
        for k in FIX_ENV:
            os.environ.pop(k, None)
    assert plans["384"] == PARENT_PLAN and plans["512"] == SPLIT_PLAN, plans
    moved = [n for n in before if not torch.equal(got["384"][n], got["512"][n])]
    assert not moved, "probes in front of the C = 512 block differ between the schedules: %s" % moved[:6]
    for n in mid:
        e = rel_l2(got["512"][n].numpy(), got["384"][n].numpy())
        print("%-58s rel-L2 split vs per-GEMM %.3e" % (n, e))
        assert e < 2e-5, (n, e)
    assert rel_l2(ys["512"].numpy(), ys["384"].numpy()) < 2e-5
