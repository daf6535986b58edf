"""CPU: the trained-like generator (tests/offdist_cases.py) is pinned, and the isolated bounds of tests/test_gpu_offdist.py have teeth.

(1) severity = 0 reproduces synth.make_state_dict and the layer-wise tests' inputs bit for bit.  (2) On a reduced run (B = 2,
T = 96, L = 20: the full depth of config 1, fewer frames) the chosen profile keeps the reference inside a third of every layer-wise
bound (fp32 oracle vs fp64 oracle), keeps the floor guard, and reaches the regime: median |mean| / sigma >= 3 at a LayerNorm of
every width and a GroupNorm of every level.  (3) The fp64 restatements of parity_metrics agree with the oracle's own blocks.
(4) Faults planted in the restatements on these weights exceed the bound the GPU test derives, on all 16 transformers and all 22
resnet blocks; test_what_default_weights_hide says what severity = 0 hides and what it does not."""
import numpy as np
import pytest
import torch

import offdist_cases as oc
from conftest import UNET_CASES
from parity_metrics import (FRAME_BOUND, attn_chain_fp64, ff_tail_fp64, frame_errors, isolated_bound, proj_in_fp64, resnet_fp64,
                            resnet_input_taps)

B, T, L = 2, 96, 20
KW = UNET_CASES["cfg1"][0]
BLOCKS = ["down_blocks.0.attentions.1.", "up_blocks.2.attentions.0.", "down_blocks.2.attentions.0.", "mid_block.attentions.0."]   # C = 128, 256, 384, 512


def _case(severity):
    sd, sample, t, enc, mask = oc.case_tensors(KW, B, T, L, severity=severity)
    r32, (y64, p64) = oc.oracle_pair(KW, sd, sample, t, enc, mask)
    return {"sd": sd, "enc": enc, "mask": mask, "r32": r32, "y64": y64, "pr": p64}


@pytest.fixture(scope="module")
def trained():
    return _case(oc.PROFILES["trained"]["severity"])


@pytest.fixture(scope="module")
def default():
    return _case(0.0)


def test_severity_zero_is_make_state_dict_bit_for_bit():
    from diff_vits_amd import synth
    from diff_vits_amd.unet1d.unet_1d_condition import UNet1DConditionModel
    with torch.device("meta"):
        shapes = {k: tuple(v.shape) for k, v in UNet1DConditionModel(**KW).state_dict().items()}
    base, zero = synth.make_state_dict(shapes, seed=1234), oc.make_state_dict_trained(shapes, seed=1234, severity=0.0)
    assert list(base) == list(zero)
    for k in base:
        assert base[k].dtype == zero[k].dtype and np.array_equal(base[k].view(np.uint32), zero[k].view(np.uint32)), k
    some = oc.make_state_dict_trained(shapes, seed=1234, **oc.PROFILES["trained"])
    assert all(np.isfinite(v).all() for v in some.values())
    changed = [k for k in base if not np.array_equal(base[k], some[k])]
    assert changed and all(k.endswith(".bias") or "norm" in k for k in changed)
    g = np.concatenate([v for k, v in some.items() if k.endswith(".weight") and v.ndim == 1 and "norm" in k.split(".")[-2]])
    assert (g < 0).any() and np.abs(g).max() / np.median(np.abs(g)) > 8 and np.abs(g).max() / np.abs(g).min() > 30
    x, c, e = oc.make_inputs_trained(3, 80, 128, 50, 20, 128, severity=0.0)
    assert np.array_equal(x, synth.normal(61, "x", (3, 80, 50))) and np.array_equal(c, synth.normal(61, "c", (3, 128, 50)))
    assert np.array_equal(e, synth.normal(61, "e", (3, 20, 128)))
    assert np.array_equal(oc.make_state_dict_trained(shapes, seed=1234, **oc.PROFILES["trained"])["conv_in.bias"], some["conv_in.bias"])


def test_the_reference_alone_stays_in_bounds_and_the_regime_is_reached(trained):
    """Conditions (a), (b), (c) of the profile on the reduced run (tools/offdist_reference.py checks them at the GPU test's shapes)."""
    lines, worst = oc.reference_margins(trained["r32"][1], trained["r32"][0], trained["pr"], trained["y64"])
    fig = oc.regime_figures(trained["pr"])
    print(worst, fig["ln_by_width"], fig["gn_by_level"])
    assert worst["floored_ok"]
    assert oc.margins_ok(worst), worst
    assert oc.regime_reached(fig), (fig["ln_by_width"], fig["gn_by_level"])


def test_default_weights_do_not_reach_the_regime(default):
    fig = oc.regime_figures(default["pr"])
    assert max(fig["ln_by_width"].values()) < 0.5 and max(fig["gn_by_level"].values()) < 0.5, fig


def _stretches(c, p):
    sd, pr, tb = c["sd"], c["pr"], p + "transformer_blocks.0."
    xin = pr[p.replace("attentions", "resnets")[:-1]]
    return {
        "proj_in": (lambda **k: proj_in_fp64(sd, p, xin, 8, **k), pr[p + "proj_in"]),
        "attn1": (lambda **k: attn_chain_fp64(sd, tb, "attn1", pr[p + "proj_in"], 8, **k), pr[tb + "attn1"]),
        "attn2": (lambda **k: attn_chain_fp64(sd, tb, "attn2", pr[tb + "attn1"], 8, c["enc"], c["mask"], **k), pr[tb + "attn2"]),
        "ff": (lambda **k: ff_tail_fp64(sd, p, pr[tb + "attn2"], xin, **k), pr[p[:-1]]),
    }


@pytest.mark.parametrize("p", BLOCKS, ids=["C128", "C256", "C384", "C512"])
def test_restatements_agree_with_the_oracle_in_fp64(trained, p):
    for name, (fn, want) in _stretches(trained, p).items():
        fe = frame_errors(fn(), want)
        assert fe["floored_ok"] and fe["worst"] < 1e-12, (name, fe["worst"])
        emu = frame_errors(fn(emulate=True), want)
        assert emu["worst"] < FRAME_BOUND, (name, emu["worst"])          # the documented arithmetic itself is inside the budget here


def test_resnet_restatement_agrees_with_the_oracle_in_fp64(trained):
    sd, pr = trained["sd"], trained["pr"]
    for name in ("down_blocks.1.resnets.0", "mid_block.resnets.1", "up_blocks.1.resnets.0", "up_blocks.3.resnets.2"):
        xin, skip = resnet_input_taps()[name]
        got = resnet_fp64(sd, name + ".", pr[xin], pr["emb"], 8, skip=None if skip is None else pr[skip])
        assert frame_errors(got, pr[name])["worst"] < 1e-12, name


ALL_BLOCKS = ([("down_blocks.%d.attentions.%d." % (i, j)) for i in range(3) for j in range(2)] + ["mid_block.attentions.0."] +
              [("up_blocks.%d.attentions.%d." % (i, j)) for i in range(1, 4) for j in range(3)])
# the feed-forward tails (all at C = 128 / 256) on which the rounded-row mean moves a frame by more than FF_TAIL_BOUND
MEAN_FAULT_TAILS = ["down_blocks.0.attentions.0.", "down_blocks.0.attentions.1.", "down_blocks.1.attentions.0.", "up_blocks.2.attentions.0.",
                    "up_blocks.2.attentions.1.", "up_blocks.3.attentions.2."]


def _fault_figures(case, p, name):
    fn, _ = _stretches(case, p)[name]
    want = fn()
    return isolated_bound(fn(emulate=True), want), {f: frame_errors(fn(fault=f), want) for f in ("lost_lo", "mean_from_bf16", "beta_sign")}


@pytest.mark.parametrize("p", ALL_BLOCKS)
def test_planted_layernorm_faults_exceed_the_derived_bound(trained, p):
    """All 16 transformers.  The feed-forward tail (LayerNorm 3 folded into k_chain_ff / k_ff_split) depends on its LayerNorm in
    every one of them: a lost lo plane and beta with the wrong sign both exceed the derived bound, beta by more than 100 x.  beta
    with the wrong sign exceeds 10 x the bound on the two attention stretches as well.  The rounded-row mean is the smallest
    fault - about (|mean| / sigma) 2^-9 / sqrt(3 C) of a sigma, diluted by the residual: it exceeds the bound on the tails of
    MEAN_FAULT_TAILS (C = 128 / 256) and stays below 1e-4 at C = 384 / 512, where an error of that size is inside the bound."""
    bound, fe = _fault_figures(trained, p, "ff")
    assert fe["lost_lo"]["worst"] > bound and fe["beta_sign"]["worst"] > 100 * bound, (bound, {k: v["worst"] for k, v in fe.items()})
    if p in MEAN_FAULT_TAILS:
        assert fe["mean_from_bf16"]["worst"] > bound, (bound, fe["mean_from_bf16"]["worst"])
    for name in ("attn1", "attn2"):
        bound, fe = _fault_figures(trained, p, name)
        assert fe["beta_sign"]["worst"] > 10 * bound, (name, bound, fe["beta_sign"]["worst"])


def test_planted_groupnorm_faults_exceed_the_derived_bound(trained):
    sd, pr = trained["sd"], trained["pr"]
    for name, (xin, skip) in resnet_input_taps().items():
        fn = lambda **k: resnet_fp64(sd, name + ".", pr[xin], pr["emb"], 8, skip=None if skip is None else pr[skip], **k)   # noqa: E731
        want = fn()
        bound = isolated_bound(fn(emulate=True), want)
        for f in ("tscale",) + (("skip_stats",) if skip else ()):
            fe = frame_errors(fn(fault=f), want)
            assert fe["worst"] > 10 * bound, (name, f, fe["worst"], bound)


@pytest.mark.parametrize("p", ALL_BLOCKS)
def test_what_default_weights_hide(default, p):
    """severity = 0, all 16 transformers, stated as measured.  The rounded-row mean is invisible: below the derived bound (1e-4) on
    every stretch (at most 9.2e-5 on a frame).  A lost lo plane stays inside the layer-wise bounds - every frame below 1e-3 on all
    three stretches, the whole tensor below 2e-4 on the cross-attention stretch - which is all the old suite asked of these
    stretches outside the feed-forward launches; against the ISOLATED 1e-4 it is visible with default weights too (a frame at
    1.5e-4 ... 5.1e-4 on the self-attention stretch and the feed-forward tail): the isolated check, not the regime, is what
    catches it there."""
    for name in ("attn1", "attn2", "ff"):
        bound, fe = _fault_figures(default, p, name)
        assert fe["mean_from_bf16"]["worst"] < bound, (name, fe["mean_from_bf16"]["worst"], bound)
        assert fe["lost_lo"]["worst"] < FRAME_BOUND, (name, fe["lost_lo"]["worst"])
        if name == "attn2":
            assert fe["lost_lo"]["rel_l2"] < 2e-4, fe["lost_lo"]["rel_l2"]
