"""CPU: the encoders' trained-like generator (tests/offdist_enc_cases.py) is pinned, its profiles keep the reference in bounds, the
regime they reach is stated as measured, and the criteria of tests/test_gpu_offdist_enc.py have teeth on it.

(1) severity = 0 and logit gain 1 reproduce tc.state_dict() / pc.state_dict() and the layer-wise tests' inputs bit for bit; the
denoiser's trained profile (tests/offdist_cases.py) is bit for bit what it was before the encoders' names were added (a digest).
(2) On the shapes of the GPU test the chosen profiles keep the fp32 oracle inside a third of the whole-tensor and per-frame bounds
against the fp64 oracle, keep the floor cap and stay below the localisation maxima the bounds are derived from; the regime is
reached by the text encoder and, but for the row condition on one layer of either flavour, by the prompt encoder (asserted as
measured, per model over all of its layers); default weights are nowhere near it.  (3) The fp64 layer restatements agree with the oracle.  (4) Faults planted in the restatements,
every layer fed the fp64 oracle's own probe, judged by check() with the GPU test's bounds - as measured:

  fault        text encoder, trained        default            prompt encoder, trained       default
  k_lo         caught (frame 4.6e-3)        passes (6.5e-5)    caught (frame 9.9e-4 ...)     caught (2.1e-3)
  p_flush      caught (frame 1.3e-3)        passes (exact)     caught on D-2x300 (tensor)    passes (exact)
  stale_max    caught (frame 2.0e-2)        caught (4.8e-4)    - (no band term)              -
  gamma_sign   caught (frame 0.14)          caught (1.2)       caught (frame 0.46)           passes (no negative gain)
  ln_var       NOT caught (frame 4.0e-7)    passes (1.3e-7)    NOT caught (frame 9.4e-6)     passes (2.6e-7)

ln_var - the variance as E[x^2] - mean^2 in fp32 - costs about (mean / sigma)^2 2^-24 of the variance: at the |mean| / sigma of 5 - 15
this regime reaches that is 1e-6 ... 1e-5, two orders below the criteria.  It is recorded here as out of their reach, not hidden,
and nothing asserts that it stays uncaught: a test of k_ln_affine alone against fp64 would be the check that sees it (the C ABI
has no operator entry for that kernel today).  p_flush on the prompt encoder is caught on D-2x300 alone: the other three shapes
have at most 99 keys and too little weight below 2^-14 (worst frame 2.5e-5 ... 2.7e-4, inside the criteria).
The text encoder's default gamma is U(-0.1, 0.1) (synth.make_state_dict knows no `gamma` leaf), so its sign matters there too."""
import hashlib

import numpy as np
import pytest
import torch

import offdist_cases as oc
import offdist_enc_cases as ec
import prompt_cases as pc
import tenc_cases as tc
from conftest import UNET_CASES
from parity_metrics import FRAME_BOUND, PENC_LOCALISATION_BOUND

DEFAULT = dict(severity=0.0, logit_gain=1.0)
# sha256 over (name, bytes) of make_state_dict_trained(<cfg1 shapes>, seed 1234, PROFILES["trained"]), computed at the parent commit
DENOISER_TRAINED_DIGEST = "b59b60731f3c284bec3dda6e8028d44813a3961168617a646c297c81692be7f7"
PENC_FAULTS = tuple(f for f in ec.FAULTS if f != "stale_max")


def _bits_equal(a, b):
    return list(a) == list(b) and all(a[k].dtype == b[k].dtype and torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)


def test_severity_zero_and_gain_one_reproduce_the_default_cases_bit_for_bit():
    assert _bits_equal(ec.tenc_state_dict(**DEFAULT), tc.state_dict())
    for fl in pc.FLAVOURS:
        assert _bits_equal(ec.penc_state_dict(fl, **DEFAULT), pc.state_dict(fl))
    for a, b in zip(ec.tenc_inputs(3, 75, [75, 40, 9], **DEFAULT), tc.inputs(3, 75, [75, 40, 9])):
        assert torch.equal(a, b)
    for a, b in zip(ec.penc_inputs("D", 3, 75, [75, 1, 50], **DEFAULT), pc.inputs("D", 3, 75, [75, 1, 50])):
        assert torch.equal(a, b)
    # ... and the profile moves what it says it moves
    sd, base = ec.tenc_state_dict(**ec.PROFILES["tenc"]), tc.state_dict()
    changed = {k for k in base if not torch.equal(sd[k], base[k])}
    assert all(k.endswith((".bias", ".gamma", ".beta", "emb_rel_k", "emb_rel_v")) or k in ("emb.weight", "tone_emb.weight", "language_emb.weight")
               for k in changed), sorted(changed)
    assert {"emb.weight", "encoder.norm_layers_1.0.gamma", "encoder.norm_layers_2.5.beta", "encoder.attn_layers.0.conv_k.bias",
            "encoder.attn_layers.3.emb_rel_v"} <= changed
    q8 = ec.tenc_state_dict(severity=0.0, logit_gain=8.0)
    assert all(torch.equal(q8[k], base[k] * (8.0 if ".conv_q." in k else 1.0)) for k in base)
    p8, pb = ec.penc_state_dict("D", severity=0.0, logit_gain=8.0), pc.state_dict("D")
    for k in pb:
        want = pb[k].clone()
        if k.endswith("in_proj_weight"):
            want[:128] *= 8.0
        assert torch.equal(p8[k], want), k


def test_the_denoisers_trained_profile_is_what_it_was():
    from diff_vits_amd.unet1d.unet_1d_condition import UNet1DConditionModel
    with torch.device("meta"):
        shapes = {k: tuple(v.shape) for k, v in UNet1DConditionModel(**UNET_CASES["cfg1"][0]).state_dict().items()}
    h = hashlib.sha256()
    for k, v in oc.make_state_dict_trained(shapes, seed=1234, **oc.PROFILES["trained"]).items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v).tobytes())
    assert h.hexdigest() == DENOISER_TRAINED_DIGEST


def _run(engine, profile, loc_bound, faults):
    """Every case of the engine: the reference margins, the regime, and per fault the names check() fails and the worst frame."""
    out = {"worst": {"rel_l2": 0.0, "frame": 0.0, "ratio": 0.0, "floored": 0.0}, "stats": {}, "faults": {f: {} for f in (None,) + faults}}
    if engine == "tenc":
        sd = ec.tenc_state_dict(**profile)
        sd64 = {k: v.double() for k, v in sd.items()}
        cases = [(n,) + tc.case(n)[1:] for n in ec.TENC_CASES]
    else:
        cases = [(n,) + pc.case(n)[1:] for n in ec.PENC_CASES]
    for c in cases:
        if engine == "tenc":
            name, B, T, lengths = c
            ids, tone, lang, ln, g = ec.tenc_inputs(B, T, lengths, **profile)
            p32, p64 = ec.tenc_pair(sd, ids, ln, tone, lang, g)
            layers = lambda f, st=None: ec.tenc_layers(sd64, p64, ln, g, fault=f, stats=st)                      # noqa: E731
            check = lambda n, v, rep, fail: tc.check(n, v, p64[n], lengths, rep, fail, loc_bound=loc_bound)      # noqa: E731
        else:
            name, fl, B, L, lengths = c
            n_layers = pc.FLAVOURS[fl][0]["n_layers"]
            sdp = ec.penc_state_dict(fl, **profile)
            sdp64 = {k: v.double() for k, v in sdp.items()}
            prompt, ln = ec.penc_inputs(fl, B, L, lengths, **profile)
            p32, p64 = ec.penc_pair(sdp, prompt, ln, n_layers)
            layers = lambda f, st=None, a=sdp64, n=n_layers, ln=ln, p=p64: ec.penc_layers(a, p, ln, n, fault=f, stats=st)   # noqa: E731
            check = lambda n, v, rep, fail, p=p64, le=lengths: pc.check(n, v, p[n], le, rep, fail, masked=not n.endswith(".ffn1"),  # noqa: E731
                                                                        loc_bound=loc_bound)
        _, w = ec.reference_margins(p32, p64, lengths)
        for k in out["worst"]:
            out["worst"][k] = max(out["worst"][k], w[k])
        for f in (None,) + faults:
            st = {} if f is None else None
            rep, fail, worst = [], [], 0.0
            for n, v in layers(f, st).items():
                worst = max(worst, check(n, v, rep, fail)["worst"])
            out["faults"][f][name] = (len(fail), worst)
            if f is None:
                out["stats"][name] = st
    return out


@pytest.fixture(scope="module")
def runs():
    return {("tenc", "trained"): _run("tenc", ec.PROFILES["tenc"], ec.LOCALISATION_BOUND["tenc"], ec.FAULTS),
            ("tenc", "default"): _run("tenc", DEFAULT, tc.TENC_LOCALISATION_BOUND, ec.FAULTS),
            ("penc", "trained"): _run("penc", ec.PROFILES["penc"], ec.LOCALISATION_BOUND["penc"], PENC_FAULTS),
            ("penc", "default"): _run("penc", DEFAULT, PENC_LOCALISATION_BOUND, PENC_FAULTS)}


@pytest.mark.parametrize("engine", ["tenc", "penc"])
def test_the_reference_alone_stays_in_bounds_and_what_regime_is_reached(runs, engine):
    """The regime per MODEL, over all of its layers (the prompt encoder's flavours apart).  Reached: both conditions on the text
    encoder; the top-1 condition on both prompt-encoder flavours.  MISSED, as profiles/offdist_enc_reference.txt says: the row
    condition on one layer of either flavour - layer 1 of D at 2.35 (short of 3 by 0.65), layer 4 of P at 2.13 (short by 0.87);
    no point of the grid reaches it there (severity saturates: the figure is a ratio of two things that grow together)."""
    r = runs[(engine, "trained")]
    print(r["worst"])
    assert ec.margins_ok(r["worst"]), r["worst"]
    assert r["worst"]["ratio"] <= ec.LOCALISATION_REF_MAX[engine] + 0.005, r["worst"]      # the constant is the measured maximum
    regs = ec.regime_by_model(engine, r["stats"])
    print(regs)
    if engine == "tenc":
        assert regs["tenc"]["ok"] and len(regs["tenc"]["ln_per_layer"]) == 6, regs
    else:
        d, p = regs["penc-D"], regs["penc-P"]
        assert len(d["ln_per_layer"]) == 4 and len(p["ln_per_layer"]) == 6
        assert d["top1_ok"] and p["top1_ok"], regs
        assert [f >= ec.REGIME_MIN for f in d["ln_per_layer"]] == [True, False, True, True], d
        assert [f >= ec.REGIME_MIN for f in p["ln_per_layer"]] == [True, True, True, True, False, True], p
        assert 2.2 < d["ln_min"] < 2.5 and 2.0 < p["ln_min"] < 2.3, regs                   # the recorded misses
    for reg in ec.regime_by_model(engine, runs[(engine, "default")]["stats"]).values():
        assert reg["ln_min"] < 1.0 and reg["top1"] < 0.2, reg


@pytest.mark.parametrize("engine,kind", [("tenc", "trained"), ("tenc", "default"), ("penc", "trained"), ("penc", "default")])
def test_restatements_agree_with_the_oracle_in_fp64(runs, engine, kind):
    for name, (failed, worst) in runs[(engine, kind)]["faults"][None].items():
        assert failed == 0 and worst < 1e-12, (name, failed, worst)


def _caught(r, fault, every=True):
    hits = [failed > 0 for failed, _ in r["faults"][fault].values()]
    return all(hits) if every else any(hits)


def test_planted_faults_text_encoder(runs):
    tr, de = runs[("tenc", "trained")], runs[("tenc", "default")]
    for f in ("k_lo", "p_flush", "stale_max", "gamma_sign"):
        assert _caught(tr, f), (f, tr["faults"][f])                       # on both shapes
    for f in ("k_lo", "stale_max", "gamma_sign"):
        assert all(w > FRAME_BOUND for _, w in tr["faults"][f].values()), (f, tr["faults"][f])
    # default weights let the K lo plane and the flushed P through (P never gets near 2^-14 on a flat distribution: exact)
    for f in ("k_lo", "p_flush"):
        assert not _caught(de, f, every=False), (f, de["faults"][f])
    assert all(w < 1e-12 for _, w in de["faults"]["p_flush"].values())
    # ... and do NOT hide a stale maximum or gamma's sign (default gamma is U(-0.1, 0.1))
    assert _caught(de, "stale_max") and _caught(de, "gamma_sign")
    # ln_var: the recorded figures (module docstring) - the fault is real (not zero) and far smaller than any criterion here
    print("ln_var, trained / default:", tr["faults"]["ln_var"], de["faults"]["ln_var"])
    assert all(1e-9 < w for _, w in tr["faults"]["ln_var"].values())


def test_planted_faults_prompt_encoder(runs):
    tr, de = runs[("penc", "trained")], runs[("penc", "default")]
    for f in ("k_lo", "gamma_sign"):
        assert _caught(tr, f), (f, tr["faults"][f])                       # on all four shapes
    assert tr["faults"]["p_flush"]["D-2x300"][0] > 0, tr["faults"]["p_flush"]      # 300 keys: the one shape with enough weight below 2^-14
    # default weights hide the flushed P (exact) and gamma's sign (no gain is negative); the K lo plane they do not hide
    assert all(w < 1e-12 for _, w in de["faults"]["p_flush"].values()) and all(w < 1e-12 for _, w in de["faults"]["gamma_sign"].values())
    assert _caught(de, "k_lo")
    print("ln_var, trained / default:", tr["faults"]["ln_var"], de["faults"]["ln_var"])
    print("p_flush, trained:", tr["faults"]["p_flush"])
    assert all(1e-9 < w for _, w in tr["faults"]["ln_var"].values())
