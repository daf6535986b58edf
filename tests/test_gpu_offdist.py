"""GPU: the production plan on TRAINED-LIKE weight and input statistics (tests/offdist_cases.py): log-normal norm gains with
outliers and sign changes, O(1)-and-larger biases with a common offset per layer, offset and scaled inputs.  Every other GPU
parity test of the denoiser draws PyTorch-default weights and zero-mean inputs, where a LayerNorm row and a GroupNorm group have
|mean| / sigma of about 0 and the folded normalisations cancel nothing; here the median row sits at |mean| / sigma of 6 - 15
(profiles/offdist_reference.txt: the reference alone stays inside a third of every bound used below at this severity).

Two shapes, the smallest that carry every hot-path kernel (plans asserted), DVITS_KEEP_INTERMEDIATES=tap:
(1) taps change neither the plan nor a bit of y, two forwards bit-equal, hand-overs clean; (2) every tap of utterances 0 and B - 1
against the oracle under the three layer-wise criteria, unchanged; (3) every stretch of the schedule between two taps that holds a
folded normalisation - GroupNorm -> proj_in, norm1 -> self attention, norm2 -> cross attention, the feed-forward tail, every
resnet block - against an fp64 restatement (tests/parity_metrics.py) fed the engine's OWN taps, under a bound derived from the
inputs: max(FF_TAIL_BOUND, 2 x the worst frame of a host emulation of the documented arithmetic + 2^-16).
DVITS_PARITY_REPORT=<file> appends the figures (profiles/offdist_parity.txt was made so)."""
import os

import pytest
import torch

import offdist_cases as oc
from conftest import UNET_CASES
from parity_metrics import (attn_chain_fp64, expected_probes, ff_tail_fp64, frame_errors, isolated_bound, oracle_probes, proj_in_fp64,
                            resnet_fp64, resnet_input_taps)
from test_gpu_layerwise import _check, _expected_plan, _plan_counts
from test_gpu_tapped_schedule import XF_BLOCKS, _expected_ff, _finished_in_launch, _forward

pytestmark = pytest.mark.gpu
PROFILE = oc.PROFILES["trained"]


@pytest.fixture(scope="module", params=list(oc.CASES), ids=list(oc.CASES))
def run(request):
    from diff_vits_amd.unet1d.unet_1d_condition import UNet1DConditionModel
    B, T, L, env = oc.CASES[request.param]
    kw = UNET_CASES["cfg1"][0]
    with torch.device("meta"):
        meta = UNet1DConditionModel(**kw)
    sd, sample, t, enc, mask = oc.case_tensors(kw, B, T, L, **PROFILE)
    pick = sorted({0, B - 1})
    with torch.no_grad():
        y_ref, ref = oracle_probes(kw, sd, sample[pick], t[pick], enc[pick], mask[pick])
    # the regime is reached on THIS shape (condition (c) of profiles/offdist_reference.txt, here on the fp32 oracle's intermediates)
    fig = oc.regime_figures(ref)
    assert oc.regime_reached(fig), (fig["ln_by_width"], fig["gn_by_level"])
    tapped = _forward(kw, sd, env, True, sample, t, enc, mask, 2)
    plain = _forward(kw, sd, env, False, sample, t, enc, mask, 1)
    return {"id": request.param, "B": B, "T": T, "L": L, "env": env, "kw": kw, "sd": sd, "names": expected_probes(meta), "pick": pick,
            "y_ref": y_ref, "ref": ref, "tapped": tapped, "plain": plain, "enc": enc, "mask": mask,
            "n_cu": torch.cuda.get_device_properties(0).multi_processor_count}


def _report(header, lines):
    path = os.environ.get("DVITS_PARITY_REPORT")
    if path:
        with open(path, "a") as f:
            f.write("# %s\n%s\n" % (header, "\n".join(lines)))


def test_plan_and_bit_equality(run):
    tapped, plain = run["tapped"], run["plain"]
    assert [r for r in tapped["rows"] if r[0] != "probe"] == plain["rows"]
    assert torch.isfinite(tapped["y"][0]).all()
    assert torch.equal(tapped["y"][0], plain["y"][0]) and torch.equal(tapped["y"][0], tapped["y"][1])
    for r in (tapped, plain):
        assert r["handover"][1] == 0 and not r["downgraded"], r["handover"]
    chain_ff, split = _expected_ff(run["kw"], run["B"], run["T"], run["env"], run["n_cu"])
    want = _expected_plan(run["kw"], run["B"], run["T"], run["env"], run["n_cu"])
    counts = _plan_counts([(k, 0, 0, d) for k, d in tapped["rows"]])
    got_split = {}
    for k, d in tapped["rows"]:
        if k == "chain" and d.startswith("LN+GEGLU+ffproj+res") and " wg / " in d:
            key = (int(d.split(" C=")[1]), int(d.split(" wg / ")[1].split(" ")[0]))
            got_split[key] = got_split.get(key, 0) + 1
    print("plan %s: %s, ff_split %s; expected %s, chain_ff %d, %s" % (run["id"], counts, got_split, want, chain_ff, split))
    assert chain_ff == 5 and counts["chain_ff"] == 5, counts
    assert got_split == split and counts["ff_split"] == sum(split.values()), (got_split, split)
    assert (counts["head"], counts["tail"], counts["xa"]) == (want["head"], want["tail"], want["xa"]), (counts, want)
    assert counts["conv"] >= want["conv"] >= 44 and counts["attn_frag"] >= 16, (counts, want)
    if run["id"] == "padded-3x300":
        assert split == {(256, 32): 5, (512, 32): 1}, split
    else:
        assert split.get((384, 64)) == 5 and split.get((512, 32)) == 1 and sum(n for (c, _), n in split.items() if c == 256) == 5, split
        assert want["head"] >= 5 and want["tail"] == 5 and want["xa"] == 5, want


def test_every_tap_against_the_oracle(run):
    tapped, ref, pick = run["tapped"], run["ref"], run["pick"]
    order = [d.split(" ")[0] for k, d in tapped["rows"] if k == "probe"]
    no_ff = [p + "transformer_blocks.0.ff" for _, p in XF_BLOCKS]
    assert set(run["names"]) - set(order) == set(no_ff) | set(_finished_in_launch(tapped["rows"]))
    report, failures = [], []
    for n in order:
        got = tapped["taps"][n][pick]
        assert tuple(got.shape) == tuple(ref[n].shape), (n, tuple(got.shape), tuple(ref[n].shape))
        _check(n, got, ref[n], report, failures)
    _check("y (tapped production plan)", tapped["y"][0][pick].permute(0, 2, 1).contiguous(), run["y_ref"].permute(0, 2, 1).contiguous(),
           report, failures)
    print("\n".join(report))
    _report("trained-like (severity %.2f) tapped cfg1 %s B=%d T=%d L=%d" % (PROFILE["severity"], run["id"], run["B"], run["T"], run["L"]), report)
    assert not failures, "%d of %d taps fail; in schedule order:\n%s" % (len(failures), len(report), "\n".join(failures[:6]))


def _stretch(name, kind, got, fn, lines, failures):
    want, emulated = fn(False), fn(True)
    emu = frame_errors(emulated, want)
    bound = isolated_bound(emulated, want)
    fe = frame_errors(got, want)
    lines.append("%-52s %-8s HIP tensor %.2e worst frame %.2e at %s; emulation tensor %.2e worst frame %.2e; bound %.2e" %
                 (name, kind, fe["rel_l2"], fe["worst"], fe["at"], emu["rel_l2"], emu["worst"], bound))
    if not (torch.isfinite(got).all() and fe["floored_ok"] and fe["rel_l2"] < bound and fe["worst"] < bound):
        failures.append(lines[-1])


def test_each_folded_normalisation_stretch_against_fp64(run):
    """Per transformer: GroupNorm -> proj_in, norm1 -> attn1, norm2 -> attn2, the feed-forward tail; per resnet block whose input
    and output are tapped: input tap (and the concatenated skip) -> output tap.  Inputs are the engine's own taps, all utterances."""
    taps, sd, kw = run["tapped"]["taps"], run["sd"], run["kw"]
    heads, groups = kw["attention_head_dim"], kw["norm_num_groups"]
    lines, failures = [], []
    for _, p in XF_BLOCKS:
        tb = p + "transformer_blocks.0."
        x = taps[p.replace("attentions", "resnets")[:-1]]
        h, h1, h3 = taps[p + "proj_in"], taps[tb + "attn1"], taps[tb + "attn2"]
        _stretch(p + "proj_in", "GN+proj", h, lambda e: proj_in_fp64(sd, p, x, groups, emulate=e), lines, failures)
        _stretch(tb + "attn1", "LN1+sa", h1, lambda e: attn_chain_fp64(sd, tb, "attn1", h, heads, emulate=e), lines, failures)
        _stretch(tb + "attn2", "LN2+xa", h3, lambda e: attn_chain_fp64(sd, tb, "attn2", h1, heads, run["enc"], run["mask"], emulate=e), lines, failures)
        _stretch(p[:-1], "LN3+ff", taps[p[:-1]], lambda e: ff_tail_fp64(sd, p, h3, x, emulate=e), lines, failures)
    normonly = {n[:-len(".conv1")] for n in _finished_in_launch(run["tapped"]["rows"])}
    done = {"normonly": 0, "skip": 0}
    for name, (xin, skip) in resnet_input_taps().items():
        kind = "resnet" + ("+skip" if skip else "") + ("+normonly" if name in normonly else "")
        done["normonly"] += name in normonly
        done["skip"] += skip is not None
        _stretch(name, kind, taps[name], lambda e: resnet_fp64(sd, name + ".", taps[xin], taps["emb"], groups,
                                                              skip=None if skip is None else taps[skip], emulate=e), lines, failures)
    assert done["normonly"] >= 1 and done["skip"] == 12, done
    print("\n".join(lines))
    _report("trained-like (severity %.2f) isolated stretches vs fp64, cfg1 %s B=%d T=%d L=%d" % (PROFILE["severity"], run["id"], run["B"], run["T"], run["L"]), lines)
    assert not failures, "%d of %d stretches over their bound:\n%s" % (len(failures), len(lines), "\n".join(failures[:8]))
