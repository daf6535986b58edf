"""GPU: layer-wise parity on the PRODUCTION schedule.  DVITS_KEEP_INTERMEDIATES=1 (tests/test_gpu_layerwise.py) changes the plan it
probes - no k_chain_ff / k_ff_split, no arena reuse, fp32 copies kept that production drops.  DVITS_KEEP_INTERMEDIATES=tap plans
exactly what an unset variable plans and appends one copy operation (kind "probe") behind the producer of every tensor that
exists on that plan; the copies land in side buffers outside the arena.

Per shape: (1) the taps change neither the plan nor one bit of y, and the plan holds the one-launch feed-forward kernels the
shape was chosen for; (2) every tap of utterances 0 and B - 1 against the oracle under the three criteria of the layer-wise
test; (3) each of the 16 feed-forward launches alone against an fp64 restatement fed the engine's own taps of its inputs."""
import os

import pytest
import torch

from conftest import UNET_CASES
from parity_metrics import FF_TAIL_BOUND, expected_probes, ff_tail_fp64, frame_errors, oracle_probes, seam_figures
from test_gpu_layerwise import _check, _levels, _pitch, _plan_counts

pytestmark = pytest.mark.gpu

CASES = {
    # pitches 320 / 160 / 96 / 64, padded rows on every level: k_chain_ff at C = 128, k_ff_split<256> on 32-row blocks (160 is no
    # multiple of 64), <384> refused (it has 64-row blocks only and 96 is no multiple of 64: the merged GEMM), <512> on 32-row blocks
    "padded-3x300": (3, 300, 77, {"DVITS_CONV3_MIN_TILES": "1", "DVITS_QKV_SPLIT_MIN_WG": "1", "DVITS_FF_SPLIT_MIN_WG": "1"}),
    # the planner's own thresholds: <256> and <384> on 64-row blocks, <512> on 32-row blocks, 128 workgroups each
    "4x1024": (4, 1024, 40, {}),
}
XF_BLOCKS = ([(i, "down_blocks.%d.attentions.%d." % (i, j)) for i in range(3) for j in range(2)] + [(3, "mid_block.attentions.0.")] +
             [(3 - i, "up_blocks.%d.attentions.%d." % (i, j)) for i in range(1, 4) for j in range(3)])


def _expected_ff(kw, B, T, env, n_cu):
    """(chain_ff, {(C, rows): launches}) as Builder::xf_ff / ff_split_rows / ff_split_supported (csrc) decide them: C = 128 on
    k_chain_ff; C = 256 / 384 / 512 on k_ff_split with 4 / 8 / 8 workgroups per row block of 64 rows - 32 at C = 512, at a pitch that
    is no multiple of 64 and where 32-row blocks still fit the CUs twice over; C = 384 has no 32-row form -, if the pitch holds
    whole row blocks and the launch has at least DVITS_FF_SPLIT_MIN_WG = 96 workgroups."""
    ch, Ts = kw["block_out_channels"], _levels(T)
    min_wg = int(env.get("DVITS_FF_SPLIT_MIN_WG", 96))
    chain_ff, split = 0, {}
    for lvl, _ in XF_BLOCKS:
        C, Tp = ch[lvl], _pitch(Ts[lvl])
        M = B * Tp
        if C == 128:
            chain_ff += 1
            continue
        nspl = 4 if C == 256 else 8
        rows = 64 if C == 384 else (32 if (C == 512 or Tp % 64) else (32 if (M // 32) * nspl * 2 <= n_cu else 64))
        if Tp % rows == 0 and (M // rows) * nspl >= min_wg:
            split[(C, rows)] = split.get((C, rows), 0) + 1
    return chain_ff, split


def _forward(kw, sd, env, tap, sample, t, enc, mask, runs):
    from diff_vits_amd.unet1d.unet_1d_condition import UNet1DConditionModel
    os.environ.update(env)
    if tap:
        os.environ["DVITS_KEEP_INTERMEDIATES"] = "tap"
    try:
        m = UNet1DConditionModel(backend="hip", **kw).eval()
        m.load_state_dict(sd)
        m = m.cuda()
        ys = []
        with torch.no_grad():
            for _ in range(runs):
                ys.append(m(sample.cuda(), t.cuda(), enc.cuda(), encoder_attention_mask=mask.cuda()).sample.cpu())
        torch.cuda.synchronize()
        eng = m.hip_engine()
        cx = kw["out_channels"]
        rows = [(r[0], r[3]) for r in eng.profile_forward(sample[:, :cx].contiguous().cuda(), sample[:, cx:].contiguous().cuda(), t.cuda())]
        torch.cuda.synchronize()
        out = {"y": ys, "rows": rows, "launches": eng.stats()[0], "flops": eng.stats()[1], "handover": eng.handover_status(),
               "downgraded": eng.handover_downgraded, "taps": {}}
        if tap:
            for kind, desc in rows:
                if kind == "probe":
                    name = desc.split(" ")[0]
                    out["taps"][name] = eng.probe(name)
        del m, eng
        return out
    finally:
        os.environ.pop("DVITS_KEEP_INTERMEDIATES", None)
        for k in env:
            os.environ.pop(k, None)


@pytest.fixture(scope="module", params=list(CASES), ids=list(CASES))
def run(request):
    """Both engines of one shape (inputs as tests/test_gpu_layerwise.py has them: cfg1 weights from synth, ragged prompt mask,
    per-utterance timestep), every tap on the host, and the oracle's intermediates of utterances 0 and B - 1."""
    from diff_vits_amd import synth
    from diff_vits_amd.unet1d.unet_1d_condition import UNet1DConditionModel
    B, T, L, env = CASES[request.param]
    kw = UNET_CASES["cfg1"][0]
    cx = kw["out_channels"]
    with torch.device("meta"):
        meta = UNet1DConditionModel(**kw)
    shapes = {k: tuple(v.shape) for k, v in meta.state_dict().items()}
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(shapes, seed=1234).items()}
    x = torch.from_numpy(synth.normal(61, "x", (B, cx, T)))
    cond = torch.from_numpy(synth.normal(61, "c", (B, kw["in_channels"] - cx, T)))
    enc = torch.from_numpy(synth.normal(61, "e", (B, L, kw["cross_attention_dim"])))
    mask = torch.ones(B, L, dtype=torch.bool)
    for b in range(B):
        mask[b, max(1, L - 3 * b):] = False
    t = torch.tensor([949.05 - 51.5 * b for b in range(B)])
    sample = torch.cat([x, cond], 1)
    pick = sorted({0, B - 1})
    with torch.no_grad():
        y_ref, ref = oracle_probes(kw, sd, sample[pick], t[pick], enc[pick], mask[pick])
    tapped = _forward(kw, sd, env, True, sample, t, enc, mask, 2)
    plain = _forward(kw, sd, env, False, sample, t, enc, mask, 1)
    return {"id": request.param, "B": B, "T": T, "L": L, "env": env, "kw": kw, "sd": sd, "names": expected_probes(meta), "pick": pick,
            "y_ref": y_ref, "ref": ref, "tapped": tapped, "plain": plain,
            "n_cu": torch.cuda.get_device_properties(0).multi_processor_count}


def _finished_in_launch(rows):
    """The conv1 names the plan marks as existing only normalised: a GEMM described "normonly" (its consumer's GroupNorm finished
    in the launch, no fp32 output, no raw planes) is the conv1 of the resnet block whose output is tapped next."""
    out, pending = [], False
    for kind, desc in rows:
        if kind == "gemm" and " normonly" in desc:
            assert not pending, desc
            pending = True
        elif kind == "probe" and ".resnets." in desc and not desc.split(" ")[0].endswith(".conv1"):
            if pending:
                out.append(desc.split(" ")[0] + ".conv1")
            pending = False
        elif kind == "probe" and desc.split(" ")[0].endswith(".conv1"):
            assert not pending, desc
    assert not pending
    return out


def test_taps_change_neither_the_plan_nor_the_arithmetic(run):
    tapped, plain = run["tapped"], run["plain"]
    taps = [d for k, d in tapped["rows"] if k == "probe"]
    assert [r for r in tapped["rows"] if r[0] != "probe"] == plain["rows"]
    assert not any(k == "probe" for k, _ in plain["rows"])
    assert len(taps) == len(tapped["taps"]) and tapped["launches"] - plain["launches"] == len(taps), (tapped["launches"], plain["launches"], len(taps))
    assert tapped["flops"] == plain["flops"]
    assert torch.equal(tapped["y"][0], plain["y"][0]) and torch.equal(tapped["y"][0], tapped["y"][1])
    for r in (tapped, plain):
        assert r["handover"][1] == 0 and not r["downgraded"], r["handover"]
    assert tapped["handover"] == plain["handover"]
    # ---- the plan under test is the one the shape was chosen for, not a fallback
    chain_ff, split = _expected_ff(run["kw"], run["B"], run["T"], run["env"], run["n_cu"])
    counts = _plan_counts([(k, 0, 0, d) for k, d in tapped["rows"]])
    got_split = {}
    for k, d in tapped["rows"]:
        if k == "chain" and d.startswith("LN+GEGLU+ffproj+res") and " wg / " in d:
            key = (int(d.split(" C=")[1]), int(d.split(" wg / ")[1].split(" ")[0]))
            got_split[key] = got_split.get(key, 0) + 1
    print("plan %s: chain_ff %d, ff_split %s (expected %d, %s), %d taps, %d launches without them" %
          (run["id"], counts["chain_ff"], got_split, chain_ff, split, len(taps), plain["launches"]))
    assert chain_ff == 5 and counts["chain_ff"] == 5, counts
    assert got_split == split and counts["ff_split"] == sum(split.values()), (got_split, split)
    if run["id"] == "padded-3x300":
        assert split == {(256, 32): 5, (512, 32): 1}, split              # <384> refused at pitch 96
    else:
        assert split == {(256, 64): 5, (384, 64): 5, (512, 32): 1}, split
        for (C, rows), _ in split.items():
            assert (run["B"] * _pitch(_levels(run["T"])[{256: 1, 384: 2, 512: 3}[C]]) // rows) * (4 if C == 256 else 8) == 128
    # ---- tensors whose fp32 copy production drops: tapped from their planes, and the plan says so
    dropped = [d for k, d in tapped["rows"] if k != "probe" and "-fp32" in d and "normonly" not in d]
    planes = [d for d in taps if d.endswith(" (planes)")]
    assert len(dropped) >= 1 and len(planes) == len(dropped), (dropped, planes)
    assert any(d.startswith("LN+GEGLU+ffproj+res+gnx-fp32") for d in dropped), dropped      # a feed-forward launch with out == nullptr


def test_every_tap_against_the_oracle(run):
    """All registered taps of utterances 0 and B - 1, in schedule order, then y: whole tensor 2e-4, every frame FRAME_BOUND, the
    localisation ratio (test_gpu_layerwise._check, unchanged)."""
    tapped, ref, pick = run["tapped"], run["ref"], run["pick"]
    order = [d.split(" ")[0] for k, d in tapped["rows"] if k == "probe"]
    assert len(set(order)) == len(order)
    # the names the production plan cannot register: the 16 `ff` (ff.net.2's output never exists: merged into proj_out) and the
    # conv1 that exist only normalised
    no_ff = [p + "transformer_blocks.0.ff" for _, p in XF_BLOCKS]
    no_conv1 = _finished_in_launch(tapped["rows"])
    assert len(no_conv1) >= 1, "no conv1 of this plan finishes its consumer's GroupNorm in the launch"
    assert set(run["names"]) - set(order) == set(no_ff) | set(no_conv1), (set(run["names"]) - set(order)) ^ (set(no_ff) | set(no_conv1))
    assert set(order) <= set(run["names"])
    present = [n for n in run["names"] if n.split(".")[-2:-1] in (["attentions"], ["resnets"], ["downsamplers"], ["upsamplers"])]
    assert len([n for n in present if ".attentions." in n]) == 16 and len([n for n in present if ".resnets." in n]) == 22 and \
        len([n for n in present if "samplers." in n]) == 6
    assert set(present) | {"conv_in", "emb"} <= set(order), (set(present) | {"conv_in", "emb"}) - set(order)
    report, failures = [], []
    for n in order:
        got = tapped["taps"][n][pick]
        assert tuple(got.shape) == tuple(ref[n].shape), (n, tuple(got.shape), tuple(ref[n].shape))
        _check(n, got, ref[n], report, failures)
    _check("y (tapped production plan)", tapped["y"][0][pick].permute(0, 2, 1).contiguous(), run["y_ref"].permute(0, 2, 1).contiguous(),
           report, failures)
    path = os.environ.get("DVITS_PARITY_REPORT")
    if path:
        with open(path, "a") as f:
            f.write("# tapped cfg1 B=%d T=%d L=%d %s\n%s\n" % (run["B"], run["T"], run["L"],
                                                             " ".join("%s=%s" % kv for kv in sorted(run["env"].items())), "\n".join(report)))
    assert not failures, "%d of %d taps fail; in schedule order:\n%s" % (len(failures), len(report), "\n".join(failures[:6]))


def test_one_launch_feed_forward_against_fp64(run):
    """Each of the 16 feed-forward launches alone: h3 (`...attn2`) and x (the resnet block before the transformer) are the
    engine's OWN taps, want = parity_metrics.ff_tail_fp64 (fp64, unmerged weights), got = the tapped `attentions.i`, every
    utterance, valid frames.  Whole tensor and every frame < 1e-4 (test_conv3's bound for one split-bf16 contraction; SURVEY
    section 7 measures about 1e-5 for one, which leaves about 10 x for two chained contractions and a LayerNorm) on the FULL
    output: tests/test_ff_tail_reference.py shows that the residual x does not hide a wrong tile from this bound.
    Measured on an MI355X (profiles/tapped_schedule_parity.txt): worst frame 5.0e-6 (k_chain_ff), 4.2e-6 / 4.3e-6 (k_ff_split<256>
    on 32 / 64 rows), 4.2e-6 (<384>), 2.8e-6 (<512>), 4.6e-6 (the merged GEMM that takes C = 384 at pitch 96)."""
    tapped, sd = run["tapped"], run["sd"]
    producer, prev = {}, None
    for k, d in tapped["rows"]:
        if k == "probe":
            producer[d.split(" ")[0]] = prev
        else:
            prev = (k, d)
    lines, failures = [], []
    for _, p in XF_BLOCKS:
        h3 = tapped["taps"][p + "transformer_blocks.0.attn2"]
        x = tapped["taps"][p.replace("attentions", "resnets")[:-1]]
        got = tapped["taps"][p[:-1]]
        assert torch.isfinite(got).all() and torch.isfinite(h3).all() and torch.isfinite(x).all(), p
        kind, desc = producer[p[:-1]]
        if kind == "chain" and " wg / " in desc:
            rows = int(desc.split(" wg / ")[1].split(" ")[0])
            kernel = "k_ff_split<%d> %d rows" % (got.shape[-1], rows)
        elif kind == "chain":
            rows, kernel = 32, "k_chain_ff 32 rows"
        else:
            rows, kernel = 64, "k_gemm (merged ffproj)"
        assert desc.startswith("LN+GEGLU+ffproj+res") or ("nseg=2" in desc and "K=%d" % (5 * got.shape[-1]) in desc), (p, desc)
        fe = frame_errors(got, ff_tail_fp64(sd, p, h3, x))
        sf = seam_figures(fe["per_frame"], rows)
        lines.append("%-30s %-24s tensor %.2e worst frame %.2e at %s; first %.2e last %.2e seams %.2e other %.2e%s" %
                     (p[:-1], kernel, fe["rel_l2"], fe["worst"], fe["at"], sf["first"], sf["last"], sf["seams"], sf["inner"],
                      "  [out as planes]" if "-fp32" in desc else ""))
        if not (fe["floored_ok"] and fe["rel_l2"] < FF_TAIL_BOUND and fe["worst"] < FF_TAIL_BOUND):
            failures.append(lines[-1])
    print("isolated feed-forward, %s (B=%d T=%d):\n%s" % (run["id"], run["B"], run["T"], "\n".join(lines)))
    path = os.environ.get("DVITS_PARITY_REPORT")
    if path:
        with open(path, "a") as f:
            f.write("# isolated feed-forward vs fp64, cfg1 B=%d T=%d L=%d\n%s\n" % (run["B"], run["T"], run["L"], "\n".join(lines)))
    assert not failures, "\n".join(failures)
