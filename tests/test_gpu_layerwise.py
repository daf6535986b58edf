"""GPU: every block of the denoiser against the oracle's intermediates, frame by frame, at the shapes whose planning puts the
hot-path kernels on the schedule (k_conv3 / k_conv3s / k_conv3u, k_qkv_split, k_chain2, k_attention_frag; k_ff_split /
k_chain_ff for the output - see the test's docstring).  The two older layer-wise tests (tests/test_gpu_unet.py) run at sizes
where the planner's own thresholds keep every level on k_gemm and compare one whole-tensor number per probe.

Criteria per probe (tests/parity_metrics.py): whole-tensor relative L2 < 2e-4 (the bar of the older layer-wise tests), EVERY
frame < 1e-3 (the project's budget for the denoiser output, BASELINE.json north_star), and the localisation ratio - worst frame /
whole tensor - below 3 x the largest ratio the reference shows against itself in fp64 (profiles/parity_localisation_ref.txt).
DVITS_PARITY_REPORT=<file> appends every probe's figures to that file (profiles/parity_localisation_hip.txt was made so)."""
import os

import numpy as np
import pytest
import torch

from conftest import UNET_CASES
from parity_metrics import (FRAME_BOUND, LOCALISATION_BOUND, describe, expected_probes, frame_errors, oracle_probes)

pytestmark = pytest.mark.gpu

CASES = [
    # the benchmark shape: every default kernel, 128-tile grids
    ("cfg1", 8, 1024, 256, {}),
    # padded row space (320 / 160 / 96 / 64 rows per utterance), the kernels forced at this small size
    ("cfg1", 3, 300, 77, {"DVITS_CONV3_MIN_TILES": "1", "DVITS_QKV_SPLIT_MIN_WG": "1", "DVITS_FF_SPLIT_MIN_WG": "1"}),
    # grids above the CU count; a prompt of two key tiles, the second almost empty
    ("cfg1", 16, 512, 33, {}),
    # one long utterance: Tq = 2048 attention
    ("cfg1", 1, 2048, 100, {}),
    # C = 100 in / out (channel padding), the flavour of config 5
    ("c100", 16, 99, 60, {}),
    # the bench shape with k_qkv_split's C = 128 instantiations (MODE 0 and MODE 2) on the schedule
    ("cfg1", 8, 1024, 256, {"DVITS_QKV_SPLIT_MIN_C": "128", "DVITS_QKV_XA_MIN_C": "128"}),
]


def _levels(T, n=4):
    out = [T]
    for _ in range(n - 1):
        out.append((out[-1] + 2 - 3) // 2 + 1)
    return out


def _pitch(t):
    return (t + 31) // 32 * 32


def _expected_plan(kw, B, T, env, n_cu):
    """What the planner (csrc/engine.hip) puts on the schedule for this shape, from its own rules:
    conv - stride-1 three-tap convolutions on the convolution kernels: the 44 of the 22 ResnetBlock2D (conv3_route: 64 x 64 tiles
      per utterance, at least DVITS_CONV3_MIN_TILES = 64 of them) + the Upsample2D ones whose target is exactly twice the source
      (128 x 64 tiles, at least 96 - or the lowered minimum);
    head / tail / xa - k_qkv_split launches of the block head (MODE 0), of the C = 384 self-attention tail (MODE 1) and of the
      C = 128 / 256 cross-attention chain (MODE 2): (rows / 64) x (C / 64) workgroups, between DVITS_QKV_SPLIT_MIN_WG = 96 and
      the CU count, C >= DVITS_QKV_SPLIT_MIN_C / DVITS_QKV_XA_MIN_C = 256, a row pitch of whole 64-row blocks (MODE 2: whole
      multiples of 8 row blocks); C = 512 keeps one launch per GEMM (chain_ok)."""
    ch = kw["block_out_channels"]
    Ts = _levels(T)
    min_tiles = int(env.get("DVITS_CONV3_MIN_TILES", 64))
    min_wg = int(env.get("DVITS_QKV_SPLIT_MIN_WG", 96))
    min_c = int(env.get("DVITS_QKV_SPLIT_MIN_C", 256))
    xa_min_c = int(env.get("DVITS_QKV_XA_MIN_C", 256))
    resnets = [(i, ch[i]) for i in range(4) for _ in range(2)] + [(3, ch[3])] * 2 + [(3 - i, ch[3 - i]) for i in range(4) for _ in range(3)]
    conv = sum(2 for lvl, c in resnets if B * (-(-_pitch(Ts[lvl]) // 64)) * (c // 64) >= min_tiles)
    for i in range(3):                                  # up_blocks.i.upsamplers.0: level 3 - i -> 2 - i, C = ch[3 - i]
        src, dst, c = Ts[3 - i], Ts[2 - i], ch[3 - i]
        if dst == 2 * src and B * (-(-_pitch(dst) // 128)) * (c // 64) >= (min_tiles if min_tiles < 64 else 96):
            conv += 1
    xformers = [(i, ch[i]) for i in range(3) for _ in range(2)] + [(3, ch[3])] + [(3 - i, ch[3 - i]) for i in range(1, 4) for _ in range(3)]
    head = tail = xa = 0
    for lvl, c in xformers:
        Tp = _pitch(Ts[lvl])
        if c not in (128, 256, 384) or B * Tp < 128 or Tp % 64 != 0:
            continue
        wg = (B * Tp // 64) * (c // 64)
        fits = min_wg <= wg <= n_cu
        head += 1 if (fits and c >= min_c) else 0
        if c == 384:
            tail += 1 if (fits and c >= min_c) else 0
        else:
            xa += 1 if (fits and c >= xa_min_c and (B * Tp // 64) % 8 == 0) else 0
    return {"conv": conv, "head": head, "tail": tail, "xa": xa}


def _plan_counts(rows):
    chain64 = [r[3] for r in rows if r[0] == "chain" and "wg / 64 rows" in r[3]]
    return {
        "conv": sum(1 for r in rows if r[0] == "gemm" and " resident" in r[3]),
        "conv_gnx": sum(1 for r in rows if r[0] == "gemm" and " resident" in r[3] and "+gnx" in r[3]),
        "head": sum(1 for d in chain64 if "q|Kfrag" in d),
        "tail": sum(1 for d in chain64 if d.startswith("to_out+res+LN+to_q (")),
        "xa": sum(1 for d in chain64 if d.startswith("to_out+res+LN+to_q+xattn+to_out+res (")),
        "chain": sum(1 for r in rows if r[0] == "chain"),
        "attn_frag": sum(1 for r in rows if r[0] == "attn" and r[3].endswith(" frag")),
        "ff_split": sum(1 for r in rows if r[0] == "chain" and r[3].startswith("LN+GEGLU+ffproj+res") and " wg / " in r[3]),
        "chain_ff": sum(1 for r in rows if r[0] == "chain" and r[3].startswith("LN+GEGLU+ffproj+res") and " wg / " not in r[3]),
    }


def _check(name, got, want, report, failures):
    fe = frame_errors(got, want)
    ratio = fe["worst"] / max(fe["rel_l2"], 1e-300)
    report.append("%-58s rel_l2 %.3e worst_frame %.3e at (%d, %d) ratio %5.2f floored %d/%d" %
                  (name, fe["rel_l2"], fe["worst"], fe["at"][0], fe["at"][1], ratio, fe["floored"], fe["frames"]))
    why = []
    if not fe["floored_ok"]:
        why.append("%d of %d reference frames sit on the norm floor" % (fe["floored"], fe["frames"]))
    if not fe["rel_l2"] < 2e-4:
        why.append("whole tensor %.2e >= 2e-4" % fe["rel_l2"])
    if not fe["worst"] < FRAME_BOUND:
        why.append("a frame at %.2e >= %.0e" % (fe["worst"], FRAME_BOUND))
    if not ratio < LOCALISATION_BOUND:
        why.append("localisation %.2f >= %.2f" % (ratio, LOCALISATION_BOUND))
    if why:
        failures.append("%s  [%s]" % (describe(name, got, want), "; ".join(why)))


@pytest.mark.parametrize("case,B,T,L,env", CASES, ids=["bench", "padded-3x300", "b16-512", "b1-2048", "c100-16x99", "bench-qkv128"])
def test_every_block_per_frame_on_the_hot_path_kernels(case, B, T, L, env):
    """One forward with DVITS_KEEP_INTERMEDIATES=1 against the oracle's intermediates of utterances 0 and B - 1 (utterances are
    independent through the denoiser; ragged prompt mask and per-utterance timestep as in
    test_convolution_kernels_outside_the_round5_window): all 132 probes of the module tree in schedule order, then the output,
    each under the three criteria of the module docstring; the first failing probes are reported with the worst frame and the
    worst 32 x C / 64 x 64 / 128 x 128 block located.

    The plan is asserted from eng.profile_forward, so that the probes are known to come from the kernels named above and not
    from k_gemm: the convolutions on the convolution kernels and the k_qkv_split launches as _expected_plan derives them from the
    shape, fragment attention on every level with 16-channel head groups, row-block chains wherever a level has 128 rows.

    DVITS_KEEP_INTERMEDIATES=1 itself changes the plan in six places (csrc/engine.hip): ff.net.2 and proj_out stay two GEMMs
    (merged_ffproj off - the `ff` probe exists only then), so k_ff_split / k_chain_ff are NOT planned; the arena reuses no
    buffer; conv1 keeps its fp32 output although its consumer's GroupNorm is finished in the launch; an up-path tensor keeps
    its fp32 copy beside the planes of the concatenated GroupNorm; the batched timestep-embedding table is off; no buffer
    shares its address with the production plan.  Here the one-launch feed-forward is therefore only checked on a second engine
    without the probes: its plan must hold the k_ff_split / k_chain_ff launches, and its OUTPUT goes through the same three
    criteria.  tests/test_gpu_tapped_schedule.py (DVITS_KEEP_INTERMEDIATES=tap) probes the production plan itself, layer by
    layer, and compares each feed-forward launch alone with an fp64 restatement."""
    from diff_vits_amd import synth
    from diff_vits_amd.unet1d.unet_1d_condition import UNet1DConditionModel
    kw = UNET_CASES[case][0]
    cx = kw["out_channels"]
    with torch.device("meta"):
        meta = UNet1DConditionModel(**kw)
    names = expected_probes(meta)
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
    assert set(names) == set(ref), set(names) ^ set(ref)
    order = list(ref)                                       # the oracle taps them in schedule order ...
    order.sort(key=lambda n: 0 if n == "emb" else (1 if n == "conv_in" else 2))   # ... except these two, filled in at the end

    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    got, plans, ys = {}, [], []
    for keep in (True, False):
        os.environ.update(env)
        if keep:
            os.environ["DVITS_KEEP_INTERMEDIATES"] = "1"
        try:
            m = UNet1DConditionModel(backend="hip", **kw).eval()
            m.load_state_dict(sd)
            m = m.cuda()
            with torch.no_grad():
                y = m(sample.cuda(), t.cuda(), enc.cuda(), encoder_attention_mask=mask.cuda()).sample
            torch.cuda.synchronize()
            eng = m.hip_engine()
            n_gnx, bad = eng.handover_status()
            assert bad == 0 and not eng.handover_downgraded
            if keep:
                for n in names:
                    try:
                        got[n] = eng.probe(n)[pick]
                    except RuntimeError as e:
                        raise AssertionError("the engine registers no probe %s: %s" % (n, e))
            plans.append((_plan_counts(eng.profile_forward(x.cuda(), cond.cuda(), t.cuda())), n_gnx))
            ys.append(y.cpu()[pick].permute(0, 2, 1).contiguous())
            del m, eng
        finally:
            os.environ.pop("DVITS_KEEP_INTERMEDIATES", None)
            for k in env:
                os.environ.pop(k, None)

    # ---- the plan: the probes (and the second engine's output) come from the hot-path kernels
    want = _expected_plan(kw, B, T, env, n_cu)
    print("plan expected %s\nplan with probes %s\nplan default %s" % (want, plans[0], plans[1]))
    assert want["conv"] >= 20, want                         # (every case has at least its two upper levels on the convolution kernels)
    for plan, n_gnx in plans:
        assert plan["conv"] >= want["conv"], (plan, want)
        assert (plan["head"], plan["tail"], plan["xa"]) == (want["head"], want["tail"], want["xa"]), (plan, want)
        if want["conv"] >= 44:                              # as test_convolution_kernels_outside_the_round5_window
            assert plan["conv_gnx"] >= 20 and n_gnx >= 40, (plan, n_gnx)
        assert plan["chain"] >= 20 and plan["attn_frag"] >= 16, plan
    assert plans[0][0]["ff_split"] == 0 and plans[0][0]["chain_ff"] == 0, plans[0]       # (see the docstring)
    min_ff_wg = int(env.get("DVITS_FF_SPLIT_MIN_WG", 96))
    ch, Ts = kw["block_out_channels"], _levels(T)
    assert plans[1][0]["chain_ff"] == 5, plans[1]           # the C = 128 blocks of the first level
    # k_ff_split: the C = 256 blocks (4 workgroups per 64-row block) from 96 workgroups
    if (B * _pitch(Ts[1]) // 64) * 4 >= min_ff_wg:
        assert plans[1][0]["ff_split"] >= 5, plans[1]

    # ---- parity, probe by probe
    report, failures = [], []
    for n in order:
        w = ref[n]
        assert tuple(got[n].shape) == tuple(w.shape), (n, tuple(got[n].shape), tuple(w.shape))
        _check(n, got[n], w, report, failures)
    want_y = y_ref.permute(0, 2, 1).contiguous()
    _check("y (with probes)", ys[0], want_y, report, failures)
    _check("y (default plan: one-launch feed-forward)", ys[1], want_y, report, failures)
    path = os.environ.get("DVITS_PARITY_REPORT")
    if path:
        with open(path, "a") as f:
            f.write("# %s B=%d T=%d L=%d %s\n%s\n" % (case, B, T, L, " ".join("%s=%s" % kv for kv in sorted(env.items())), "\n".join(report)))
    assert not failures, "%d of %d probes fail; in schedule order:\n%s" % (len(failures), len(report), "\n".join(failures[:6]))
