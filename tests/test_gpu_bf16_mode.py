"""GPU: the bf16 fast mode (precision="bf16") per stretch and per frame, against a one-plane emulation.

The mode runs the plain schedule - k_gemm<..., NSPLIT = 1> (its epilogue finishes the consumer's GroupNorm; the LayerNorm is
finished in its consumer) and k_attention<DP, NW, 1> - with ONE bf16 plane for every contraction operand and for P.  Its own
error is about 1e-2 of a tensor, so the single whole-tensor 3e-2 of test_unet_bf16_fast_mode lets a structural fault of that size pass.  Here every check is fed the engine's own
tapped input, which keeps the error from accumulating, and is bounded per frame by  2 x the worst frame of the host emulation of
that stretch + 2^-9  (parity_metrics.isolated_bound(mode="bf16"); tests/test_bf16_reference.py shows on the CPU that planted faults
exceed it).  The emulation follows csrc/attn_tile.h where it matters: q is scaled by d^-1/2 log2 e BEFORE it is rounded to its
plane, so the logits are not exact even for inputs that are; P = exp2(s - max) is rounded to bf16, the denominator is not.

(a) k_attention<DP, NW, 1>, every instantiation, through dv_op_attention_prec;  (b) the denoiser stretch by stretch on the tapped
production plan (DVITS_KEEP_INTERMEDIATES=tap: the plan of an unset variable plus copies - the `1` form plans the two-GEMM
feed-forward, which is not what production runs and not bit-equal to it);  (c) the whole output per frame against a whole-forward
one-plane emulation;  (d) the prompt encoder;  (e) poisoned memory;  (f) the sampler graph against the same loop without a graph.
DVITS_PARITY_REPORT=<file> appends the figures (profiles/bf16_mode_parity.txt was made so)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import bf16_cases as bc
import prompt_cases as pc
from parity_metrics import (BF16_FLOOR, frame_errors, isolated_bound, masked_frame_errors, one_plane, oracle_probes, prompt_oracle_probes,
                            sdpa_fp64)
from test_bf16_reference import _report
from test_gpu_unwritten_memory import _padding_zero, _penc_run, _poison_runs, _replan, _unet_eval, _unet_floor

pytestmark = pytest.mark.gpu
TENSOR_BOUND = 3e-2          # the documented whole-tensor figure of the mode (tests/test_gpu_unet.py test_unet_bf16_fast_mode)


def _L():
    from diff_vits_amd import _lib as L
    return L


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ============================================================================ (a) k_attention<DP, NW, 1>
@pytest.mark.parametrize("B,H,Tq,Tk,d,mask,qs", bc.ATTN_PLAIN_SHAPES)
def test_plain_attention_one_plane(B, H, Tq, Tk, d, mask, qs):
    """dv_op_attention_prec(DV_PREC_BF16) against fp64 scaled-dot-product attention on bf16-exact q, k, v.  Per query row: 2 x the
    worst row of the emulation + 2^-9; whole tensor: at most 2 x the emulation's relative L2 (with one valid key, or one key at
    all, both are exactly zero).  The output is pre-filled with NaN; two calls are bit-equal.  The shapes reach all 16 (DP, NW)
    pairs (tests/test_bf16_reference.py test_attention_shapes_cover_every_plain_instantiation) while the wave-count thresholds
    are launch_attention's defaults."""
    assert "DVITS_ATTN_NW8" not in os.environ and "DVITS_ATTN_NW4" not in os.environ
    L = _L()
    q, k, v, bias = bc.attention_case(B, H, Tq, Tk, d, mask, qs)
    ref = sdpa_fp64(q, k, v, H, bias)
    emu = frame_errors(sdpa_fp64(q, k, v, H, bias, emulate="bf16"), ref)
    row_bound, tensor_bound = 2.0 * emu["worst"] + BF16_FLOOR, 2.0 * emu["rel_l2"]
    dq, dk, dv, dbias = _dev(q), _dev(k), _dev(v), _dev(bias)
    outs = []
    for _ in range(2):
        o = torch.full((B, Tq, H * d), float("nan"), device="cuda")
        L.check(L.lib().dv_op_attention_prec(L.ptr(dq), L.ptr(dk), L.ptr(dv), L.ptr(dbias), L.ptr(o), B, H, Tq, Tk, d, L.PREC_BF16, None),
                "dv_op_attention_prec")
        torch.cuda.synchronize()
        outs.append(o.cpu())
    fe = frame_errors(outs[0], ref)
    _report("k_attention<%d, %d, 1> B=%d H=%d Tq=%d Tk=%d d=%d mask=%s scale=%d" % (bc.plain_instantiation(B, H, Tq, Tk, d) + (B, H, Tq, Tk, d, mask, qs)),
            ["HIP tensor %.3e worst row %.3e at %s; emulation tensor %.3e worst row %.3e; row bound %.3e tensor bound %.3e" %
             (fe["rel_l2"], fe["worst"], fe["at"], emu["rel_l2"], emu["worst"], row_bound, tensor_bound)])
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
    assert fe["rel_l2"] <= tensor_bound, (fe["rel_l2"], tensor_bound)
    assert fe["worst"] < row_bound, (fe["worst"], row_bound, fe["at"])


def test_attention_prec_is_dv_op_attention_in_parity_mode_and_refuses_other_precisions():
    L = _L()
    B, H, Tq, Tk, d = 2, 8, 33, 65, 16
    q, k, v, bias = (_dev(a) for a in bc.attention_case(B, H, Tq, Tk, d, "ragged", 1))
    a, b = (torch.full((B, Tq, H * d), float("nan"), device="cuda") for _ in range(2))
    L.check(L.lib().dv_op_attention(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(bias), L.ptr(a), B, H, Tq, Tk, d, None), "dv_op_attention")
    L.check(L.lib().dv_op_attention_prec(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(bias), L.ptr(b), B, H, Tq, Tk, d, L.PREC_BF16X3, None), "prec")
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert L.lib().dv_op_attention_prec(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(bias), L.ptr(b), B, H, Tq, Tk, d, 2, None) == -1
    assert b"precision 2 is not a DV_PREC_" in L.lib().dv_last_error()


def test_text_and_posterior_encoders_still_refuse_bf16():
    import qenc_cases as qc
    import tenc_cases as tc
    from diff_vits_amd.model3 import TextEncoder
    L = _L()
    te = TextEncoder(backend="hip", **tc.KW).eval()
    te.load_state_dict(tc.state_dict())
    eng = te.cuda().hip_engine()
    eng.sync_weights()
    assert L.lib().dv_tenc_prepare(eng._h, 2, 40, L.PREC_BF16) == -1
    assert b"DV_PREC_BF16 is unsupported by the text encoder" in L.lib().dv_last_error()
    qe = qc.make_module(backend="hip").cuda().hip_engine()
    qe.sync_weights()
    assert L.lib().dv_qenc_prepare(qe._h, 2, 40, L.PREC_BF16) == -1
    assert b"DV_PREC_BF16 is unsupported by the posterior encoder" in L.lib().dv_last_error()


# ============================================================================ (b), (c) the denoiser
def _plan_rows(eng):
    """(kind, description) of every operation of the prepared schedule: dv_unet_op_count / dv_unet_op_info, nothing is launched."""
    L = _L()
    n = C.c_int32()
    L.check(L.lib().dv_unet_op_count(eng.handle, C.byref(n)), "dv_unet_op_count")
    kind, desc, fl = C.create_string_buffer(16), C.create_string_buffer(128), C.c_double()
    rows = []
    for i in range(n.value):
        L.check(L.lib().dv_unet_op_info(eng.handle, i, kind, C.byref(fl), desc), "dv_unet_op_info")
        rows.append((kind.value.decode(), desc.value.decode()))
    return rows


def _model(sd, tap):
    from diff_vits_amd.unet1d.unet_1d_condition import UNet1DConditionModel
    if tap:
        os.environ["DVITS_KEEP_INTERMEDIATES"] = "tap"
    try:
        m = UNet1DConditionModel(backend="hip", **bc.KW).eval()
        m.load_state_dict(sd)
        m = m.cuda()
        m.hip_engine("bf16")
        return m
    finally:
        os.environ.pop("DVITS_KEEP_INTERMEDIATES", None)


def _forward(m, tap, sample, t, enc, mask, runs):
    if tap:
        os.environ["DVITS_KEEP_INTERMEDIATES"] = "tap"      # (read when the schedule is planned: at the first forward)
    try:
        with torch.no_grad():
            ys = [m(sample.cuda(), t.cuda(), enc.cuda(), encoder_attention_mask=mask.cuda()).sample.cpu() for _ in range(runs)]
        torch.cuda.synchronize()
    finally:
        os.environ.pop("DVITS_KEEP_INTERMEDIATES", None)
    eng = m.hip_engine()
    assert eng.precision == "bf16"
    return ys, _plan_rows(eng), eng.handover_status()


@pytest.fixture(scope="module")
def models():
    sd = bc.state_dict()
    return {"sd": sd, "tapped": _model(sd, True), "plain": _model(sd, False)}


@pytest.fixture(scope="module", params=range(len(bc.SHAPES)), ids=["%dx%d-L%d" % s for s in bc.SHAPES])
def run(request, models):
    B, T, L = bc.SHAPES[request.param]
    sd = models["sd"]
    sample, t, enc, mask = bc.inputs(B, T, L)
    ys, rows, ho = _forward(models["tapped"], True, sample, t, enc, mask, 2)
    eng = models["tapped"].hip_engine()
    taps = {d.split(" ")[0]: eng.probe(d.split(" ")[0]) for k, d in rows if k == "probe"}
    py, prows, pho = _forward(models["plain"], False, sample, t, enc, mask, 1)
    alone, _, _ = _forward(models["plain"], False, sample[:1], t[:1], enc[:1], mask[:1], 1)
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        y64 = oracle_probes(bc.KW, sd64, sample.double(), t.double(), enc.double(), mask)[0]
        y1 = oracle_probes(bc.KW, sd64, sample.double(), t.double(), enc.double(), mask, round_operand=one_plane)[0]
    return {"shape": (B, T, L), "sd": sd, "sample": sample, "enc": enc, "mask": mask, "ys": ys, "rows": rows, "ho": ho, "taps": taps,
            "plain_y": py[0], "plain_rows": prows, "plain_ho": pho, "alone": alone[0], "y64": y64, "y1": y1}


def test_what_ran(run):
    """The plain schedule and nothing else: no row-block chain, column-split or one-launch feed-forward operation (all of kind
    "chain"), no fragment attention, no resident-operand convolution; the 32 k_attention launches are there (the count of every kind
    goes to the report).  k_gemm's own epilogue may still finish its consumer's GroupNorm (" +gnx": gnx_setup asks for no precision),
    so hand-overs exist and none may have timed out.  The taps change neither the plan nor a bit of y; two forwards are bit-equal."""
    rows, plain = run["rows"], run["plain_rows"]
    assert [r for r in rows if r[0] != "probe"] == plain
    kinds = [k for k, _ in plain]
    assert "chain" not in kinds, [d for k, d in plain if k == "chain"][:3]
    attn = [d for k, d in plain if k == "attn"]
    assert len(attn) == 32 and not any("frag" in d for d in attn), attn[:4]
    assert not any(" resident" in d for k, d in plain if k == "gemm"), [d for k, d in plain if " resident" in d][:3]
    _report("bf16 mode, operations of the plan, cfg1 B=%d T=%d L=%d" % run["shape"], ["%s: %d" % (k, kinds.count(k)) for k in sorted(set(kinds))])
    assert len([r for r in rows if r[0] == "probe"]) > 80
    y = run["ys"][0]
    assert torch.isfinite(y).all() and torch.equal(y, run["ys"][1]) and torch.equal(y, run["plain_y"])
    assert run["ho"][1] == 0 and run["plain_ho"][1] == 0, (run["ho"], run["plain_ho"])


def test_every_stretch_against_fp64_on_the_engines_own_taps(run):
    """conv_in, every resnet block (the up path's with their concatenated skip), GroupNorm -> proj_in, norm1 -> self attention,
    norm2 -> cross attention under the ragged mask, the feed-forward tail, the three down- and the three up-samplers,
    conv_norm_out -> conv_out: the engine's tapped output against the fp64 restatement of the stretch on the engine's tapped input,
    every frame under 2 x the emulation's worst frame + 2^-9.  A failure names the first diverging stretch in schedule order."""
    B, T, L = run["shape"]
    items = bc.stretches(run["sd"], run["taps"], run["sample"], run["enc"], run["mask"], run["ys"][0], T)
    assert len(items) == 1 + 22 + 4 * 16 + 6 + 1
    order = {d.split(" ")[0]: i for i, (k, d) in enumerate(run["rows"]) if k == "probe"}
    items.sort(key=lambda it: order.get(it[0], len(run["rows"])))
    lines, failures = [], []
    for name, kind, got, fn in items:
        want, emulated = fn(False), fn("bf16")
        emu, bound = frame_errors(emulated, want), isolated_bound(emulated, want, "bf16")
        fe = frame_errors(got, want)
        lines.append("%-52s %-11s HIP tensor %.2e worst frame %.2e at %s; emulation tensor %.2e worst frame %.2e; bound %.2e" %
                     (name, kind, fe["rel_l2"], fe["worst"], fe["at"], emu["rel_l2"], emu["worst"], bound))
        if not (torch.isfinite(torch.as_tensor(got)).all() and fe["floored_ok"] and fe["worst"] < bound):
            failures.append(lines[-1])
    _report("bf16 mode, isolated stretches vs fp64, cfg1 B=%d T=%d L=%d" % (B, T, L), lines)
    assert not failures, "%d of %d stretches over their bound; first in schedule order:\n%s" % (len(failures), len(lines), "\n".join(failures[:8]))


def test_whole_output_per_frame(run):
    """y against the fp64 oracle: the tensor under the documented 3e-2, every frame under 2 x the worst frame of the whole-forward
    one-plane emulation (the factor: the emulation rounds unfolded weights and sums in another order); utterance 0 run alone agrees
    with utterance 0 inside the batch to the same per-frame bound.  (The output holds T frames per utterance and no padding rows:
    the padded row spaces are inside the plan, and test_every_stretch reads every one of them through its taps.)"""
    cl = lambda v: v.permute(0, 2, 1).contiguous()    # noqa: E731
    emu = frame_errors(cl(run["y1"]), cl(run["y64"]))
    fe = frame_errors(cl(run["ys"][0]), cl(run["y64"]))
    bound = 2.0 * emu["worst"]
    solo = frame_errors(cl(run["alone"]), cl(run["ys"][0][:1]))
    _report("bf16 mode, whole output vs fp64 oracle, cfg1 B=%d T=%d L=%d" % run["shape"],
            ["HIP tensor %.3e worst frame %.3e at %s; emulation tensor %.3e worst frame %.3e; frame bound %.3e; utterance 0 alone vs in the "
             "batch: tensor %.3e worst frame %.3e" % (fe["rel_l2"], fe["worst"], fe["at"], emu["rel_l2"], emu["worst"], bound, solo["rel_l2"],
                                                      solo["worst"])])
    assert fe["floored_ok"] and 1e-4 < fe["rel_l2"] < TENSOR_BOUND, fe["rel_l2"]
    assert fe["worst"] < bound, (fe["worst"], bound, fe["at"])
    assert run["alone"].shape == run["ys"][0][:1].shape and solo["worst"] < bound, (solo["worst"], bound, solo["at"])


# ============================================================================ (d) the prompt encoder
PENC_CASES = [("D", 3, 75, [75, 1, 50]), ("P", 2, 36, [36, 20]), ("D", 2, 300, [300, 77])]


def _penc(flavour, sd):
    from diff_vits_amd.model3 import PromptEncoder
    m = PromptEncoder(p_dropout=0.2, backend="hip", **pc.FLAVOURS[flavour][0]).eval()
    m.load_state_dict(sd)
    m = m.cuda()
    m.hip_engine().sync_weights("bf16")
    return m


@pytest.mark.parametrize("flavour,B,L,lengths", PENC_CASES, ids=["D-3x75", "P-2x36", "D-2x300"])
def test_prompt_encoder_per_frame(flavour, B, L, lengths):
    """Both flavours, ragged lengths (one set with a single-frame utterance): the output's valid frames against the fp64 oracle
    under 2 x the worst frame of its one-plane emulation (the same hook), the tensor under 3e-2, padding frames exactly zero,
    two forwards bit-equal."""
    n_layers = pc.FLAVOURS[flavour][0]["n_layers"]
    sd = pc.state_dict(flavour)
    prompt, ln = pc.inputs(flavour, B, L, lengths)
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        y64 = prompt_oracle_probes(sd64, prompt.double(), ln, n_layers)[0]
        y1 = prompt_oracle_probes(sd64, prompt.double(), ln, n_layers, round_operand=one_plane)[0]
    m = _penc(flavour, sd)
    with torch.no_grad():
        ys = [m.encode_channels_last(prompt.cuda(), ln.cuda()).cpu() for _ in range(2)]
    torch.cuda.synchronize()
    assert m.hip_engine().precision == "bf16" and torch.equal(ys[0], ys[1])
    emu = masked_frame_errors(y1, y64, lengths)
    fe = masked_frame_errors(ys[0], y64, lengths)
    bound = 2.0 * emu["worst"]
    _report("bf16 mode, prompt encoder %s B=%d L=%d lengths %s" % (flavour, B, L, lengths),
            ["HIP tensor %.3e worst frame %.3e at %s; emulation tensor %.3e worst frame %.3e; frame bound %.3e" %
             (fe["rel_l2"], fe["worst"], fe["at"], emu["rel_l2"], emu["worst"], bound)])
    assert torch.isfinite(ys[0]).all() and fe["padding_zero"], fe["first_nonzero"]
    assert 1e-4 < fe["rel_l2"] < TENSOR_BOUND, fe["rel_l2"]
    assert fe["worst"] < bound, (fe["worst"], bound, fe["at"])


# ============================================================================ (e) memory the plan never wrote
def test_denoiser_bf16_under_poison(models, monkeypatch):
    m = models["plain"]
    B, T, Lk = bc.SHAPES[0]
    sample, t, enc, mask = bc.inputs(B, T, Lk)
    cx = bc.KW["out_channels"]
    args = (sample[:, :cx].contiguous().cuda(), sample[:, cx:].contiguous().cuda(), t.cuda(), enc.cuda(), mask.cuda())
    try:
        _poison_runs("denoiser", "bf16 forward %dx%d L=%d" % (B, T, Lk), lambda: [_unet_eval(m, *args, fresh=True)], _unet_floor(B, T), monkeypatch)
        assert m.hip_engine().precision == "bf16"
    finally:
        _replan(m)


def test_prompt_encoder_bf16_under_poison(monkeypatch):
    flavour, B, L, lengths = PENC_CASES[0]
    m = _penc(flavour, pc.state_dict(flavour))
    prompt, _ = pc.inputs(flavour, B, L, lengths)

    class _Wrap:                      # (_penc_run drives Diffusion_Encoder.prompt_encoder)
        prompt_encoder = m

    floor = 2 * B * L * pc.FLAVOURS[flavour][0]["hidden_channels"] * 2
    _poison_runs("prompt", "bf16 D %dx%d ragged" % (B, L), lambda: _penc_run(_Wrap, prompt.numpy(), np.asarray(lengths, np.int64), True), floor,
                 monkeypatch, _padding_zero(lengths))
    assert m.hip_engine().precision == "bf16"


# ============================================================================ (f) the sampler
def test_sampler_graph_equals_the_same_loop_without_a_graph(models, monkeypatch):
    """Four steps of DPM-Solver++ 2M on the bf16 engine at (2, 64, 20): dv_sampler_run's captured graph, replayed, against the same
    events enqueued one by one (DVITS_NO_GRAPH=1: the same kernels on the stream) - bit-equal, finite."""
    from diff_vits_amd import synth
    from diff_vits_amd.sampler._plan import Plan
    L = _L()
    m = models["plain"]
    B, T, Lk = 2, 64, 20
    sample, _, enc, mask = bc.inputs(B, T, Lk)
    cx = bc.KW["out_channels"]
    x, cond = sample[:, :cx].contiguous().cuda(), sample[:, cx:].contiguous().cuda()

    def go(plan):
        eng = m.hip_engine()
        eng.prepare(B, T, Lk)
        eng.set_cond(enc.cuda(), m._bias_from_mask(mask.cuda(), torch.float32))
        xb, outs = x.clone(), []
        for _ in range(2):                        # (the second call on the same buffers replays the captured graph)
            xb.copy_(x)
            L.check(L.lib().dv_sampler_run(plan.handle, eng.handle, L.ptr(xb), L.ptr(cond), L.stream_ptr()), "dv_sampler_run")
            torch.cuda.synchronize()
            outs.append(xb.cpu())
        assert eng.precision == "bf16" and eng.handover_status()[1] == 0 and torch.equal(outs[0], outs[1])
        return outs[1], plan.graph_nodes()
    try:
        _replan(m)
        plan = Plan(L.SOLVER_DPMPP, synth.make_betas(), 4, 2, "time_uniform", True)
        first, nodes = go(plan)
        assert nodes > 0
        monkeypatch.setenv("DVITS_NO_GRAPH", "1")
        stepped, nodes_stepped = go(Plan(L.SOLVER_DPMPP, synth.make_betas(), 4, 2, "time_uniform", True))
        monkeypatch.delenv("DVITS_NO_GRAPH")
        assert nodes_stepped == 0, "the fresh plan captured a graph: DVITS_NO_GRAPH did not take effect"
        assert torch.isfinite(first).all() and torch.equal(first, stepped)
    finally:
        monkeypatch.delenv("DVITS_NO_GRAPH", raising=False)
        _replan(m)
