"""GPU: no output may depend on memory the plan never wrote.

Every engine runs its activations in device memory that is allocated at prepare time and not initialised (the denoiser's and the
prompt encoder's slab, the row engines' dmalloc(zero = false) buffers, the scratch of the dv_op_* entry points), and the Arena
hands a released block to any later tensor.  Two families of tests, none with a tolerance:

  poison   the same inputs on a freshly prepared schedule with DVITS_POISON unset, `big` (byte 0x4B: ~1.3e7 as fp32 and as bf16) and
           `nan` (byte 0xFF): all three outputs finite and torch.equal, the row engines' padding frames exactly zero,
           dv_poisoned_bytes() unmoved while the knob is unset, and under either fill moved by the plan's own unzeroed byte count:
           the growth of dv_unwritten_bytes() over the same run, which the library counts at every such request whether the knob is
           set or not (the slab, the sum of the unzeroed dmalloc / OpScratch requests, the sampler plan's float buffers) - "plan
           bytes", itself at least a floor worked out from the case's shape.
  history  call A, then call B on ONE prepared schedule: B equals B on a freshly prepared schedule.  A leaves the worst
           leftovers: full lengths, values x 50, other conditioning.

DVITS_PARITY_REPORT=<file> appends the table (profiles/unwritten_memory.txt was made so)."""
import os

import numpy as np
import pytest
import torch

import norm_cases as nc
import qenc_cases as qc
import tenc_cases as tc
from conftest import UNET_CASES
from diff_vits_amd import _lib as L
from diff_vits_amd import synth

pytestmark = pytest.mark.gpu

FILLS = (None, "big", "nan")
_HEAD = "%-10s %-28s %12s %12s  %s" % ("engine", "case", "floor bytes", "plan bytes", "verdict per fill")


def _report(line):
    print(line)
    path = os.environ.get("DVITS_PARITY_REPORT")
    if path:
        new = not os.path.exists(path) or os.path.getsize(path) == 0
        with open(path, "a") as f:
            f.write((_HEAD + "\n" if new else "") + line + "\n")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _normal(name, shape, std=1.0):
    return synth.normal(77, "uw." + name, shape, std=std)


def _poison_runs(engine, case, run, floor, monkeypatch, check=None):
    """run() -> list of tensors, once per fill on a fresh schedule; the assertions of the module docstring.  check(outs) holds
    what a single run must satisfy beyond finiteness (padding frames)."""
    outs, grew, plan = {}, {}, {}
    for fill in FILLS:
        if fill is None:
            monkeypatch.delenv("DVITS_POISON", raising=False)
        else:
            monkeypatch.setenv("DVITS_POISON", fill)
        before, asked = L.lib().dv_poisoned_bytes(), L.lib().dv_unwritten_bytes()
        outs[fill] = [t.detach().cpu().clone() for t in run()]
        torch.cuda.synchronize()
        grew[fill], plan[fill] = L.lib().dv_poisoned_bytes() - before, L.lib().dv_unwritten_bytes() - asked
    monkeypatch.delenv("DVITS_POISON", raising=False)
    verdict = []
    for fill in FILLS:
        finite = all(bool(torch.isfinite(t).all()) if t.is_floating_point() else True for t in outs[fill])
        same = all(torch.equal(a, b) for a, b in zip(outs[fill], outs[None]))
        verdict.append("%s: finite %s, equal %s, +%d" % (fill or "unset", finite, same, grew[fill]))
    _report("%-10s %-28s %12d %12d  %s" % (engine, case, floor, plan["big"], "; ".join(verdict)))
    assert grew[None] == 0, "the knob is unset and dv_poisoned_bytes() moved by %d" % grew[None]
    # (a handle's first prepare also packs its weights, some through unzeroed staging buffers: the three figures may differ)
    assert all(plan[f] >= floor for f in FILLS), (plan, floor)
    assert grew["big"] == plan["big"] and grew["nan"] == plan["nan"], "the fill did not cover what the plan asked for: %s of %s" % (grew, plan)
    for fill in FILLS:
        for i, (a, b) in enumerate(zip(outs[fill], outs[None])):
            if a.is_floating_point():
                assert bool(torch.isfinite(a).all()), "%s %s: output %d of the %s run is not finite" % (engine, case, i, fill or "unset")
            assert torch.equal(a, b), "%s %s: output %d of the %s run differs from the unset run" % (engine, case, i, fill)
        if check:
            check(outs[fill])
    return outs


def _padding_zero(lengths, axis_last=True):
    def check(outs):
        for i, t in enumerate(outs):
            for b, n in enumerate(lengths):
                pad = t[b, ..., int(n):] if axis_last else t[b, int(n):]
                assert not bool(pad.any()), "output %d: a padding frame of utterance %d is not zero" % (i, b)
    return check


# ============================================================================ the denoiser
def _pitch(t):
    return (t + 31) // 32 * 32


@pytest.fixture(scope="module")
def unet():
    from diff_vits_amd.unet1d.unet_1d_condition import UNet1DConditionModel
    kw = UNET_CASES["cfg1"][0]
    with torch.device("meta"):
        shapes = {k: tuple(v.shape) for k, v in UNet1DConditionModel(**kw).state_dict().items()}
    m = UNet1DConditionModel(backend="hip", **kw).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(shapes, seed=1234).items()})
    m = m.cuda()
    m.hip_engine("bf16x3")
    return m


def _unet_inputs(B, T, L, kw=UNET_CASES["cfg1"][0]):
    """As tests/test_gpu_layerwise.py: ragged prompt mask, per-utterance timestep."""
    cx = kw["out_channels"]
    x = torch.from_numpy(synth.normal(61, "x", (B, cx, T))).cuda()
    cond = torch.from_numpy(synth.normal(61, "c", (B, kw["in_channels"] - cx, T))).cuda()
    enc = torch.from_numpy(synth.normal(61, "e", (B, L, kw["cross_attention_dim"]))).cuda()
    mask = torch.ones(B, L, dtype=torch.bool)
    for b in range(B):
        mask[b, max(1, L - 3 * b):] = False
    t = torch.tensor([949.05 - 51.5 * b for b in range(B)]).cuda()
    return x, cond, t, enc, mask.cuda()


def _replan(m):
    eng = m.hip_engine()
    eng._prepared = None                                          # every cached schedule goes: the next prepare plans and allocates anew
    return eng


def _unet_eval(m, x, cond, t, enc, mask, fresh):
    eng = _replan(m) if fresh else m.hip_engine()
    eng.prepare(x.shape[0], x.shape[2], enc.shape[1])
    eng.set_cond(enc, m._bias_from_mask(mask, torch.float32))
    y = eng.eval(x, cond, t).clone()
    torch.cuda.synchronize()
    assert eng.handover_status()[1] == 0 and not eng.handover_downgraded
    return y


FIRST = (2, 37, 20)                                               # pitches 64 / 32 / 32 / 32: every level is padded
SECOND_ENV = {"DVITS_CONV3_MIN_TILES": "1", "DVITS_QKV_SPLIT_MIN_WG": "1", "DVITS_FF_SPLIT_MIN_WG": "1"}


def _unet_floor(B, T):
    return 2 * B * _pitch(T) * 128 * 4                            # the first level's residual stream and one more tensor of its size


@pytest.mark.parametrize("shape,env", [(FIRST, {}), ((3, 300, 77), SECOND_ENV)], ids=["2x37", "padded-3x300"])
def test_denoiser_forward_under_poison(unet, shape, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    args = _unet_inputs(*shape)
    try:
        _poison_runs("denoiser", "forward %dx%d L=%d" % shape, lambda: [_unet_eval(unet, *args, fresh=True)], _unet_floor(*shape[:2]),
                     monkeypatch)
        if env:
            rows = unet.hip_engine().profile_forward(*args[:3])
            kinds = " | ".join(r[3] for r in rows if r[0] == "chain")
            assert "LN+GEGLU+ffproj+res" in kinds and " wg / " in kinds, kinds     # (k_chain_xa_ff / k_ff_split are on this plan)
    finally:
        for k in env:
            monkeypatch.delenv(k, raising=False)
        _replan(unet)


def test_denoiser_taps_under_poison(unet, monkeypatch):
    """DVITS_KEEP_INTERMEDIATES=tap at the first shape: every tap of the nan run is finite on its valid frames and equal to the
    unset run's.  A failure names the first tap in schedule order: that localises the launch that read unwritten memory."""
    args = _unet_inputs(*FIRST)
    monkeypatch.setenv("DVITS_KEEP_INTERMEDIATES", "tap")
    taps = {}
    try:
        for fill in (None, "nan"):
            if fill:
                monkeypatch.setenv("DVITS_POISON", fill)
            y = _unet_eval(unet, *args, fresh=True)
            eng = unet.hip_engine()
            names = [r[3].split(" ")[0] for r in eng.profile_forward(*args[:3]) if r[0] == "probe"]
            torch.cuda.synchronize()
            taps[fill] = [("y", y.cpu())] + [(n, eng.probe(n)) for n in names]
    finally:
        monkeypatch.delenv("DVITS_POISON", raising=False)
        monkeypatch.delenv("DVITS_KEEP_INTERMEDIATES", raising=False)
        _replan(unet)
    assert len(taps[None]) > 80 and [n for n, _ in taps[None]] == [n for n, _ in taps["nan"]]
    order = list(range(1, len(taps[None]))) + [0]                  # schedule order: the output last
    bad = [taps[None][i][0] for i in order
           if not bool(torch.isfinite(taps["nan"][i][1]).all()) or not torch.equal(taps[None][i][1], taps["nan"][i][1])]
    _report("%-10s %-28s %12s %12s  %d taps, first differing: %s" % ("denoiser", "taps 2x37 (nan vs unset)", "-", "-", len(taps[None]) - 1,
                                                                    bad[0] if bad else "none"))
    assert not bad, "%d taps differ or are not finite under nan; in schedule order: %s" % (len(bad), bad[:6])


def _sample(m, x, cond, enc, mask, guided):
    from diff_vits_amd.sampler import dpm_solver
    import guidance_cases as gc
    import thresholding_cases as thc
    _replan(m)
    native = dpm_solver.NativeUNetModel(m, cond, enc, mask)
    skw = dict(steps=4, order=2, skip_type="time_uniform", method="multistep")
    if guided:
        uenc = torch.zeros_like(enc)
        solver, _, _ = gc.make_guided_solver("dpm", native, enc, uenc, 2.0, correcting_x0_fn="dynamic_thresholding",
                                             dynamic_thresholding_ratio=thc.GRAPH_THR_RATIO, thresholding_max_val=thc.GRAPH_THR_MAX)
    else:
        ns = dpm_solver.NoiseScheduleVP("discrete", betas=torch.from_numpy(synth.make_betas()))
        solver = dpm_solver.DPM_Solver(dpm_solver.model_wrapper(native, ns, model_type="x_start"), ns, algorithm_type="dpmsolver++")
    with torch.no_grad():
        out = solver.sample(x, **skw).clone()
    torch.cuda.synchronize()
    assert m.hip_engine().handover_status()[1] == 0
    return out


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guidance+thresholding"])
def test_native_sampler_under_poison(unet, guided, monkeypatch):
    """Four steps of DPM-Solver++ 2M in the captured graph at the first shape (the guided run plans the denoiser at 2 B)."""
    B, T, Lk = FIRST
    x, cond, _, enc, mask = _unet_inputs(B, T, Lk)
    try:
        _poison_runs("sampler", "4 steps " + ("cfg+thr" if guided else "plain"), lambda: [_sample(unet, x, cond, enc, mask, guided)],
                     _unet_floor(B, T), monkeypatch)
    finally:
        _replan(unet)


def _plan_run(plan, m, x, cond, enc, mask, options):
    """dv_sampler_run of `plan` on a copy of x; `options` switches thresholding + guidance (scale 2, zero unconditional states)
    + known frames on, None clears all three."""
    import thresholding_cases as thc
    B, _, T = x.shape
    eng = m.hip_engine()
    if options is None:
        plan.set_thresholding(None)
        plan.set_guidance(None)
        plan.bind_known_frames(None, None, None)
        eng.prepare(B, T, enc.shape[1])
        eng.set_cond(enc, m._bias_from_mask(mask, torch.float32))
    else:
        plan.set_thresholding((thc.GRAPH_THR_RATIO, thc.GRAPH_THR_MAX, None))
        plan.set_guidance(2.0)
        plan.bind_known_frames(*options)
        eng.prepare(2 * B, T, enc.shape[1])
        eng.set_cond(torch.cat([torch.zeros_like(enc), enc]), m._bias_from_mask(torch.cat([mask, mask]), torch.float32))
    xb = x.clone()
    L.check(L.lib().dv_sampler_run(plan.handle, eng.handle, L.ptr(xb), L.ptr(cond), L.stream_ptr()), "dv_sampler_run")
    torch.cuda.synchronize()
    assert eng.handover_status()[1] == 0
    return xb


@pytest.mark.parametrize("order", ["options-then-plain", "plain-then-options"])
def test_sampler_plan_history_on_one_plan(unet, order):
    """ONE plan object, 4 steps of DPM-Solver++ 2M: a run with thresholding + guidance + known frames, then all three cleared and a
    plain run - and the reverse.  The second run equals the same run on a fresh plan that never saw the other setting.  The first
    run's inputs are x 50, so that what it leaves in the history slots, the pair buffers and xp is large."""
    from diff_vits_amd.sampler._plan import Plan
    B, T, Lk = FIRST
    x, cond, _, enc, mask = _unet_inputs(B, T, Lk)
    known = (0.5 * torch.from_numpy(synth.normal(63, "kf.known", tuple(x.shape)))).cuda()
    eps = torch.from_numpy(synth.normal(63, "kf.eps", tuple(x.shape))).cuda()
    keep = torch.zeros(B, T, dtype=torch.uint8, device="cuda")
    keep[0, :T // 3] = 1
    keep[1, 9:T - 5] = 1
    options = (known, eps, keep)
    first, second = (options, None) if order == "options-then-plain" else (None, options)

    def new_plan():
        return Plan(L.SOLVER_DPMPP, synth.make_betas(), 4, 2, "time_uniform", True, known_frames=True)
    try:
        _replan(unet)
        want = _plan_run(new_plan(), unet, x, cond, enc, mask, second)
        plan = new_plan()
        _plan_run(plan, unet, 50.0 * x, cond, 50.0 * enc, torch.ones_like(mask), first)
        got = _plan_run(plan, unet, x, cond, enc, mask, second)
        ok = bool(torch.isfinite(got).all()) and torch.equal(got, want)
        plain = _plan_run(new_plan(), unet, x, cond, enc, mask, None if second is not None else options)
        _report("%-10s %-28s %12s %12s  equal %s" % ("sampler", "plan history " + order, "-", "-", ok))
        assert not torch.equal(want, plain), "the options changed nothing: the case tests nothing"
        assert ok, "the second run on the plan differs from the same run on a fresh plan (%s)" % order
    finally:
        _replan(unet)


def test_denoiser_history_on_one_schedule(unet):
    """A: all-valid prompt mask, enc x 50.  B: the ragged mask.  Then A with enrolled voices bound to both rows, B after rebinding
    to the plain condition."""
    x, cond, t, enc, mask = _unet_inputs(*FIRST)
    try:
        want = _unet_eval(unet, x, cond, t, enc, mask, fresh=True)
        _unet_eval(unet, 50.0 * x, cond, t, 50.0 * enc, torch.ones_like(mask), fresh=True)
        builds = unet.hip_engine().plan_builds
        got = _unet_eval(unet, x, cond, t, enc, mask, fresh=False)
        assert unet.hip_engine().plan_builds == builds
        ok = torch.equal(got, want)
        _report("%-10s %-28s %12s %12s  after full mask, enc x 50: equal %s" % ("denoiser", "history 2x37", "-", "-", ok))
        assert ok, "the forward after a call with an all-valid mask and enc x 50 differs from the fresh one"

        eng = _replan(unet)
        eng.prepare(*FIRST)
        other = 50.0 * torch.from_numpy(synth.normal(62, "e.voices", tuple(enc.shape))).cuda()
        voices = eng.enroll(other, None)
        eng.bind_voices([0, 1], voices)
        eng.eval(50.0 * x, cond, t)
        builds = eng.plan_builds
        got = _unet_eval(unet, x, cond, t, enc, mask, fresh=False)
        assert eng.plan_builds == builds
        ok = torch.equal(got, want)
        _report("%-10s %-28s %12s %12s  after bound voices: equal %s" % ("denoiser", "history 2x37 voices", "-", "-", ok))
        assert ok, "the forward after enrolled voices were bound to both rows differs from the fresh one"
    finally:
        _replan(unet)


# ============================================================================ the posterior encoder
@pytest.fixture(scope="module")
def qenc():
    return qc.make_module(backend="hip").cuda()


def _qenc_run(module, y, lengths, g, noise, fresh):
    if fresh:
        module.hip_engine()._prepared = None
    with torch.no_grad():
        z, m, logs, _ = module(_dev(y), _dev(np.asarray(lengths, np.int64)), _dev(g), noise=_dev(noise))
    torch.cuda.synchronize()
    return [z.clone(), m.clone(), logs.clone()]


@pytest.mark.parametrize("name", ["ragged", "two_bm_plus_1"])
def test_posterior_encoder_under_poison(qenc, name, monkeypatch):
    T, lengths = qc.CASES[name]
    y, ln, g, noise = qc.make_inputs(name)
    M, H, C = len(lengths) * T, qc.CFG["hidden_channels"], qc.CFG["out_channels"]
    floor = M * H * 4 * 3 + M * 2 * C * 4                          # x ping-pong, the skip sum, the projection
    _poison_runs("posterior", name + " with g", lambda: _qenc_run(qenc, y, ln, g, noise, True), floor, monkeypatch, _padding_zero(lengths))


@pytest.mark.parametrize("order", ["full-then-ragged", "ragged-then-full", "full-then-length-1"])
def test_posterior_encoder_history_on_one_schedule(qenc, order):
    """`ragged` ends its utterances 1 and 2 rows into a 64-row tile: the five-tap halo of the last valid frame lands on rows the
    full-length call filled."""
    T, lengths = qc.CASES["ragged"]
    y, _, g, noise = qc.make_inputs("ragged")
    full = ([T] * len(lengths), 50.0 * y, 50.0 * g)
    short = ([1] + lengths[1:] if order == "full-then-length-1" else lengths, y, g)
    first, second = (short, full) if order == "ragged-then-full" else (full, short)
    want = _qenc_run(qenc, second[1], second[0], second[2], noise, True)
    _qenc_run(qenc, first[1], first[0], first[2], noise, True)
    prepared = qenc.hip_engine()._prepared
    got = _qenc_run(qenc, second[1], second[0], second[2], noise, False)
    assert qenc.hip_engine()._prepared == prepared and prepared is not None
    ok = all(torch.equal(a, b) for a, b in zip(got, want))
    _report("%-10s %-28s %12s %12s  equal %s" % ("posterior", "history " + order, "-", "-", ok))
    _padding_zero(second[0])([t.cpu() for t in got])
    for k, a, b in zip(("z", "m", "logs"), got, want):
        assert torch.equal(a, b), "%s of the second call differs from the same call on a fresh schedule (%s)" % (k, order)


# ============================================================================ the text encoder
@pytest.fixture(scope="module")
def tenc():
    from diff_vits_amd.model3 import TextEncoder
    m = TextEncoder(backend="hip", **tc.KW).eval()
    m.load_state_dict(tc.state_dict())
    return m.cuda()


def _tenc_run(m, ids, ln, tone, lang, g, fresh):
    if fresh:
        m.hip_engine()._prepared = None
    with torch.no_grad():
        x, mm, logs, _ = m(ids.cuda(), ln.cuda(), tone.cuda(), lang.cuda(), g.cuda())
    torch.cuda.synchronize()
    return [x.clone(), mm.clone(), logs.clone()]


def test_text_encoder_under_poison(tenc, monkeypatch):
    _, B, T, lengths = tc.case("3x75")
    ids, tone, lang, ln, g = tc.inputs(B, T, lengths)
    floor = B * T * tc.KW["hidden_channels"] * 4 * 4                 # x, x1, y1, x2
    _poison_runs("text", "3x75 (75, 40, 9) with g", lambda: _tenc_run(tenc, ids, ln, tone, lang, g, True), floor, monkeypatch,
                 _padding_zero(lengths))


def test_text_encoder_history_on_one_schedule(tenc):
    """A: full lengths, other ids, g x 50.  B: 65 = 2 x 32 + 1, 33 = 32 + 1 and 9 tokens."""
    B, T, lengths = 3, 75, [65, 33, 9]
    ids, tone, lang, ln, g = tc.inputs(B, T, lengths)
    ids_o, tone_o, lang_o, _, g_o = tc.inputs(B, T, lengths, tag="te.other")
    want = _tenc_run(tenc, ids, ln, tone, lang, g, True)
    _tenc_run(tenc, ids_o, torch.full((B,), T, dtype=torch.int64), tone_o, lang_o, 50.0 * g_o, True)
    prepared = tenc.hip_engine()._prepared
    got = _tenc_run(tenc, ids, ln, tone, lang, g, False)
    assert tenc.hip_engine()._prepared == prepared and prepared is not None
    ok = all(torch.equal(a, b) for a, b in zip(got, want))
    _report("%-10s %-28s %12s %12s  equal %s" % ("text", "history full-then-ragged", "-", "-", ok))
    _padding_zero(lengths)([t.cpu() for t in got])
    for k, a, b in zip(("x", "m", "logs"), got, want):
        assert torch.equal(a, b), "%s of the ragged call differs from the same call on a fresh schedule" % k


# ============================================================================ the prompt encoder
@pytest.fixture(scope="module")
def penc(gold):
    from diff_vits_amd.model3 import Diffusion_Encoder
    from test_prompt_cpu import diffusion_state_dict, prompt_case
    g, kw, x, cond, prompt, lengths, t = prompt_case(gold, "cfg")
    m = Diffusion_Encoder(backend="hip", **kw).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in diffusion_state_dict(kw).items()})
    B, _, Lp = prompt.shape
    ragged = np.array([max(1, Lp - 1 - (5 * b) % Lp) for b in range(B)], np.int64)
    return m.cuda(), kw, prompt, ragged


def _penc_run(m, prompt, lengths, fresh):
    if fresh:
        m.prompt_encoder.hip_engine()._prepared = None
    with torch.no_grad():
        enc = m.prompt_encoder(_dev(prompt), _dev(lengths))
    torch.cuda.synchronize()
    return [enc.clone()]


def test_prompt_encoder_under_poison(penc, monkeypatch):
    m, kw, prompt, ragged = penc
    B, _, Lp = prompt.shape
    floor = 2 * B * Lp * kw["hidden_channels"] * 4
    _poison_runs("prompt", "cfg %dx%d ragged" % (B, Lp), lambda: _penc_run(m, prompt, ragged, True), floor, monkeypatch, _padding_zero(ragged))


def test_prompt_encoder_history_on_one_schedule(penc):
    m, kw, prompt, ragged = penc
    B, _, Lp = prompt.shape
    want = _penc_run(m, prompt, ragged, True)
    _penc_run(m, 50.0 * prompt, np.full((B,), Lp, np.int64), True)
    prepared = m.prompt_encoder.hip_engine()._prepared
    got = _penc_run(m, prompt, ragged, False)
    assert m.prompt_encoder.hip_engine()._prepared == prepared and prepared is not None
    ok = torch.equal(got[0], want[0])
    _report("%-10s %-28s %12s %12s  equal %s" % ("prompt", "history full x 50, ragged", "-", "-", ok))
    _padding_zero(ragged)([got[0].cpu()])
    assert ok, "the ragged call after a full-length prompt x 50 differs from the same call on a fresh schedule"


# ============================================================================ the mel front-end
def test_mel_history_on_one_handle():
    """A: 4 recordings of 16000 samples, amplitude x 50.  B: 2 recordings at n_max = 5000, ragged, on the same handle.  (The handle
    keeps tables only and the module allocates its output per call: nothing here can carry history by construction; the case
    pins that.)"""
    from diff_vits_amd.mel import MelSpectrogram
    big = _dev(50.0 * _normal("mel.a", (4, 16000), 0.1))
    wave, ns = _dev(_normal("mel.b", (2, 5000), 0.1)), torch.tensor([5000, 3001], device="cuda")
    outs = []
    for history in (False, True):
        mod = MelSpectrogram(backend="hip").cuda()
        if history:
            mod(big, torch.tensor([16000] * 4, device="cuda"), log=True)
        out, frames = mod(wave, ns, log=True)
        torch.cuda.synchronize()
        outs.append((out.cpu(), frames.cpu()))
    ok = torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    _report("%-10s %-28s %12s %12s  equal %s" % ("mel", "history 4x16000 x 50, 2x5000", "-", "-", ok))
    assert bool(torch.isfinite(outs[1][0]).all())
    _padding_zero(outs[1][1].tolist())([outs[1][0]])
    assert ok, "the short batch after a long loud one differs from the same batch on a fresh handle"


# ============================================================================ single operators
def _nan(shape):
    return torch.full(shape, float("nan"), device="cuda")


def _op_conv3(B, Cin, T, Tp, Cout, up2):
    rng = np.random.default_rng(7)
    x = np.empty((B, Tp, Cin), np.float32)
    x[:, :T] = _normal("c3.x", (B, T, Cin))
    x[:, T:] = (3.0e4 * rng.standard_normal((B, Tp - T, Cin))).astype(np.float32)      # (the input's own padding rows: as test_conv3)
    dx, dw, db = _dev(x), _dev(_normal("c3.w", (Cout, Cin, 3), 1.0 / np.sqrt(3 * Cin))), _dev(_normal("c3.b", (Cout,), 0.1))
    To, Tpo = (2 * T, (2 * T + 31) // 32 * 32) if up2 else (T, Tp)

    def run():
        y = _nan((B, Tpo, Cout))
        L.check(L.lib().dv_op_conv3(L.ptr(dx), L.ptr(dw), L.ptr(db), None, None, L.ptr(y), B, Cin, T, Tp, Cout, 0, up2, None), "dv_op_conv3")
        return [y[:, :To]]
    return run, 2 * B * Tp * Cin * 2


def _op_attention_frag():
    B, H, Tq, Tk, d = 2, 8, 300, 65, 16
    q, k, v = (_dev(_normal("af." + n, (B, t, H * d))) for n, t in (("q", Tq), ("k", Tk), ("v", Tk)))
    bias = np.zeros((B, Tk), np.float32)
    for b in range(B):
        bias[b, max(1, Tk - 7 * (b + 1)):] = -10000.0
    db = _dev(bias)

    def run():
        o = _nan((B, Tq, H * d))
        L.check(L.lib().dv_op_attention_frag(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(db), L.ptr(o), B, H, Tq, Tk, d, None), "dv_op_attention_frag")
        return [o]
    return run, B * Tk * 2 * H * d * 4


def _op_geglu():
    M, K, No, ldo = 130, 64, 32, 36
    dx, dw, db = _dev(_normal("gg.x", (M, K))), _dev(_normal("gg.w", (2 * No, K), K ** -0.5)), _dev(_normal("gg.b", (2 * No,), 0.1))

    def run():
        hi, lo = (torch.zeros((M, ldo), dtype=torch.int16, device="cuda") for _ in range(2))
        L.check(L.lib().dv_op_linear_planes(L.ptr(dx), L.ptr(dw), L.ptr(db), None, L.ptr(hi), L.ptr(lo), M, K, 2 * No, ldo, 1, 0, None),
                "dv_op_linear_planes")
        both = (hi[:, :No].to(torch.int32) << 16).view(torch.float32) + (lo[:, :No].to(torch.int32) << 16).view(torch.float32)
        return [hi, lo, both]
    return run, 2 * M * K * 2


def _op_gemm_fused_splitk():
    M, K, N = 130, 256, 96
    dx, dw, db = _dev(_normal("sk.x", (M, K))), _dev(_normal("sk.w", (N, K), K ** -0.5)), _dev(_normal("sk.b", (N,), 0.1))

    def run():
        y = _nan((M, N))
        L.check(L.lib().dv_op_gemm(L.ptr(dx), L.ptr(dw), L.ptr(db), None, None, L.ptr(y), None, None, M, K, N, 0, N, 0, L.GEMM_STORE, 0, 0,
                                   2 | L.GEMM_SPLITK_FUSED, L.PREC_BF16X3, None), "dv_op_gemm")
        return [y]
    return run, 2 * M * K * 2


def _op_layer_norm():
    M, C = 33, 128
    g, b = nc.affine(C)
    dx, dg, db = _dev(nc.edge_values("unit", (M, C), "uw.ln")), _dev(g), _dev(b)
    dm = _dev((np.arange(M) % 5 != 0).astype(np.float32))

    def run():
        y = _nan((M, C))
        hi, lo = (torch.zeros((M, C), dtype=torch.int16, device="cuda") for _ in range(2))
        L.check(L.lib().dv_op_layer_norm(L.ptr(dx), L.ptr(dg), L.ptr(db), L.ptr(dm), L.ptr(y), L.ptr(hi), L.ptr(lo), None, None, M, C, 1e-5,
                                         L.LN_AFFINE, None), "dv_op_layer_norm")
        return [y, hi, lo]
    return run, 0                                                  # (the entry point allocates nothing)


def _op_linear_ln():
    M, C, N = 33, 128, 96
    _, w1, b1 = nc.producer(C, False)
    g, b = nc.affine(C)
    w2, b2 = nc.consumer(N, C, False)
    d = [_dev(a) for a in (nc.edge_values("unit", (M, C), "uw.lln"), w1, b1, None, g, b, w2, b2)]

    def run():
        y1, rs, y2 = _nan((M, C)), _nan((M, C // 32, 2)), _nan((M, N))
        L.check(L.lib().dv_op_linear_ln(*[L.ptr(t) for t in d], M, C, C, N, 1, L.ptr(y1), L.ptr(rs), L.ptr(y2), None), "dv_op_linear_ln")
        return [y1, rs, y2]
    return run, 2 * M * C * 2 * 2


def _op_linear_gn():
    B, T, Tp, C, G = 2, 33, 64, 128, 8
    _, w, b = nc.producer(C, False)
    g, be = nc.affine(C)
    d = [_dev(a) for a in (nc.group_values("unit", B, T, Tp, C, G, "uw.lgn"), w, b, g, be)]

    def run():
        y = _nan((B, Tp, C))
        hi, lo = (torch.zeros((B, Tp, C), dtype=torch.int16, device="cuda") for _ in range(2))
        L.check(L.lib().dv_op_linear_gn(*[L.ptr(t) for t in d], B, T, Tp, C, C, G, 1e-5, L.GN_STAT16, L.ptr(y), None, L.ptr(hi), L.ptr(lo), None),
                "dv_op_linear_gn")
        return [y, hi, lo]
    return run, 2 * B * Tp * C * 2


OPS = {
    "conv3 (2,256,63,64,256)": lambda: _op_conv3(2, 256, 63, 64, 256, 0),
    "conv3 up2 (2,256,50,64,256)": lambda: _op_conv3(2, 256, 50, 64, 256, 1),
    "attention_frag (2,8,300,65,16)": _op_attention_frag,
    "linear_planes GEGLU 130x64x32": _op_geglu,
    "gemm fused split-K 130x256x96": _op_gemm_fused_splitk,
    "layer_norm affine 33x128": _op_layer_norm,
    "linear_ln 33x128": _op_linear_ln,
    "linear_gn stat16 33/64x128": _op_linear_gn,
}


@pytest.mark.parametrize("name", list(OPS))
def test_single_operator_under_poison(name, monkeypatch):
    run, floor = OPS[name]()
    _poison_runs("op", name, run, floor, monkeypatch)
