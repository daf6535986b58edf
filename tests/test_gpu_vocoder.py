"""Native vocoder on the GPU: the two new kernels in isolation against fp64 of their own fp32 inputs, the whole engine per probe
and per 256-sample block against the fp64 restatement (tests/vocoder_cases.py), bitwise reproducibility, and the product call.

Figures are printed before every assertion; with DVITS_VOCODER_REPORT=<path> they are appended to that file as well (that is how
profiles/vocoder_parity.txt is produced)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import parity_metrics as pm
import vocoder_cases as vc
from diff_vits_amd import _lib, vocoder

pytestmark = pytest.mark.gpu
CFGS = {"full": vc.CFG_FULL, "small": vc.CFG_SMALL}
_cache = {}


def report(line):
    print(line)
    path = os.environ.get("DVITS_VOCODER_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def weights(name):
    if ("sd", name) not in _cache:
        _cache[("sd", name)] = vc.make_weights(CFGS[name])
    return _cache[("sd", name)]


def refs(name, case, emulate):
    """The restatement of one case (computed once, shared, never modified)."""
    key = (name, vc.case_id(case), emulate)
    if key not in _cache:
        B, T, lengths = case
        _cache[key] = vc.reference(weights(name), CFGS[name], vc.make_mel(B, T, lengths), lengths, emulate=emulate)
    return _cache[key]


def engine(name, precision="bf16x3"):
    return vocoder.Vocoder.from_state_dict(weights(name), backend="hip", precision=precision).to("cuda")


def lens(lengths):
    return torch.tensor(lengths, dtype=torch.int64, device="cuda")


# ------------------------------------------------------------------------------------------ dv_op_dwconv_ln
def dw_inputs(edge, B, T, C):
    """x [B, T, C], w [C, 1, 7], b [C] (float32) that put the convolution's OUTPUT rows at a value edge: unit; a row mean of
    30 sigma (through the bias: the taps' sums differ per channel, so an offset input would not give one); variance 0 (input
    and taps equal across the channels); sigma 1e-3 about 0.5 (variance ~ eps)."""
    g = torch.Generator().manual_seed(100 + C + T)
    x = torch.randn(B, T, C, generator=g)
    w = torch.randn(C, 1, 7, generator=g) * 7 ** -0.5
    b = 0.1 * torch.randn(C, generator=g)
    if edge == "offset30":
        b = b + 30.0
    if edge in ("constant", "small-sigma"):
        w = w[:1].expand(C, 1, 7).contiguous()
        b = torch.full((C,), 0.25)
        x = x[:, :, :1].expand(B, T, C).contiguous()
        if edge == "small-sigma":
            x = 0.5 + 1e-3 * torch.randn(B, T, C, generator=g)
    gamma = 1.0 + 0.3 * (2 * torch.rand(C, generator=g) - 1)
    beta = 0.1 * torch.randn(C, generator=g)
    return x, w, b, gamma, beta


def dw_torch(x, w, b, gamma, beta, lengths, dtype):
    out = torch.zeros(x.shape, dtype=dtype)
    for i, n in enumerate(lengths):
        if 2 <= n <= x.shape[1]:
            y = torch.nn.functional.conv1d(x[i:i + 1, :n].to(dtype).transpose(1, 2), w.to(dtype), b.to(dtype), padding=3, groups=x.shape[2])
            out[i, :n] = torch.nn.functional.layer_norm(y.transpose(1, 2), (x.shape[2],), gamma.to(dtype), beta.to(dtype), 1e-6)[0]
    return out


@pytest.mark.parametrize("C_", [512, 128])
@pytest.mark.parametrize("edge", ["unit", "offset30", "constant", "small-sigma"])
def test_dwconv_ln_op(edge, C_):
    """Every frame under 2 x the fp32 torch path's worst frame + 2^-23 of the frame's peak (max-abs per frame, both measured
    here against fp64 of the same fp32 input); padding rows exactly zero; the planes are the split of the fp32 result."""
    B, T, lengths = 3, 37, [37, 20, 2]
    x, w, b, gamma, beta = dw_inputs(edge, B, T, C_)
    want = dw_torch(x, w, b, gamma, beta, lengths, torch.float64)
    f32 = dw_torch(x, w, b, gamma, beta, lengths, torch.float32)
    d = [t.cuda().contiguous() for t in (x, w, b, gamma, beta)]
    y = torch.full((B, T, C_), float("nan"), device="cuda")
    hi = torch.zeros((B, T, C_), dtype=torch.int16, device="cuda")
    lo = torch.zeros_like(hi)
    d_len = lens(lengths)
    _lib.check(_lib.lib().dv_op_dwconv_ln(*[_lib.ptr(t) for t in d], _lib.ptr(d_len), B, T, C_, 1e-6, _lib.ptr(y), _lib.ptr(hi),
                                          _lib.ptr(lo), _lib.stream_ptr()), "dv_op_dwconv_ln")
    got = y.cpu()
    err = (got.double() - want).abs().amax(-1)
    ref_err = (f32.double() - want).abs().amax(-1)
    bound = 2.0 * float(ref_err.max()) + 2.0 ** -23 * want.abs().amax(-1)
    report("dwconv_ln %-11s C=%d: worst frame %.3e (fp32 torch %.3e, bound >= %.3e)" % (edge, C_, float(err.max()), float(ref_err.max()), float(bound.min())))
    for i, n in enumerate(lengths):
        assert float(got[i, n:].abs().sum()) == 0.0
    assert bool((err <= bound).all()), (edge, float(err.max()), float(bound.min()))
    planes = (hi.cpu().to(torch.int32) & 0xffff) << 16, (lo.cpu().to(torch.int32) & 0xffff) << 16
    joined = planes[0].view(torch.float32).double() + planes[1].view(torch.float32).double()
    assert float((joined - got.double()).abs().max()) <= 2.0 ** -16 * float(got.abs().max())


# ------------------------------------------------------------------------------------------ dv_op_istft_head
def head_logits(B, T, seed=3):
    """fp32 logits [B, T, 1026]: log-magnitudes about -2 +- 2 with entries at -20 and at 4.7 (above the clip), phases up to 50 rad."""
    g = torch.Generator().manual_seed(seed + T)
    m = -2.0 + 2.0 * torch.randn(B, T, 513, generator=g)
    m[:, :, 7::31] = -20.0
    m[:, :, 11::53] = 4.7
    p = 100.0 * torch.rand(B, T, 513, generator=g) - 50.0
    return torch.cat([m, p], -1).contiguous()


@pytest.mark.parametrize("case", [(3, 37, [37, 12, 2]), (2, 8, [8, 0]), (1, 300, [300])], ids=vc.case_id)
def test_istft_head_op(case):
    """Per 256-sample block (max-abs) under 2 x the fp32 torch.istft path's worst block + 2^-23 of the utterance's peak, against
    torch.istft in fp64 of the same fp32 logits; samples at or past n_b exactly zero; samples[b] correct."""
    B, T, lengths = case
    logits = head_logits(B, T)
    win = torch.hann_window(1024, periodic=True)
    wave = torch.full((B, (T - 1) * 256), float("nan"), device="cuda")
    samples = torch.full((B,), -1, dtype=torch.int64, device="cuda")
    d_logits, d_win, d_len = logits.cuda(), win.cuda(), lens(lengths)          # (kept alive across the call)
    _lib.check(_lib.lib().dv_op_istft_head(_lib.ptr(d_logits), _lib.ptr(d_win), _lib.ptr(d_len), B, T, _lib.ptr(wave),
                                           _lib.ptr(samples), _lib.stream_ptr()), "dv_op_istft_head")
    got = wave.cpu()
    assert samples.tolist() == [(n - 1) * 256 if 2 <= n <= T else 0 for n in lengths]
    for b, n in enumerate(lengths):
        nb = (n - 1) * 256 if 2 <= n <= T else 0
        assert float(got[b, nb:].abs().sum()) == 0.0, b
        if not nb:
            continue
        want = vc.head_to_wave(logits[b, :n].double(), win.double())
        f32 = vc.head_to_wave(logits[b, :n], win)
        err = (got[b, :nb].double() - want).abs().reshape(n - 1, 256).amax(-1)
        ref_err = (f32.double() - want).abs().reshape(n - 1, 256).amax(-1)
        peak = float(want.abs().max())
        bound = 2.0 * float(ref_err.max()) + 2.0 ** -23 * peak
        edge = np.zeros(n - 1, dtype=bool)
        edge[:2] = True
        edge[-2:] = True
        e = err.numpy()
        report("istft_head B=%d T=%d row %d (L=%d): peak %.2f; worst block %.3e (first / last two blocks %.3e, interior %.3e); fp32 torch.istft "
               "worst block %.3e; bound %.3e" % (B, T, b, n, peak, e.max(), e[edge].max(), e[~edge].max() if (~edge).any() else 0.0,
                                                  float(ref_err.max()), bound))
        assert float(err.max()) <= bound, (b, float(err.max()), bound)


# ------------------------------------------------------------------------------------------ whole engine
def run_kept(name, case, precision):
    B, T, lengths = case
    old = os.environ.get("DVITS_KEEP_INTERMEDIATES")
    os.environ["DVITS_KEEP_INTERMEDIATES"] = "1"
    try:
        v = engine(name, precision)
        wave, samples = v.decode_with_lengths(vc.make_mel(B, T, lengths).cuda(), lens(lengths))
    finally:
        if old is None:
            del os.environ["DVITS_KEEP_INTERMEDIATES"]
        else:
            os.environ["DVITS_KEEP_INTERMEDIATES"] = old
    got = {n: v.probe(n) for n in vc.probe_names(CFGS[name]["n_layers"])}
    got["wave"], got["samples"] = wave.cpu(), samples.cpu()
    return got


ENGINE_CASES = [("full", c) for c in vc.CASES] + [("small", vc.CASES[2]), ("small", vc.CASES[4])]


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
@pytest.mark.parametrize("name,case", ENGINE_CASES, ids=lambda v: v if isinstance(v, str) else vc.case_id(v))
def test_engine(name, case, precision):
    """Every probe under masked_frame_errors' criteria (2e-4 whole tensor, FRAME_BOUND per frame, localisation against 3 x the
    reference side's maximum) and the waveform per block under isolated_bound(emulation, want); bf16: both against the one-plane
    emulation (mode="bf16")."""
    B, T, lengths = case
    mode = "bf16" if precision == "bf16" else None
    want, emu = refs(name, case, False), refs(name, case, "bf16" if mode else True)
    got = run_kept(name, case, precision)
    for n in ("head", "wave"):
        if n == "wave":
            _, fig = vc.wave_failures(got[n], emu[n], want[n], lengths, T, mode)
        elif mode:
            _, fig = vc.wave_like_probe(n, got[n], emu[n], want[n], lengths, T)
        else:
            _, fig = vc.probe_failures(n, got[n], want[n], lengths, T)
        report("engine %s %s %s %s: %s" % (name, vc.case_id(case), precision, n, ", ".join("%s %.3e" % kv for kv in sorted(fig.items()))))
    fails = vc.engine_failures(got, emu, want, CFGS[name], lengths, T, mode)
    assert not fails, fails[:6]


# ------------------------------------------------------------------------------------------ bitwise
def test_two_forwards_and_replaced_utterance_bitwise():
    B, T, lengths = vc.CASES[2]
    v = engine("small")
    mel = vc.make_mel(B, T, lengths).cuda()
    a, sa = v.decode_with_lengths(mel, lens(lengths))
    b, sb = v.decode_with_lengths(mel, lens(lengths))
    assert torch.equal(a, b) and torch.equal(sa, sb)
    mel2 = mel.clone()
    mel2[1] = vc.make_mel(1, T, [T], seed=99).cuda()[0]
    c = v.decode(mel2, lens(lengths))
    assert torch.equal(c[0], a[0]) and torch.equal(c[2], a[2]) and not torch.equal(c[1], a[1])


def test_graph_replay_equals_eager():
    B, T, lengths = vc.CASES[2]
    v = engine("small")
    mel, ln = vc.make_mel(B, T, lengths).cuda(), lens(lengths)
    eager = v.decode(mel, ln).clone()
    eng = v.prepare(B, T, mel.device)
    wave = torch.zeros_like(eager)
    samples = torch.zeros(B, dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            _lib.check(_lib.lib().dv_voc_forward(eng.h, _lib.ptr(mel), _lib.ptr(ln), _lib.ptr(wave), _lib.ptr(samples), _lib.stream_ptr()), "dv_voc_forward")
    wave.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(wave, eager) and samples.tolist() == [(n - 1) * 256 for n in lengths]


@pytest.mark.parametrize("knob", ["nan", "big"])
def test_poisoned_plan_memory_changes_nothing(knob):
    B, T, lengths = vc.CASES[4]
    mel, ln = vc.make_mel(B, T, lengths).cuda(), lens(lengths)
    clean = engine("small").decode(mel, ln)
    os.environ["DVITS_POISON"] = knob
    try:
        before = _lib.lib().dv_poisoned_bytes()
        got = engine("small").decode(mel, ln)
        assert _lib.lib().dv_poisoned_bytes() > before
    finally:
        del os.environ["DVITS_POISON"]
    assert bool(torch.isfinite(got).all()) and torch.equal(got, clean)


def test_full_then_ragged_equals_fresh_ragged():
    B, T, lengths = vc.CASES[2]
    mel = vc.make_mel(B, T, lengths).cuda()
    v = engine("small")
    v.decode(mel)                                   # every row T frames: the buffers now hold values on every row
    a = v.decode(mel, lens(lengths))
    b = engine("small").decode(mel, lens(lengths))
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------ product
def test_sample_from_prior_with_the_native_vocoder(gold):
    from test_gpu_prompt import _ns2
    from test_prompt_cpu import PassThroughVocoder
    g, cfg, m, content, refer, noise = _ns2(gold)
    args = (torch.from_numpy(content).cuda(), torch.from_numpy(refer).cuda(), torch.from_numpy(g["text_lengths"]).cuda(),
            torch.from_numpy(g["spec_lengths"]).cuda())
    vcfg = dict(vc.CFG_SMALL, n_mels=m.dim)
    v = vocoder.Vocoder.from_state_dict(vc.make_weights(vcfg), backend="hip")
    T = content.shape[2]
    frames = torch.tensor([T - 3] * content.shape[0], dtype=torch.int64)
    audio, mel = m.sample_from_prior(*args, v, "unipc", noise=torch.from_numpy(noise).cuda(), frame_lengths=frames)
    assert tuple(audio.shape) == (mel.shape[0], (T - 1) * 256)
    assert torch.equal(audio, v.decode(mel, frames.cuda()))
    assert float(audio[:, (T - 4) * 256:].abs().sum()) == 0.0 and float(audio.abs().max()) > 0.0
    audio2, mel2 = m.sample_from_prior(*args, v, "unipc", noise=torch.from_numpy(noise).cuda())
    assert torch.equal(mel2, mel) and torch.equal(audio2, v.decode(mel))
    # any other object is called exactly as before
    audio3, mel3 = m.sample_from_prior(*args, PassThroughVocoder(), "unipc", noise=torch.from_numpy(noise).cuda(), frame_lengths=frames)
    assert torch.equal(mel3, mel) and tuple(audio3.shape) == (mel.shape[0], T)
    assert pm.frame_errors(audio3[:, :, None].cpu(), mel.mean(dim=1)[:, :, None].cpu())["worst"] == 0.0
