"""GPU: the native log-mel front-end (dv_mel_forward / k_log_mel, csrc/kernels_mel.hip; mel.MelSpectrogram(backend='hip'),
tts_infer.refer_prompt / recording_mels) against the fp64 restatement of tests/mel_cases.py, under its criteria:

  linear  per frame  max_m |v - v64| / max(peak_f, clip) <= MEL_FRAME_BOUND      (profiles/mel_reference.txt: measured, 2 x max(a, b))
  log     per element |y - log(max(v64, clip))| <= MEL_FRAME_BOUND * max(peak_f, clip) / max(v64, clip) + 4 * 2^-24 * |log|   (derived)
  frames  == 1 + n // 256, every element at or past a row's frames exactly 0.

The torch path on the GPU (rocFFT) runs on the same rows, its figure is printed beside the kernel's and held to the same bound.
Bitwise: a ragged batch's rows equal the B = 1 calls, two calls agree, NaN behind every row's samples changes no bit (a read past a row's
end cannot pass that), guard words around the outputs stay intact, one capture-and-replay equals the eager call.  Product surface:
refer_prompt and recording_mels -> VITS.align on both backends.  DVITS_PARITY_REPORT=<file> appends the figures
(profiles/mel_parity.txt was made so)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mel_cases as mc
from conftest import rel_l2
from diff_vits_amd import _lib, tts_infer
from diff_vits_amd.mel import MelSpectrogram

pytestmark = pytest.mark.gpu

_REF, _MODS = {}, {}


def reference(name, power=1):
    key = (name, power)
    if key not in _REF:
        case = mc.CASES[name]
        window, fb = mc.tables(case["mel_kw"])
        wave = mc.make_wave(case)
        v64, frames = mc.restate64(wave, case["n"], window, fb, power)
        for a in (v64, frames):
            a.setflags(write=False)
        _REF[key] = (wave, v64, frames)
    return _REF[key]


def module(name, power=1, backend="hip"):
    key = (tuple(sorted(mc.CASES[name]["mel_kw"].items())), power, backend)
    if key not in _MODS:
        _MODS[key] = MelSpectrogram(power=float(power), backend=backend, **mc.CASES[name]["mel_kw"]).cuda()
    return _MODS[key]


def run(name, power=1, log=False, backend="hip", wave=None):
    case = mc.CASES[name]
    wave = reference(name, power)[0] if wave is None else wave
    out, frames = module(name, power, backend)(torch.from_numpy(wave).cuda(), torch.tensor(case["n"], device="cuda"), log=log)
    torch.cuda.synchronize()
    return out.cpu().numpy(), frames.cpu().numpy()


def _report(line):
    print(line)
    path = os.environ.get("DVITS_PARITY_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


PARITY = [(n, 1) for n in mc.CASES] + [(n, 2) for n in mc.POWER2_CASES]


@pytest.mark.parametrize("log", [False, True], ids=["linear", "log"])
@pytest.mark.parametrize("name,power", PARITY)
def test_against_the_fp64_restatement(name, power, log):
    case = mc.CASES[name]
    wave, v64, frames = reference(name, power)
    got, fr = run(name, power, log)
    ref, rfr = run(name, power, log, backend=None)
    fig = (lambda o: mc.log_error(o, v64, frames)) if log else (lambda o: mc.linear_error(o, v64, frames))
    unit = "of its tolerance" if log else "(bound %.1e)" % mc.MEL_FRAME_BOUND
    _report("%-18s power %d %-6s k_log_mel %.3e  torch/rocFFT %.3e  %s" % (name, power, "log" if log else "linear", fig(got), fig(ref), unit))
    assert mc.check(case, got, fr, v64, log) == []
    assert mc.check(case, ref, rfr, v64, log) == [], "the torch path on the GPU"


def test_zeros_and_closed_forms():
    for name in ("zeros_n513", "zeros_n2048"):
        lin, fr = run(name)
        log, _ = run(name, log=True)
        assert not lin.any()
        want = np.log(np.float64(np.float32(1e-7)))
        assert float(np.abs(log[0, :, :int(fr[0])] - want).max()) <= 2.0 ** -22 * abs(want)


@pytest.mark.parametrize("name", ["ragged4096", "ragged5000"])
def test_bitwise_rows_repeats_and_nan_tail(name):
    case = mc.CASES[name]
    wave = reference(name)[0]
    for log in (False, True):
        got, fr = run(name, log=log)
        again, fr2 = run(name, log=log)
        assert np.array_equal(got.view(np.uint32), again.view(np.uint32)) and np.array_equal(fr, fr2)
        m = module(name)
        for b, n in enumerate(case["n"]):
            alone, f1 = m(torch.from_numpy(wave[b:b + 1, :n].copy()).cuda(), torch.tensor([n], device="cuda"), log=log)
            assert int(f1[0]) == int(fr[b])
            assert np.array_equal(got[b, :, :int(fr[b])].view(np.uint32), alone[0].cpu().numpy().view(np.uint32)), (b, n)
        poisoned, fr3 = run(name, log=log, wave=mc.make_wave(case, fill=np.nan))
        assert np.all(np.isfinite(poisoned)) and np.array_equal(fr, fr3)
        assert np.array_equal(got.view(np.uint32), poisoned.view(np.uint32))


def test_no_write_outside_the_result():
    name = "ragged5000"
    case = mc.CASES[name]
    want, wfr = run(name, log=True)
    m = module(name)
    B, n_max = len(case["n"]), case["n_max"]
    L_max, G = 1 + n_max // mc.HOP, 1024
    n_out = B * 100 * L_max
    buf = torch.full((G + n_out + G,), 12345.0, device="cuda")
    fbuf = torch.full((16 + B + 16,), -77, dtype=torch.int64, device="cuda")
    wave = torch.from_numpy(reference(name)[0]).cuda()
    n = torch.tensor(case["n"], device="cuda")
    rc = _lib.lib().dv_mel_forward(m._hip.h, _lib.ptr(wave), _lib.ptr(n), B, n_max, C.c_void_p(buf.data_ptr() + 4 * G),
                                   C.c_void_p(fbuf.data_ptr() + 8 * 16), L_max, _lib.MEL_LOG, _lib.stream_ptr())
    _lib.check(rc, "dv_mel_forward")
    torch.cuda.synchronize()
    assert bool((buf[:G] == 12345.0).all()) and bool((buf[G + n_out:] == 12345.0).all())
    assert bool((fbuf[:16] == -77).all()) and bool((fbuf[16 + B:] == -77).all())
    assert np.array_equal(buf[G:G + n_out].cpu().numpy().reshape(want.shape).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(fbuf[16:16 + B].cpu().numpy(), wfr)


def test_capture_and_replay_on_the_current_stream():
    name = "ragged4096"
    case = mc.CASES[name]
    want, wfr = run(name, log=True)
    m = module(name)
    wave = torch.from_numpy(reference(name)[0]).cuda()
    n = torch.tensor(case["n"], device="cuda")
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):          # one kernel node: a linear graph
        out, frames = m(wave, n, validate=False, log=True)
    out.zero_()
    frames.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)) and np.array_equal(frames.cpu().numpy(), wfr)
    # a side stream: the call is ordered on the stream that is current, not on the default one
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out2, _ = m(wave, n, validate=False, log=True)
    s.synchronize()
    assert np.array_equal(out2.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_c_abi_refuses_before_launching():
    name = "noise_n1025"
    run(name)
    L, h = _lib.lib(), module(name)._hip.h
    f = torch.zeros(200 * 8, device="cuda")
    i64 = torch.full((1,), 1025, dtype=torch.int64, device="cuda")
    p, s = _lib.ptr, _lib.stream_ptr()
    assert L.dv_mel_forward(h, None, p(i64), 1, 1025, p(f), p(i64), 5, 0, s) == -1 and b"null" in L.dv_last_error()
    assert L.dv_mel_forward(h, p(f), p(i64), 0, 1025, p(f), p(i64), 5, 0, s) == -1
    assert L.dv_mel_forward(h, p(f), p(i64), 1, 512, p(f), p(i64), 3, 0, s) == -1 and b"n_max" in L.dv_last_error()
    assert L.dv_mel_forward(h, p(f), p(i64), 1, 1025, p(f), p(i64), 6, 0, s) == -1 and b"L_max" in L.dv_last_error()
    assert L.dv_mel_forward(h, p(f), p(i64), 1, 1025, p(f), p(i64), 5, 4, s) == -1 and b"flag" in L.dv_last_error()
    win, fb = mc.tables()
    hh = C.c_void_p()
    for cfg, word in ((_lib.MelCfg(2048, 256, 100, 1, 1e-7), b"n_fft"), (_lib.MelCfg(1024, 128, 100, 1, 1e-7), b"hop"),
                      (_lib.MelCfg(1024, 256, 100, 0, 1e-7), b"center"), (_lib.MelCfg(1024, 256, 129, 1, 1e-7), b"n_mels"),
                      (_lib.MelCfg(1024, 256, 100, 1, 0.0), b"log_clip")):
        assert L.dv_mel_create(C.byref(cfg), win.ctypes.data_as(C.c_void_p), fb.ctypes.data_as(C.c_void_p), C.byref(hh)) == -1
        assert word in L.dv_last_error()
    # a length outside [513, n_max] with validate=False is a value, not a fault: the row is zeros, its frame count 0
    m = module(name)
    out, frames = m(torch.ones(2, 2048, device="cuda"), torch.tensor([300, 2048], device="cuda"), validate=False)
    assert frames.tolist() == [0, 9] and not out[0].any() and bool(out[1].any())
    with pytest.raises(ValueError, match="lengths must be in"):
        m(torch.ones(2, 2048, device="cuda"), torch.tensor([300, 2048], device="cuda"))
    with pytest.raises(ValueError, match="power"):
        MelSpectrogram(power=3.0, backend="hip").cuda()(torch.ones(1, 2048, device="cuda"))


def test_refer_prompt_on_both_backends():
    n = 24000
    wave = torch.from_numpy(mc.signal("noise", n, 5)[None, :])
    hip = tts_infer.refer_prompt(wave, "cuda", mel_backend="hip")
    ref = tts_infer.refer_prompt(wave, "cuda")
    assert hip.shape == ref.shape == (1, 100, 1 + n // 256)
    window, fb = mc.tables()
    v64, frames = mc.restate64(wave.numpy(), [n], window, fb)
    for label, y in (("k_log_mel", hip), ("torch", ref)):
        e = mc.log_error(y.cpu().numpy(), v64, frames)
        print("refer_prompt %s: %.3f of the log tolerance" % (label, e))
        assert e <= 1.0, label


def test_recordings_to_align(gold):
    from test_align_cpu import align_case, align_mirror
    g, sd, _, noise = align_case(gold)
    model = align_mirror(g, sd, posterior_backend="hip", text_encoder_backend="hip").cuda()
    Ty = int(g["Ty"])
    ns = [(int(yl) - 1) * 256 + 100 for yl in g["y_lengths"]]
    n_max = (Ty - 1) * 256 + 100
    waves = np.zeros((len(ns), n_max), np.float32)
    for b, n in enumerate(ns):
        waves[b, :n] = mc.signal("noise", n, 40 + b)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    scores = {}
    for backend in ("hip", None):
        y, yl = tts_infer.recording_mels(waves, ns, "cuda", mel_backend=backend)
        assert tuple(y.shape) == (len(ns), 100, Ty) and yl.tolist() == [int(v) for v in g["y_lengths"]]
        with torch.no_grad():
            _, _, s = model.align(dev(g["text"]), dev(g["x_lengths"]), y, yl, dev(g["tone"]), dev(g["language"]), noise=dev(noise),
                                  align_backend="hip", return_scores=True)
        scores[backend] = s.cpu().numpy()
    for b, (ty, tx) in enumerate(zip(g["y_lengths"], g["x_lengths"])):
        r = rel_l2(scores["hip"][b, :ty, :tx], scores[None][b, :ty, :tx])
        print("align scores, native mel vs torch mel, row %d: rel-L2 %.3e" % (b, r))
        assert r < 1e-5, b
