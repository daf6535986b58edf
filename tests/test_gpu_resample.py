"""GPU: the native sample-rate converter (dv_resample_forward / k_resample, csrc/kernels_resample.hip; audio.Resample(backend='hip'),
tts_infer.refer_prompt / recording_mels / save_wav) against the fp64 restatement of tests/resample_cases.py, under its criterion:

  block   per 256 output samples  max |v - v64| / max(block peak, 0.1 x row rms) <= RESAMPLE_BLOCK_BOUND   (profiles/resample_reference.txt:
          measured, 2 x max(a, b))
  n_out   == ceil(n N / o), every element at or past a row's n_out exactly 0, the output finite.

Per ratio the rows are chosen so that N_out is TILE - 1, TILE, TILE + 1 and 2 TILE + 1 (when upsampling N_out moves in steps of
n / o: the first length that reaches the target), plus N = 1 and N < width, over mel_cases' signal kinds.  The torch route on the
GPU runs on the same rows and its figure is printed beside the kernel's.  A ragged batch of five rows with five rate pairs is one
launch; NaN behind every row's samples changes no bit (a read past a row's end cannot pass that).  Bitwise: rows equal the B = 1
calls, two calls agree, replacing one row leaves the others, a capture-and-replay equals the eager call.  Product surface:
refer_prompt, recording_mels -> VITS.align, save_wav on both backends.  DVITS_PARITY_REPORT=<file> appends the worst block per ratio
(profiles/resample_parity.txt was made so)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mel_cases as mc
import resample_cases as rc
from diff_vits_amd import _lib, tts_infer
from diff_vits_amd.audio import Resample, read_wav, write_wav

pytestmark = pytest.mark.gpu

_REF, _MODS = {}, {}


def case_of(name):
    return rc.CHUNKED_CASE if name == rc.CHUNKED_CASE["name"] else rc.CASES[name]


def reference(name):
    if name not in _REF:
        case = case_of(name)
        wave, pairs = rc.make_wave(case), rc.case_pairs(case)
        v64, n_out = rc.restate64(wave, case["n"], pairs)
        for a in (wave, v64, n_out):
            a.setflags(write=False)
        _REF[name] = (wave, v64, n_out)
    return _REF[name]


def module(name, backend="hip"):
    case = case_of(name)
    key = (tuple(case["rates"]), case["new"], backend)
    if key not in _MODS:
        _MODS[key] = Resample(case["rates"], case["new"], backend=backend)
    return _MODS[key]


def run(name, backend="hip", wave=None):
    case = case_of(name)
    wave = reference(name)[0] if wave is None else wave
    out, n_out = module(name, backend)(torch.from_numpy(np.array(wave)).cuda(), torch.tensor(case["n"], device="cuda"))
    torch.cuda.synchronize()
    return out.cpu().numpy(), n_out.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _report(line):
    print(line)
    path = os.environ.get("DVITS_PARITY_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@pytest.mark.parametrize("ratio", list(rc.RATIO_CASES))
def test_against_the_fp64_restatement(ratio):
    worst = {"k_resample": (0.0, ""), "torch": (0.0, "")}
    for name in rc.RATIO_CASES[ratio]:
        case = rc.CASES[name]
        wave, v64, n_out = reference(name)
        for label, backend in (("k_resample", "hip"), ("torch", None)):
            got, no = run(name, backend)
            e = rc.block_error(got, v64, n_out) if np.array_equal(no, n_out) else float("inf")
            if e >= worst[label][0]:
                worst[label] = (e, name)
            assert rc.check(case, got, no, v64) == [], (label, name)
    _report("%-8s worst block  k_resample %.3e (%s)  torch on the GPU %.3e (%s)  (bound %.1e)"
            % ((ratio,) + worst["k_resample"] + worst["torch"] + (rc.RESAMPLE_BLOCK_BOUND,)))


@pytest.mark.parametrize("name", ["ragged3000", "ragged3333", "with_identity"])
def test_ragged_batch_in_one_launch_with_nan_behind_the_rows(name):
    case = rc.CASES[name]
    wave, v64, n_out = reference(name)
    got, no = run(name)
    assert np.array_equal(no, rc.expected_n_out(case)) and np.all(np.isfinite(got))
    assert rc.padding_is_zero(got, no)
    assert rc.check(case, got, no, v64) == []
    _report("%-14s worst block  k_resample %.3e  (bound %.1e)" % (name, rc.block_error(got, v64, n_out), rc.RESAMPLE_BLOCK_BOUND))
    poisoned, no2 = run(name, wave=rc.make_wave(case, fill=np.nan))
    assert np.all(np.isfinite(poisoned)) and np.array_equal(no, no2)
    assert np.array_equal(bits(got), bits(poisoned))
    if name == "with_identity":          # the delta table copies every bit
        assert np.array_equal(bits(got[0, :1000]), bits(wave[0, :1000])) and got[2, 0] == 1.0


def test_bitwise_repeats_rows_alone_and_a_replaced_row():
    name = "ragged3333"
    case = rc.CASES[name]
    wave = np.array(reference(name)[0])
    got, no = run(name)
    again, no2 = run(name)
    assert np.array_equal(bits(got), bits(again)) and np.array_equal(no, no2)
    for b, (N, rate) in enumerate(zip(case["n"], case["rates"])):
        m = Resample(rate, case["new"], backend="hip")
        alone = m(torch.from_numpy(wave[b:b + 1, :N].copy()).cuda())[0].cpu().numpy()
        assert alone.shape == (int(no[b]),) and np.array_equal(bits(got[b, :int(no[b])]), bits(alone)), (b, N)
    other = wave.copy()
    other[2] = rc.signal("tone", wave.shape[1], 77)
    changed, _ = run(name, wave=other)
    keep = [0, 1, 3, 4]
    assert np.array_equal(bits(got[keep]), bits(changed[keep])) and not np.array_equal(got[2], changed[2])


def test_chunked_tile_within_the_a_priori_bound_of_its_sum():
    """o : n = 1000 : 1 - table and span do not fit the LDS together, the tile goes in two chunks; ~12 000 taps per output."""
    case = rc.CHUNKED_CASE
    wave, v64, n_out = reference(case["name"])
    (pair,) = rc.case_pairs(case)
    got, no = run(case["name"])
    assert no.tolist() == [20] and rc.padding_is_zero(got, no)
    tol = (int(rc.table(*pair)[3].max()) + 1) * 2.0 ** -24 * rc.abs_sum64(wave[0], *pair)
    e = float((np.abs(got[0, :20] - v64[0, :20]) / tol).max())
    print("1000:1 chunked: worst |error| = %.3f of (taps + 1) 2^-24 sum |h x|" % e)
    assert e <= 1.0


def test_no_write_outside_the_result_and_capture_replay():
    name = "ragged3333"
    case = rc.CASES[name]
    want, wno = run(name)
    m = module(name)
    B, n_max, W, G = len(case["n"]), case["n_max"], rc.out_width(case), 1024
    buf = torch.full((G + B * W + G,), 12345.0, device="cuda")
    nbuf = torch.full((16 + B + 16,), -77, dtype=torch.int64, device="cuda")
    wave = torch.from_numpy(np.array(reference(name)[0])).cuda()
    n = torch.tensor(case["n"], device="cuda")
    pair = torch.tensor(m.row_pair, dtype=torch.int32, device="cuda")
    rc_ = _lib.lib().dv_resample_forward(m._hip.h, _lib.ptr(wave), _lib.ptr(n), _lib.ptr(pair), B, n_max, C.c_void_p(buf.data_ptr() + 4 * G), W,
                                         C.c_void_p(nbuf.data_ptr() + 8 * 16), _lib.stream_ptr())
    _lib.check(rc_, "dv_resample_forward")
    torch.cuda.synchronize()
    assert bool((buf[:G] == 12345.0).all()) and bool((buf[G + B * W:] == 12345.0).all())
    assert bool((nbuf[:16] == -77).all()) and bool((nbuf[16 + B:] == -77).all())
    assert np.array_equal(bits(buf[G:G + B * W].cpu().numpy().reshape(want.shape)), bits(want))
    assert np.array_equal(nbuf[16:16 + B].cpu().numpy(), wno)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):          # one kernel node: a linear graph
        out, n_out = m(wave, n, validate=False)
    out.zero_()
    n_out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(want)) and np.array_equal(n_out.cpu().numpy(), wno)


def test_c_abi_refuses_before_launching():
    name = "44100to24000_noise_out513"
    run(name)
    L, h = _lib.lib(), module(name)._hip.h
    n_max = rc.CASES[name]["n_max"]
    W = rc.out_width(rc.CASES[name])
    f = torch.zeros(4096, device="cuda")
    i64 = torch.full((2,), n_max, dtype=torch.int64, device="cuda")
    i32 = torch.zeros(2, dtype=torch.int32, device="cuda")
    p, s = _lib.ptr, _lib.stream_ptr()
    off = lambda t, k: C.c_void_p(t.data_ptr() + k)  # noqa: E731
    for args in ((None, p(f), p(i64), None, 1, n_max, p(f), W, p(i64), s), (h, None, p(i64), None, 1, n_max, p(f), W, p(i64), s),
                 (h, p(f), None, None, 1, n_max, p(f), W, p(i64), s), (h, p(f), p(i64), None, 1, n_max, None, W, p(i64), s),
                 (h, p(f), p(i64), None, 1, n_max, p(f), W, None, s)):
        assert L.dv_resample_forward(*args) == -1 and b"null" in L.dv_last_error()
    for B in (0, 65536):
        assert L.dv_resample_forward(h, p(f), p(i64), None, B, n_max, p(f), W, p(i64), s) == -1 and b"B =" in L.dv_last_error()
    for bad in (0, 2 ** 30 + 1):
        assert L.dv_resample_forward(h, p(f), p(i64), None, 1, bad, p(f), W, p(i64), s) == -1 and b"n_max" in L.dv_last_error()
    for bad in (W - 1, W + 1):
        assert L.dv_resample_forward(h, p(f), p(i64), None, 1, n_max, p(f), bad, p(i64), s) == -1 and b"n_out_max" in L.dv_last_error()
    for args in ((h, off(f, 2), p(i64), None, 1, n_max, p(f), W, p(i64), s), (h, p(f), off(i64, 4), None, 1, n_max, p(f), W, p(i64), s),
                 (h, p(f), p(i64), off(i32, 2), 1, n_max, p(f), W, p(i64), s), (h, p(f), p(i64), None, 1, n_max, off(f, 1), W, p(i64), s),
                 (h, p(f), p(i64), None, 1, n_max, p(f), W, off(i64, 4), s)):
        assert L.dv_resample_forward(*args) == -1 and b"misaligned" in L.dv_last_error()
    hh = C.c_void_p()
    mk = lambda *v: np.array(v, dtype=np.int32).ctypes.data_as(C.c_void_p)  # noqa: E731
    for o, n, k, word in ((mk(44101), mk(24000), 1, b"<= 1024"), (mk(0), mk(24000), 1, b">= 1"), (mk(2), mk(1), 0, b"n_pairs"), (mk(2), mk(1), 65, b"n_pairs")):
        assert L.dv_resample_create(o, n, k, C.byref(hh)) == -1 and word in L.dv_last_error()
    assert L.dv_resample_create(None, mk(1), 1, C.byref(hh)) == -1 and b"null" in L.dv_last_error()
    # a length outside [0, n_max] or a pair outside the handle's, with validate=False / through the ABI: a value, not a fault
    m = Resample([44100, 16000, 44100], 24000, backend="hip")
    x = torch.ones(3, 2000, device="cuda")
    out, n_out = m(x, torch.tensor([2001, 2000, -1], device="cuda"), validate=False)
    assert n_out.tolist() == [0, 3000, 0] and not out[0].any() and not out[2].any() and bool(out[1].any())
    with pytest.raises(ValueError, match="lengths must be in"):
        m(x, torch.tensor([2001, 2000, 5], device="cuda"))
    out = torch.full((3, m.out_width(2000)), 5.0, device="cuda")
    n_out = torch.full((3,), 9, dtype=torch.int64, device="cuda")
    full = torch.tensor([2000, 2000, 2000], device="cuda")
    pair = torch.tensor([2, 1, -1], dtype=torch.int32, device="cuda")
    _lib.check(L.dv_resample_forward(m._hip.h, p(x), p(full), p(pair), 3, 2000, p(out), m.out_width(2000), p(n_out), s), "dv_resample_forward")
    torch.cuda.synchronize()
    assert n_out.tolist() == [0, 3000, 0] and not out[0].any() and not out[2].any() and bool(out[1].any())


def test_refer_prompt_from_a_file_on_both_routes(tmp_path):
    n = 44100
    x = torch.from_numpy(mc.signal("noise", n, 5)[None, :])
    path = str(tmp_path / "prompt.wav")
    write_wav(path, x, 44100, bits=32)
    hip = tts_infer.refer_prompt(path, "cuda", audio_backend="native", resample_backend="hip", mel_backend="hip")
    ref = tts_infer.refer_prompt(path, "cuda", audio_backend="native")
    assert hip.shape == ref.shape == (1, 100, 1 + 24000 // 256)
    # the fp64 chain: restated conversion, then the restated mel of that waveform
    y64 = rc.restate_row64(x[0].numpy(), 147, 80)
    window, fb = mc.tables()
    v64, frames = mc.restate64(y64[None, :], [len(y64)], window, fb)
    for label, y in (("k_resample + k_log_mel", hip), ("torch", ref)):
        e = mc.log_error(y.cpu().numpy(), v64, frames)
        print("refer_prompt from a 44.1 kHz file, %s: %.3f of the log tolerance" % (label, e))
        assert e <= 1.0, label


def test_recordings_at_their_own_rates_to_align(gold):
    from test_align_cpu import align_case, align_mirror
    g, sd, _, noise = align_case(gold)
    model = align_mirror(g, sd, posterior_backend="hip", text_encoder_backend="hip").cuda()
    Ty = int(g["Ty"])
    rates = [44100, 16000, 48000, 22050][:len(g["y_lengths"])]
    rates += [24000] * (len(g["y_lengths"]) - len(rates))
    # every row long enough at its own rate for (y_length - 1) * 256 + 100 samples at 24 kHz
    want = [(int(yl) - 1) * 256 + 100 for yl in g["y_lengths"]]
    ns = [rc.length_for(w, *rc.reduce_pair(r, 24000)) for w, r in zip(want, rates)]
    n_max = max(ns)
    waves = np.zeros((len(ns), n_max), np.float32)
    for b, n in enumerate(ns):
        waves[b, :n] = mc.signal("noise", n, 40 + b)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    durations = {}
    for backend in ("hip", None):
        y, yl = tts_infer.recording_mels(waves, ns, "cuda", mel_backend=backend, sample_rates=rates, resample_backend=backend)
        assert yl.tolist() == [int(v) for v in g["y_lengths"]]
        assert y.shape[2] >= Ty and not y[:, :, Ty:].any()
        y = y[:, :, :Ty].contiguous()
        with torch.no_grad():
            res = model.align(dev(g["text"]), dev(g["x_lengths"]), y, yl, dev(g["tone"]), dev(g["language"]), noise=dev(noise), align_backend="hip")
        durations[backend] = res[0].cpu().numpy()
    assert durations["hip"].dtype.kind == "i" and np.array_equal(durations["hip"], durations[None])


def test_save_wav_converts_on_the_kernel(tmp_path):
    samples = torch.from_numpy(mc.signal("noise", 24000, 8)[None, :]) * 0.5
    tts_infer.save_wav(str(tmp_path / "hip.wav"), samples, out_rate=16000, resample_backend="hip")
    tts_infer.save_wav(str(tmp_path / "ref.wav"), samples, out_rate=16000)
    a, sr = read_wav(str(tmp_path / "hip.wav"))
    b, sr2 = read_wav(str(tmp_path / "ref.wav"))
    assert sr == sr2 == 16000 and a.shape == b.shape == (1, 16000)
    # both routes are within RESAMPLE_BLOCK_BOUND x the peak of the same fp64 values (<< one code), then rounded: at most one code apart
    assert float((a - b).abs().max()) <= 1.0 / 32768.0
