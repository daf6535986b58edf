"""CPU: what the log-mel front-end's GPU tests trust (tests/mel_cases.py), the torch backend's ragged path and the host-side refusals.

  * the fp64 restatement (explicit reflect index map + explicit DFT matrix) equals mel.py's fp64 torch.stft path on full-length rows to
    <= 1e-12 of the frame's peak;
  * MelSpectrogram.forward with `lengths`: every row equals the stand-alone call on its own samples bit for bit, zeros behind it; the
    zero-padded batch WITHOUT lengths is what the ragged path corrects (its last valid frames differ);
  * `lengths=None` is bit-equal to the code path this module had before `lengths` existed, on tests/test_mel.py's inputs;
  * (a) mel.py's fp32 path and (b) the numpy emulation of the kernel's arithmetic both sit at <= 0.5 of MEL_FRAME_BOUND - by
    construction (the bound is 2 x their worst figure, tools/mel_reference.py -> profiles/mel_reference.txt): this guards the constant
    against drifting away from the case list, it is not evidence about the kernel;
  * planted faults of the emulation: each one breaks the named criterion on the named case - the criteria can see every mistake the
    kernel could plausibly make;
  * closed forms: all zeros, unit impulses, DC."""
import math

import numpy as np
import pytest
import torch

import mel_cases as mc
from diff_vits_amd.mel import MelSpectrogram, reference_mel_prompt

_REF = {}


def reference(name, power=1):
    """(wave, window, fb, v64, frames) of a case, computed once and shared."""
    key = (name, power)
    if key not in _REF:
        case = mc.CASES[name]
        window, fb = mc.tables(case["mel_kw"])
        wave = mc.make_wave(case)
        v64, frames = mc.restate64(wave, case["n"], window, fb, power)
        for a in (v64, frames):
            a.setflags(write=False)
        _REF[key] = (wave, window, fb, v64, frames)
    return _REF[key]


SMALL = [n for n in mc.CASES if not n.startswith("b16")]


@pytest.mark.parametrize("name", ["noise_n513", "noise_n1025", "tone_n2048", "dc_n1025", "quiet_n2048"])
def test_restatement_equals_the_fp64_stft_path(name):
    wave, window, fb, v64, frames = reference(name)
    m = MelSpectrogram().double()
    got = m(torch.from_numpy(wave).double()).numpy()
    assert got.shape == v64.shape
    peak = np.maximum(got.max(1, keepdims=True), mc.CLIP)
    assert float((np.abs(got - v64) / peak).max()) <= 1e-12


def test_torch_backend_with_lengths_is_each_row_alone():
    case = mc.CASES["ragged5000"]
    wave = torch.from_numpy(mc.make_wave(case, fill=7.0))          # whatever lies behind a row's samples must not matter
    m = MelSpectrogram()
    out, frames = m(wave, torch.tensor(case["n"]))
    assert out.shape == (5, 100, 1 + 5000 // 256) and frames.tolist() == [1 + n // 256 for n in case["n"]]
    for b, n in enumerate(case["n"]):
        alone = m(wave[b:b + 1, :n])[0]
        assert torch.equal(out[b, :, :alone.shape[-1]], alone)
        assert not out[b, :, alone.shape[-1]:].any()
    log_out, _ = reference_mel_prompt(wave, lengths=torch.tensor(case["n"]))
    for b, n in enumerate(case["n"]):
        assert torch.equal(log_out[b, :, :1 + n // 256], reference_mel_prompt(wave[b:b + 1, :n])[0])
        assert not log_out[b, :, 1 + n // 256:].any()


def test_zero_padded_batch_without_lengths_is_what_lengths_corrects():
    x = torch.zeros(1, 8000)
    x[0, :5000] = torch.from_numpy(mc.signal("noise", 5000, 3))
    m = MelSpectrogram()
    padded = m(x)[0, :, :1 + 5000 // 256]
    alone = m(x[:, :5000])[0]
    ragged, _ = m(x, torch.tensor([5000]))
    assert float((padded[:, -2:] - alone[:, -2:]).abs().max()) > 0.5          # the contamination the ragged path removes
    assert torch.equal(ragged[0, :, :alone.shape[-1]], alone)


def _forward_before(m, waveform):
    """MelSpectrogram.forward as it was before `lengths` / `backend` existed, op for op."""
    shape = waveform.shape
    x = waveform.reshape(-1, shape[-1])
    spec = torch.stft(x, m.n_fft, hop_length=m.hop_length, win_length=m.n_fft, window=m.window.to(x), center=m.center,
                      pad_mode="reflect", normalized=False, onesided=True, return_complex=True).abs()
    if m.power != 1.0:
        spec = spec.pow(m.power)
    mel = torch.matmul(spec.transpose(-1, -2), m.fb.to(spec)).transpose(-1, -2)
    return mel.reshape(shape[:-1] + mel.shape[-2:])


def test_default_path_is_bit_equal_to_before():
    sr = 24000
    tone = torch.sin(2 * math.pi * 3000.0 * torch.arange(sr, dtype=torch.float32) / sr).unsqueeze(0)
    noise = torch.from_numpy(np.random.RandomState(0).randn(2, 5000).astype(np.float32))
    for x in (tone, noise):
        for power in (1.0, 2.0):
            m = MelSpectrogram(power=power)
            assert torch.equal(m(x), _forward_before(m, x))
    assert torch.equal(reference_mel_prompt(noise), torch.log(torch.clip(_forward_before(MelSpectrogram(), noise), min=1e-7)))


def _figures(name, power):
    wave, window, fb, v64, frames = reference(name, power)
    case = mc.CASES[name]
    m = MelSpectrogram(power=float(power), **case["mel_kw"])
    n = torch.tensor(case["n"])
    a_lin, a_fr = m(torch.from_numpy(wave), n)
    a_log, _ = m(torch.from_numpy(wave), n, log=True)
    b_lin, b_fr = mc.emulate32(wave, case["n"], window, fb, power)
    b_log, _ = mc.emulate32(wave, case["n"], window, fb, power, log=True)
    return case, v64, (a_lin.numpy(), a_log.numpy(), a_fr.numpy()), (b_lin, b_log, b_fr)


@pytest.mark.parametrize("name,power", [(n, 1) for n in mc.CASES] + [(n, 2) for n in mc.POWER2_CASES])
def test_fp32_torch_path_and_emulation_sit_at_half_the_bound(name, power):
    case, v64, a, b = _figures(name, power)
    for label, (lin, log, fr) in (("a: mel.py fp32", a), ("b: emulation", b)):
        half = 0.5 * mc.MEL_FRAME_BOUND
        assert mc.check(case, lin, fr, v64, False, half) == [], label
        assert mc.check(case, log, fr, v64, True) == [], label


# fault -> (the case, the criterion) that catches it
CAUGHT_BY = {
    "symmetric_pad": ("impN1_n1025", "linear"),      # the repeated edge sample doubles the impulse at n - 1
    "buffer_end": ("ragged4096", "linear"),          # rows shorter than the buffer reflect zeros in: the contamination of the issue
    "ceil_frames": ("noise_n768", "frames"),         # n a multiple of the hop: ceil(n / hop) is one frame short
    "symmetric_hann": ("dc_n1025", "linear"),
    "no_nyquist": ("fmax12500_n1025", "linear"),     # the only filterbank here whose row 512 is non-zero
    "band_hi_short": ("noise_n1025", "linear"),
    "bf16x3": ("tone_n2048", "log"),                 # the tone 80 dB down loses its digits in the log
}


@pytest.mark.parametrize("fault", mc.FAULTS)
def test_planted_fault_is_caught(fault):
    name, criterion = CAUGHT_BY[fault]
    wave, window, fb, v64, frames = reference(name)
    case = mc.CASES[name]
    log = criterion == "log"
    clean, fr = mc.emulate32(wave, case["n"], window, fb, log=log)
    assert mc.check(case, clean, fr, v64, log) == []
    out, fr = mc.emulate32(wave, case["n"], window, fb, log=log, fault=fault)
    bad = dict(mc.check(case, out, fr, v64, log))
    assert criterion in bad, (fault, bad)


def test_zeros_closed_form():
    for name in ("zeros_n513", "zeros_n2048"):
        wave, window, fb, v64, frames = reference(name)
        case = mc.CASES[name]
        lin, _ = mc.emulate32(wave, case["n"], window, fb)
        log, _ = mc.emulate32(wave, case["n"], window, fb, log=True)
        assert not lin.any()
        want = math.log(float(np.float32(1e-7)))
        assert float(np.abs(log[0, :, :int(frames[0])] - want).max()) <= 2.0 ** -22 * abs(want)


@pytest.mark.parametrize("kind", ["imp0", "imp1", "impN1", "impN2", "impB"])
def test_impulse_closed_form(kind):
    """Every bin's magnitude of a frame that sees the impulse once is the window value at its position: mel = window * colsum(fb)."""
    n = 1025
    wave, window, fb, v64, frames = reference("%s_n%d" % (kind, n))
    pos = mc.impulse_position(kind, n)
    idx = mc.frame_index(n)
    colsum = fb.astype(np.float64).sum(0)
    checked = 0
    for f in range(int(frames[0])):
        hits = np.nonzero(idx[f] == pos)[0]
        if len(hits) == 1:
            want = float(window[hits[0]]) * colsum
            assert float(np.abs(v64[0, :, f] - want).max()) <= 1e-12 * max(want.max(), 1e-30) + 1e-15
            checked += 1
    assert checked >= 1


def test_dc_closed_form():
    """Periodic Hann on a constant: bins 0 and 1 carry 512 and 256, the others only the float32 rounding of the window's 1024
    entries (each <= 2^-25, so <= 1024 * 2^-25 per bin, times the band's weights)."""
    wave, window, fb, v64, frames = reference("dc_n2048")
    want = 512.0 * fb[0].astype(np.float64) + 256.0 * fb[1].astype(np.float64)
    assert float(np.abs(v64[0, :, 4] - want).max()) <= 1024 * 2.0 ** -25 * float(fb.astype(np.float64).sum(0).max())


def test_host_refusals():
    m = MelSpectrogram(backend="hip")
    x = torch.zeros(2, 4096)
    with pytest.raises(ValueError, match="GPU"):
        m(x, torch.tensor([4096, 4096]))
    with pytest.raises(ValueError, match="GPU"):
        m(x)
    with pytest.raises(ValueError, match="GPU"):
        m(x.double(), torch.tensor([4096, 4096]))
    with pytest.raises(ValueError):
        MelSpectrogram(backend="triton")
    t = MelSpectrogram()
    for bad in ([512, 4096], [4096, 4097], [0, 4096]):
        with pytest.raises(ValueError, match="lengths must be in"):
            t(x, torch.tensor(bad))
        with pytest.raises(ValueError, match="lengths must be in"):
            m.check_lengths(x, torch.tensor(bad))
    with pytest.raises(ValueError, match="integer"):
        t(x, torch.tensor([4096.0, 4096.0]))
    with pytest.raises(ValueError, match="integer"):
        t(x, torch.tensor([4096]))
