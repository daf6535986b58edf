"""CPU: what the sample-rate converter's GPU tests trust (tests/resample_cases.py), audio.Resample's torch backend and the host-side
refusals.

  * the torch backend (conv1d with stride o + interleave), run in fp64, equals the dense fp64 restatement to <= 1e-12 of the row's peak
    on all nine ratios;
  * known answers: N_out is the ceiling formula, orig == new is the identity, an impulse at sample 0 / N - 1 reads the table back,
    a constant comes back to the table's own ripple (measured: <= 8.8e-4, profiles/resample_reference.txt; asserted below 1e-3, a
    figure the definition's 0.99 roll-off and 6-crossing window produce, not the arithmetic), a tone below both Nyquist frequencies
    keeps amplitude and frequency, a tone between them is attenuated as the fp64 restatement attenuates it (within 1 dB);
  * each row of a ragged batch equals the row alone, bit for bit;
  * (a) the fp32 torch route and (b) the numpy emulation of the kernel's arithmetic both sit at <= 0.5 of RESAMPLE_BLOCK_BOUND - by
    construction (the bound is 2 x their worst figure, tools/resample_reference.py -> profiles/resample_reference.txt): this guards
    the constant against drifting away from the case list, it is not evidence about the kernel;
  * planted faults of the emulation: each one breaks the criterion on the named case."""
import math
import os
import re

import numpy as np
import pytest
import torch

import resample_cases as rc
from diff_vits_amd.audio import Resample, filter_table, output_length, reduce_pair, resample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REF = {}


def reference(name):
    """(wave, pairs, v64, n_out) of a case, computed once and shared."""
    if name not in _REF:
        case = rc.CASES[name]
        wave, pairs = rc.make_wave(case), rc.case_pairs(case)
        v64, n_out = rc.restate64(wave, case["n"], pairs)
        for a in (wave, v64, n_out):
            a.setflags(write=False)
        _REF[name] = (wave, pairs, v64, n_out)
    return _REF[name]


@pytest.mark.parametrize("orig,new", rc.RATES, ids=[rc.ratio_name(o, n) for o, n in rc.RATES])
def test_torch_backend_in_fp64_equals_the_restatement(orig, new):
    o, n = reduce_pair(orig, new)
    for N in (1, 7, 1000, rc.length_for(rc.TILE + 1, o, n)):
        x = rc.signal("noise", N, 5 + N)
        got = Resample(orig, new)(torch.from_numpy(x).double()[None, :])[0].numpy()
        want = rc.restate_row64(x, o, n)
        assert got.shape == want.shape == (output_length(N, o, n),)
        assert float(np.abs(got - want).max()) <= 1e-12 * float(np.abs(want).max())


def test_table_is_the_issues_formula():
    """h[p][j] term by term in plain Python floats, against the vectorised audio.filter_table; rounded once to fp32."""
    for o, n in ((147, 80), (2, 3), (3, 2)):
        h, width = filter_table(o, n)
        base = min(o, n) * 0.99
        assert width == math.ceil(6 * o / base) and h.shape == (n, 2 * width + o) and h.dtype == np.float32
        for p in (0, 1, n - 1):
            for j in range(h.shape[1]):
                t = min(max((-p / n + (j - width) / o) * base, -6.0), 6.0)
                want = (1.0 if t == 0 else math.sin(math.pi * t) / (math.pi * t)) * math.cos(math.pi * t / 12) ** 2 * base / o
                assert abs(float(h[p, j]) - want) <= 2.0 ** -24 * abs(want) + 1e-45, (o, n, p, j)
    # most taps of a phase are exact zeros; about 2 width + 2 are not
    h, width, first, count = rc.table(147, 80)
    assert int(count.max()) <= 2 * width + 2 < h.shape[1]


@pytest.mark.parametrize("orig,new", rc.RATES, ids=[rc.ratio_name(o, n) for o, n in rc.RATES])
def test_output_length_identity_and_impulses(orig, new):
    o, n = reduce_pair(orig, new)
    h, width = filter_table(o, n)
    m = Resample(orig, new)
    for N in sorted({1, max(o - 1, 1), o, o + 1, 997}):
        y = m(torch.zeros(2, N))
        assert y.shape == (2, math.ceil(n * N / o)) and y.shape[1] == output_length(N, o, n)
    x = torch.from_numpy(rc.signal("noise", 100, 1))[None, :]
    assert Resample(orig, orig)(x) is x
    N = 3 * o + 5
    for pos in (0, N - 1):
        x = np.zeros(N, np.float32)
        x[pos] = 1.0
        y = m(torch.from_numpy(x)[None, :])[0].numpy()
        y64 = rc.restate_row64(x, o, n)
        checked = 0
        for i in range(len(y)):
            q, p = divmod(i, n)
            j = pos - (q * o - width)                       # the tap that multiplies sample `pos`
            want = float(h[p, j]) if 0 <= j < h.shape[1] else 0.0
            assert y64[i] == want and abs(float(y[i]) - want) <= 2.0 ** -23 * abs(want)
            checked += 0 <= j < h.shape[1]
        assert checked >= 1


@pytest.mark.parametrize("orig,new", rc.RATES, ids=[rc.ratio_name(o, n) for o, n in rc.RATES])
def test_constant_and_tones(orig, new):
    o, n = reduce_pair(orig, new)
    _, width = filter_table(o, n)
    m = Resample(orig, new)
    # a constant, at least `width` input samples from both ends: the table's own ripple (measured 4.6e-4 .. 8.8e-4 per ratio)
    N = 4 * width + 6 * o
    y = m(torch.ones(1, N))[0].numpy()
    pos = np.arange(len(y)) * o / n
    inner = (pos >= width) & (pos <= N - 1 - width)
    ripple = float(np.abs(y[inner] - 1.0).max())
    print("%s ripple %.3e" % (rc.ratio_name(orig, new), ripple))
    assert inner.sum() >= n and ripple <= 1e-3
    # a tone below both Nyquist frequencies: amplitude and frequency survive
    f, N = 0.2 * min(orig, new), 4096
    x = np.sin(2 * np.pi * f * np.arange(N) / orig).astype(np.float32)
    y = m(torch.from_numpy(x)[None, :])[0].numpy().astype(np.float64)
    cut = len(y) // 8
    mid = y[cut:-cut]
    t = np.arange(cut, len(y) - cut) / new
    basis = np.stack([np.sin(2 * np.pi * f * t), np.cos(2 * np.pi * f * t)], 1)
    coef, res, _, _ = np.linalg.lstsq(basis, mid, rcond=None)
    assert abs(float(np.hypot(*coef)) - 1.0) <= 2e-3                      # amplitude: the ripple again
    assert float(np.sqrt(np.mean((mid - basis @ coef) ** 2))) <= 2e-3     # nothing but that frequency
    assert abs(float(np.arctan2(coef[1], coef[0]))) <= 1e-3               # and no delay
    if new < orig:
        # a tone between the new Nyquist and the old one: attenuated as the fp64 restatement attenuates it
        f = 0.5 * (new / 2.0 + orig / 2.0)
        x = np.sin(2 * np.pi * f * np.arange(N) / orig).astype(np.float32)
        db = lambda v: 20.0 * math.log10(float(np.sqrt(np.mean(v[cut:-cut].astype(np.float64) ** 2))) / math.sqrt(0.5))  # noqa: E731
        want = db(rc.restate_row64(x, o, n))
        line = [l for l in open(os.path.join(ROOT, "profiles", "resample_reference.txt")) if re.match(r"\s+%s\s.*attenuation" % rc.ratio_name(orig, new), l)]
        assert len(line) == 1 and abs(float(line[0].split()[-2]) - want) <= 0.01, "profiles/resample_reference.txt is stale"
        assert want <= -40.0
        torch32 = m(torch.from_numpy(x)[None, :])[0].numpy()
        emu32, _ = rc.emulate32(x[None, :], [N], [(o, n)])
        for label, v in (("torch fp32", torch32), ("emulation", emu32[0])):
            print("%s stop-band tone %.1f Hz: fp64 %.2f dB, %s %.2f dB" % (rc.ratio_name(orig, new), f, want, label, db(v)))
            assert abs(db(v) - want) <= 1.0, label


def test_ragged_rows_equal_the_rows_alone():
    for name in ("ragged3000", "with_identity"):
        case = rc.CASES[name]
        wave = torch.from_numpy(rc.make_wave(case, fill=7.0))          # whatever lies behind a row's samples must not matter
        m = Resample(case["rates"], case["new"])
        out, n_out = m(wave, torch.tensor(case["n"]))
        assert out.shape == (len(case["n"]), rc.out_width(case)) and n_out.tolist() == rc.expected_n_out(case).tolist()
        for b, (N, rate) in enumerate(zip(case["n"], case["rates"])):
            alone = Resample(rate, case["new"])(wave[b:b + 1, :N])[0]
            assert torch.equal(out[b, :alone.shape[0]], alone) and not out[b, alone.shape[0]:].any()
    x = torch.from_numpy(rc.signal("noise", 500, 3))[None, :]
    assert torch.equal(resample(x, 44100), Resample(44100)(x))


@pytest.mark.parametrize("name", list(rc.CASES))
def test_fp32_torch_route_and_emulation_sit_at_half_the_bound(name):
    case = rc.CASES[name]
    wave, pairs, v64, n_out = reference(name)
    a, a_n = Resample(case["rates"], case["new"])(torch.from_numpy(np.array(wave)), torch.tensor(case["n"]))
    b, b_n = rc.emulate32(wave, case["n"], pairs)
    half = 0.5 * rc.RESAMPLE_BLOCK_BOUND
    assert rc.check(case, a.numpy(), a_n.numpy(), v64, half) == [], "a: audio.Resample fp32"
    assert rc.check(case, b, b_n, v64, half) == [], "b: emulation"


def test_bound_is_twice_the_profiles_worst_figure():
    text = open(os.path.join(ROOT, "profiles", "resample_reference.txt")).read()
    a = float(re.search(r"\(a\) worst block (\S+)", text).group(1))
    b = float(re.search(r"\(b\) worst block (\S+)", text).group(1))
    assert 2 * max(a, b) <= rc.RESAMPLE_BLOCK_BOUND <= 2.1 * max(a, b)
    assert "NOTE" not in text


# fault -> (the case, the criterion) that catches it
CAUGHT_BY = {
    "phase_off": ("44100to24000_noise_out513", "block"),
    "pad_short": ("44100to24000_noise_out513", "block"),
    "read_behind": ("ragged3000", "block"),                  # rows shorter than the buffer: what lies behind them leaks in
    "floor_len": ("44100to24000_noise_out513", "n_out"),
    "last_tap": ("48000to24000_impN1", "block"),             # the range's last tap is small: an impulse next to silence shows it
    "seam_short": ("16000to24000_noise_out1025", "block"),   # the first tile's last output reads the sample that is missing
}


@pytest.mark.parametrize("fault", rc.FAULTS)
def test_planted_fault_is_caught(fault):
    name, criterion = CAUGHT_BY[fault]
    case = rc.CASES[name]
    wave, pairs = rc.make_wave(case, fill=0.25), rc.case_pairs(case)
    _, _, v64, n_out = reference(name)
    clean, no = rc.emulate32(wave, case["n"], pairs)
    assert rc.check(case, clean, no, v64) == []
    out, no = rc.emulate32(wave, case["n"], pairs, fault=fault)
    bad = dict(rc.check(case, out, no, v64))
    assert criterion in bad, (fault, bad)


def test_chunked_case_emulation_within_its_a_priori_bound():
    case = rc.CHUNKED_CASE
    wave, (pair,) = rc.make_wave(case), rc.case_pairs(case)
    v64 = rc.restate_row64(wave[0], *pair)
    tol = (int(rc.table(*pair)[3].max()) + 1) * 2.0 ** -24 * rc.abs_sum64(wave[0], *pair)
    got, n_out = rc.emulate32(wave, case["n"], [pair])
    assert n_out.tolist() == [20] and float((np.abs(got[0, :20] - v64) / tol).max()) <= 1.0


def test_host_refusals():
    x = torch.zeros(2, 4096)
    m = Resample(44100, backend="hip")
    with pytest.raises(ValueError, match="GPU"):
        m(x)
    with pytest.raises(ValueError, match="GPU"):
        m(x, torch.tensor([4096, 4096]))
    with pytest.raises(ValueError):
        Resample(44100, backend="triton")
    with pytest.raises(ValueError, match="<= 1024"):
        Resample(44101, 24000, backend="hip")
    with pytest.raises(ValueError, match="positive"):
        Resample(0, 24000)
    t = Resample(44100)
    for bad in ([-1, 4096], [4096, 4097]):
        with pytest.raises(ValueError, match="lengths must be in"):
            t(x, torch.tensor(bad))
    with pytest.raises(ValueError, match="integer"):
        t(x, torch.tensor([4096.0, 4096.0]))
    with pytest.raises(ValueError, match="rows"):
        Resample([44100, 16000, 8000])(x, torch.tensor([4096, 4096]))
    with pytest.raises(ValueError, match="need lengths"):
        Resample([44100, 16000])(x)
