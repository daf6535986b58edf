#!/usr/bin/env python
"""Where RESAMPLE_BLOCK_BOUND (tests/resample_cases.py) comes from.  CPU only.  Over the case list of tests/resample_cases.py, against
the fp64 restatement `restate64`:
  (a) audio.Resample's fp32 torch route on the CPU (every row on its own truncated waveform: Resample.forward with lengths);
  (b) `emulate32`, the numpy float32 emulation of k_resample's own arithmetic (per-phase tap ranges, ascending sums, staged span).
The figure is the block criterion: per block of 256 output samples the worst |v - v64| over the block's fp64 peak, floored at
0.1 x the row's rms.  The bound is 2 x the larger of the two (the factor covers fma contraction, which the emulation cannot hold
equal), rounded up to two digits.  Also: the table's own ripple on a constant, the attenuation of a tone between the two Nyquist
frequencies (what tests/test_resample_reference.py holds the fp32 paths to within 1 dB), and where every planted fault first shows.

    python tools/resample_reference.py > profiles/resample_reference.txt"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import diff_vits_amd  # noqa: E402,F401
import resample_cases as rc  # noqa: E402
from diff_vits_amd.audio import Resample, filter_table, reduce_pair  # noqa: E402


def torch_route(case, wave):
    m = Resample(case["rates"], case["new"])
    out, n_out = m(torch.from_numpy(wave), torch.tensor(case["n"]))
    return out.numpy(), n_out.numpy()


def ripple(orig, new):
    """Worst |y - 1| of the fp64 restatement on a constant, at least `width` input samples away from both ends."""
    o, n = reduce_pair(orig, new)
    _, width = filter_table(o, n)
    N = 4 * width + 6 * o
    y = rc.restate_row64(np.ones(N, np.float32), o, n)
    pos = np.arange(len(y)) * o / n                      # the input position of every output
    inner = (pos >= width) & (pos <= N - 1 - width)
    return float(np.abs(y[inner] - 1.0).max())


def stopband_tone(orig, new):
    """(frequency, attenuation in dB of the fp64 restatement) of a tone midway between the new Nyquist and the old one."""
    o, n = reduce_pair(orig, new)
    f = 0.5 * (new / 2.0 + orig / 2.0)
    N = 4096
    x = np.sin(2 * np.pi * f * np.arange(N) / orig).astype(np.float32)
    y = rc.restate_row64(x, o, n)
    cut = len(y) // 8
    return f, 20.0 * math.log10(float(np.sqrt(np.mean(y[cut:-cut] ** 2))) / math.sqrt(0.5))


def main():
    torch.manual_seed(0)
    torch.set_num_threads(min(8, torch.get_num_threads()))
    worst = {"a": (0.0, ""), "b": (0.0, "")}
    print("# block criterion per case: (a) audio.Resample fp32 torch route on the CPU, (b) numpy fp32 emulation of k_resample")
    print("# %-32s %11s %11s" % ("case", "a_block", "b_block"))
    for name, case in rc.CASES.items():
        wave, pairs = rc.make_wave(case), rc.case_pairs(case)
        v64, n_out = rc.restate64(wave, case["n"], pairs)
        a, _ = torch_route(case, wave)
        b, _ = rc.emulate32(wave, case["n"], pairs)
        fig = {"a": rc.block_error(a, v64, n_out), "b": rc.block_error(b, v64, n_out)}
        for k in fig:
            if fig[k] > worst[k][0]:
                worst[k] = (fig[k], name)
        print("  %-32s %11.3e %11.3e" % (name, fig["a"], fig["b"]))
    top = max(worst["a"][0], worst["b"][0])
    digits = 10.0 ** (math.floor(math.log10(2 * top)) - 1)
    bound = math.ceil(2 * top / digits - 1e-9) * digits
    print("# (a) worst block %.3e at %s" % worst["a"])
    print("# (b) worst block %.3e at %s" % worst["b"])
    print("# RESAMPLE_BLOCK_BOUND = 2 x max(a, b), rounded up to two digits = %.1e" % bound)
    if abs(bound - rc.RESAMPLE_BLOCK_BOUND) > 1e-9 * bound:
        print("# NOTE tests/resample_cases.py holds RESAMPLE_BLOCK_BOUND = %.3e" % rc.RESAMPLE_BLOCK_BOUND)
    print("# the table's own ripple on a constant (fp64 restatement, >= width input samples from both ends): worst |y - 1| per ratio")
    for orig, new in rc.RATES:
        print("  %-8s %6d -> %6d  ripple %.3e" % (rc.ratio_name(orig, new), orig, new, ripple(orig, new)))
    print("# a tone midway between the new Nyquist and the old one (fp64 restatement, rms over the middle 3/4 against the input's)")
    for orig, new in rc.RATES:
        if new < orig:
            f, db = stopband_tone(orig, new)
            print("  %-8s %6d -> %6d  tone %8.1f Hz  attenuation %7.2f dB" % (rc.ratio_name(orig, new), orig, new, f, db))
    print("# planted faults of the emulation: the first case (in list order) and criterion that catches each, and the worst block figure")
    for fault in rc.FAULTS:
        first, worst_f = None, (0.0, "")
        for name, case in rc.CASES.items():
            wave, pairs = rc.make_wave(case, fill=0.25), rc.case_pairs(case)
            v64, n_out = rc.restate64(wave, case["n"], pairs)
            out, no = rc.emulate32(wave, case["n"], pairs, fault=fault)
            bad = rc.check(case, out, no, v64, bound)
            if bad and first is None:
                first = (name, bad[0][0])
            if np.array_equal(no, n_out):
                e = rc.block_error(out, v64, n_out)
                if e > worst_f[0]:
                    worst_f = (e, name)
        print("  %-12s caught by %-28s criterion %-8s worst block %.3e (%s) = %.1f x the bound"
              % (fault, first[0] if first else "NOTHING", first[1] if first else "-", worst_f[0], worst_f[1], worst_f[0] / bound))


if __name__ == "__main__":
    main()
