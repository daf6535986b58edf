#!/usr/bin/env python
"""Where MEL_FRAME_BOUND (tests/mel_cases.py) comes from.  CPU only.  Over the case list of tests/mel_cases.py, against the fp64
restatement `restate64`:
  (a) mel.py's fp32 torch path on the CPU (every row on its own truncated waveform: MelSpectrogram.forward with lengths);
  (b) `emulate32`, the numpy float32 emulation of k_log_mel's own arithmetic (same packing, radix passes, rounded twiddles, band sums).
The figure is the linear-mel criterion: worst frame's max_m |v - v64| / max(peak_f, clip).  The bound is 2 x the larger of the two
(the factor covers fma contraction and the device's sqrtf, which the emulation cannot hold equal), rounded up to two digits.
Also: by how much every planted fault of the emulation misses, the bf16x3 (rejected MFMA contraction) design among them.

    python tools/mel_reference.py > profiles/mel_reference.txt"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import diff_vits_amd  # noqa: E402,F401
import mel_cases as mc  # noqa: E402
from diff_vits_amd.mel import MelSpectrogram  # noqa: E402


def main():
    torch.manual_seed(0)
    torch.set_num_threads(min(8, torch.get_num_threads()))
    worst = {"a": (0.0, ""), "b": (0.0, "")}
    worst_log = {"a": (0.0, ""), "b": (0.0, "")}
    print("# linear-mel criterion per case: (a) mel.py fp32 on the CPU, (b) numpy fp32 emulation of k_log_mel; log: worst |dy| / tolerance")
    print("# %-22s %5s %11s %11s %11s %11s" % ("case", "power", "a_linear", "b_linear", "a_log/tol", "b_log/tol"))
    for name, case in mc.CASES.items():
        window, fb = mc.tables(case["mel_kw"])
        wave = mc.make_wave(case)
        for power in (1, 2) if name in mc.POWER2_CASES else (1,):
            v64, frames = mc.restate64(wave, case["n"], window, fb, power)
            m = MelSpectrogram(power=float(power), **case["mel_kw"])
            a_lin, _ = m(torch.from_numpy(wave), torch.tensor(case["n"]))
            a_log, _ = m(torch.from_numpy(wave), torch.tensor(case["n"]), log=True)
            b_lin, _ = mc.emulate32(wave, case["n"], window, fb, power)
            b_log, _ = mc.emulate32(wave, case["n"], window, fb, power, log=True)
            fig = {"a": mc.linear_error(a_lin.numpy(), v64, frames), "b": mc.linear_error(b_lin, v64, frames)}
            for k in fig:
                if fig[k] > worst[k][0]:
                    worst[k] = (fig[k], "%s power %d" % (name, power))
            # the log tolerance needs the bound: reported against the bound that results below, so keep the inputs
            worst_log.setdefault("rows", []).append((name, power, fig, a_log.numpy(), b_log, v64, frames))
    top = max(worst["a"][0], worst["b"][0])
    digits = 10.0 ** (math.floor(math.log10(2 * top)) - 1)
    bound = math.ceil(2 * top / digits) * digits
    for name, power, fig, a_log, b_log, v64, frames in worst_log.pop("rows"):
        la, lb = mc.log_error(a_log, v64, frames, bound), mc.log_error(b_log, v64, frames, bound)
        for k, v in (("a", la), ("b", lb)):
            if v > worst_log[k][0]:
                worst_log[k] = (v, "%s power %d" % (name, power))
        print("  %-22s %5d %11.3e %11.3e %11.3f %11.3f" % (name, power, fig["a"], fig["b"], la, lb))
    print("# (a) worst linear %.3e at %s" % worst["a"])
    print("# (b) worst linear %.3e at %s" % worst["b"])
    print("# MEL_FRAME_BOUND = 2 x max(a, b), rounded up to two digits = %.1e" % bound)
    print("# log criterion against that bound: (a) worst %.3f of its tolerance at %s, (b) worst %.3f at %s" % (worst_log["a"] + worst_log["b"]))
    if abs(bound - mc.MEL_FRAME_BOUND) > 1e-12 * bound:
        print("# NOTE tests/mel_cases.py holds MEL_FRAME_BOUND = %.3e" % mc.MEL_FRAME_BOUND)
    print("# planted faults of the emulation: the first case (in list order) and criterion that catches each, and the worst linear figure")
    for fault in mc.FAULTS:
        first, worst_f = None, (0.0, "")
        for name, case in mc.CASES.items():
            if name.startswith("b16"):
                continue
            window, fb = mc.tables(case["mel_kw"])
            wave = mc.make_wave(case)
            v64, frames = mc.restate64(wave, case["n"], window, fb, 1)
            out, fr = mc.emulate32(wave, case["n"], window, fb, 1, fault=fault)
            bad = mc.check(case, out, fr, v64, False, bound)
            if bad and first is None:
                first = (name, bad[0][0])
            if np.array_equal(fr, frames):
                e = mc.linear_error(out, v64, frames)
                if e > worst_f[0]:
                    worst_f = (e, name)
        print("  %-16s caught by %-18s criterion %-8s worst linear %.3e (%s) = %.1f x the bound"
              % (fault, first[0] if first else "NOTHING", first[1] if first else "-", worst_f[0], worst_f[1], worst_f[0] / bound))


if __name__ == "__main__":
    main()
