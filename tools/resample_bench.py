#!/usr/bin/env python
"""Sample-rate conversion: the native launch (audio.Resample(backend='hip'), k_resample) against the torch-ops route of the same build
(torchaudio's algorithm on conv1d), same process, same GPU:
  B = 1 / 3 s and B = 16 / 11 s of 44.1 kHz audio -> 24 kHz (full-length batches: one conv1d call for the torch route);
  the ragged B = 16 batch with mixed rates (44.1 / 16 / 48 / 22.05 kHz rows of 11 s, 0.25 s shorter from row to row), where the
  torch route loops over the rows and the kernel is one launch;
  24 -> 16 kHz on a B = 16 vocoder output of 11 s.
HIP events around each call, median and 10th / 90th percentile of --reps after --warmup; kernel launches per call from
torch.profiler's device events; peak allocator memory above the inputs.

    python tools/resample_bench.py > profiles/resample_bench.txt"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import diff_vits_amd  # noqa: E402,F401
from diff_vits_amd import _lib  # noqa: E402
from diff_vits_amd.audio import Resample  # noqa: E402
from mel_bench import launches, peak_above_inputs, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "resample_bench needs a GPU"
    print("# %s, %s, torch %s" % (_lib.lib().dv_version().decode(), torch.cuda.get_device_name(0), torch.__version__))
    print("# us per call: median [10th .. 90th percentile] of %d calls after %d warm-up calls, HIP events" % (a.reps, a.warmup))
    configs = []
    for B, sec, orig, new in ((1, 3, 44100, 24000), (16, 11, 44100, 24000), (16, 11, 24000, 16000)):
        n = orig * sec
        x = 0.3 * torch.randn(B, n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(B))
        full = torch.full((B,), n, dtype=torch.int64, device="cuda")
        hip, ref = Resample(orig, new, backend="hip"), Resample(orig, new)
        configs.append(("B=%-2d %2d s %5d -> %5d" % (B, sec, orig, new),
                        [("k_resample", lambda hip=hip, x=x, full=full: hip(x, full, validate=False)[0]),
                         ("k_resample+check", lambda hip=hip, x=x, full=full: hip(x, full)[0]),
                         ("torch batch", lambda ref=ref, x=x: ref(x))]))
    rates = [(44100, 16000, 48000, 22050)[b % 4] for b in range(16)]
    ns = [r * 11 - (r // 4) * b for b, r in enumerate(rates)]
    x = 0.3 * torch.randn(16, max(ns), device="cuda", generator=torch.Generator(device="cuda").manual_seed(99))
    rag = torch.tensor(ns, dtype=torch.int64, device="cuda")
    hip, ref = Resample(rates, 24000, backend="hip"), Resample(rates, 24000)
    configs.append(("B=16 11 s mixed -> 24000 ragged", [("k_resample", lambda: hip(x, rag, validate=False)[0]), ("torch rows", lambda: ref(x, rag)[0])]))
    for title, routes in configs:
        res = {}
        for label, fn in routes:
            med, lo, hi = timed(fn, a.warmup, a.reps)
            try:
                ltxt = "%d" % launches(fn)[0]
            except Exception as e:      # the count is a report, the timing above does not depend on it
                ltxt = "not measured (%s)" % type(e).__name__
            res[label] = med
            print("%-32s %-18s %9.1f us [%8.1f .. %8.1f]   launches per call %s   peak memory above the inputs %.2f MiB"
                  % (title, label, med, lo, hi, ltxt, peak_above_inputs(fn) / 2 ** 20))
        other = routes[-1][0]
        d = float((routes[0][1]() - routes[-1][1]()).abs().max())
        print("%-32s %s / k_resample = %.2fx   (largest |difference| between the two: %.2e)" % (title, other, res[other] / res["k_resample"], d))


if __name__ == "__main__":
    main()
