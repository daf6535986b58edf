#!/usr/bin/env python
"""Log-mel front-end: the native launch (mel.MelSpectrogram(backend='hip'), k_log_mel) against the torch path of the same build, same
process, same GPU, at the shapes of profiles/regulator_bench.txt: B = 1 with 3 s and B = 16 with 11 s of 24 kHz audio.  Both compute
log(clip(mel)) of a full-length batch (the torch path has no other correct batch form: with ragged rows it loops over them, timed
here as `torch rows` for the B = 16 shape with lengths [n, n - 4000, ...]).  HIP events around each call, median of --reps after
--warmup; kernel launches per call from torch.profiler's device events; peak allocator memory above the inputs.

    python tools/mel_bench.py > profiles/mel_bench.txt"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import diff_vits_amd  # noqa: E402,F401
from diff_vits_amd import _lib  # noqa: E402
from diff_vits_amd.mel import MelSpectrogram  # noqa: E402


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return statistics.median(ts), ts[len(ts) // 10], ts[-1 - len(ts) // 10]


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    dev = [e for e in prof.events() if str(e.device_type).endswith("CUDA")]
    return len(dev), sorted({e.name[:48] for e in dev})


def peak_above_inputs(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mel_bench needs a GPU"
    print("# %s, %s, torch %s" % (_lib.lib().dv_version().decode(), torch.cuda.get_device_name(0), torch.__version__))
    print("# us per call: median [10th .. 90th percentile] of %d calls after %d warm-up calls, HIP events; log(clip(mel)), power 1" % (a.reps, a.warmup))
    hip, ref = MelSpectrogram(backend="hip").cuda(), MelSpectrogram().cuda()
    for B, sec in ((1, 3), (16, 11)):
        n = 24000 * sec
        g = torch.Generator(device="cuda").manual_seed(B)
        x = 0.3 * torch.randn(B, n, device="cuda", generator=g)
        full = torch.full((B,), n, dtype=torch.int64, device="cuda")
        routes = [("k_log_mel", lambda: hip(x, full, validate=False, log=True)[0]),
                  ("k_log_mel+check", lambda: hip(x, full, log=True)[0]),
                  ("torch batch", lambda: torch.log(torch.clip(ref(x), min=1e-7)))]
        if B > 1:
            rag = torch.tensor([n - 4000 * b for b in range(B)], dtype=torch.int64, device="cuda")
            routes += [("k_log_mel ragged", lambda: hip(x, rag, validate=False, log=True)[0]), ("torch rows ragged", lambda: ref(x, rag, log=True)[0])]
        res = {}
        for label, fn in routes:
            med, lo, hi = timed(fn, a.warmup, a.reps)
            try:
                nl, names = launches(fn)
                ltxt = "%d" % nl
            except Exception as e:      # the count is a report, the timing above does not depend on it
                ltxt = "not measured (%s)" % type(e).__name__
            res[label] = med
            print("B=%-2d n=%-6d %-18s %9.1f us [%8.1f .. %8.1f]   launches per call %s   peak memory above the inputs %.2f MiB"
                  % (B, n, label, med, lo, hi, ltxt, peak_above_inputs(fn) / 2 ** 20))
        d = float((routes[0][1]() - routes[2][1]()).abs().max())
        print("B=%-2d n=%-6d torch batch / k_log_mel = %.2fx   (largest |log-mel difference| between the two: %.2e)" % (B, n, res["torch batch"] / res["k_log_mel"], d))


if __name__ == "__main__":
    main()
