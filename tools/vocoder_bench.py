"""Vocoder timing (not bench.py): backend="hip" against backend="torch" on the same GPU at B = 1 / T = 300 and B = 16 / T = 1024,
with launches per forward, peak memory above the inputs and samples per second against 24 kHz.  The torch path is the yardstick.

    python tools/vocoder_bench.py [--reps 20] [--out profiles/vocoder_bench.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import vocoder_cases as vc  # noqa: E402
from diff_vits_amd import _lib, vocoder  # noqa: E402


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        t.append(e0.elapsed_time(e1))
    t.sort()
    return t[len(t) // 2], t[0], t[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cfg = vc.CFG_FULL
    sd = vc.make_weights(cfg)
    lines = ["vocoder: backend='hip' vs backend='torch' (eager fp32) on one GPU, C = 512 / I = 1536 / 8 layers; median (min .. max) of %d" % a.reps]
    for B, T in ((1, 300), (16, 1024)):
        mel = vc.make_mel(B, T, [T] * B).cuda()
        res = {}
        for backend in ("hip", "torch"):
            v = vocoder.Vocoder.from_state_dict(sd, backend=backend).to("cuda")
            unwritten = _lib.lib().dv_unwritten_bytes()
            v.decode(mel)
            unwritten = _lib.lib().dv_unwritten_bytes() - unwritten      # the plan's activation memory (dmalloc(zero = false))
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            v.decode(mel)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base        # (torch's allocator: the hip engine's plan memory is outside it)
            med, lo, hi = timed(lambda: v.decode(mel), a.reps)
            res[backend] = med
            extra = ""
            if backend == "hip":
                n, fl = v.stats()
                extra = ", plan activation memory %.1f MiB, %d launches per forward, %.1f GFLOP" % (unwritten / 2 ** 20, n, fl / 1e9)
            samples = B * (T - 1) * 256
            lines.append("B=%d T=%d %-5s: %.3f ms (%.3f .. %.3f), %.1f M samples/s = %.0f x real time at 24 kHz, torch-allocator peak above the inputs %.1f MiB%s"
                         % (B, T, backend, med, lo, hi, samples / med / 1e3, samples / 24000.0 / (med / 1e3), peak / 2 ** 20, extra))
        lines.append("B=%d T=%d: hip / torch = %.2f x" % (B, T, res["torch"] / res["hip"]))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
