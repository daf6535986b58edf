#!/usr/bin/env python3
"""Forced alignment on the GPU: the two native operators (dv_op_mas_scores, dv_op_mas_path; csrc/kernels_align.hip) at the
product's sizes, HIP events around 50 calls after 10 warm-up calls in one process; beside them what the reference's route costs on
the same GPU BEFORE its CPU search even starts - the torch expression of the scores plus the device-to-host copy of
[B, Ty, Tx] - and, from the stamped instantiation (dv_op_mas_path_timed), which part of a search wave's time is the row loop.
Writes profiles/align_bench.txt (or the file given).   Run:  python tools/align_bench.py [FILE]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import diff_vits_amd  # noqa: E402,F401
from diff_vits_amd import _lib, synth  # noqa: E402
from diff_vits_amd.model3 import mas_scores  # noqa: E402

SIZES = [(1, 100, 265), (16, 150, 1047)]          # (B, Tx, Ty)
C, WARM, CALLS = 128, 10, 50


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / CALLS          # microseconds per call


def main():
    L = _lib.lib()
    lines = ["forced alignment, %s, build %s; HIP events around %d calls after %d warm-up calls, microseconds per call"
             % (torch.cuda.get_device_name(0), L.dv_version().decode(), CALLS, WARM)]
    for B, Tx, Ty in SIZES:
        z = torch.from_numpy(synth.normal(3, "ab.z", (B, C, Ty))).cuda()
        m_p = torch.from_numpy(synth.normal(3, "ab.m", (B, C, Tx))).cuda()
        logs_p = (torch.from_numpy(synth.normal(3, "ab.l", (B, C, Tx), std=0.4)) - 0.5).cuda()
        yl = torch.tensor([Ty - 7 * (b % 5) for b in range(B)], dtype=torch.int64).cuda()
        xl = torch.tensor([Tx - 3 * (b % 4) for b in range(B)], dtype=torch.int64).cuda()
        sc = torch.empty((B, Ty, Tx), device="cuda")
        dur = torch.empty((B, Tx), dtype=torch.int32, device="cuda")
        tok = torch.empty((B, Ty), dtype=torch.int32, device="cuda")
        ticks = torch.zeros((B, 2), dtype=torch.int64, device="cuda")
        need = L.dv_op_mas_scratch_bytes(B, Ty, Tx)
        scratch = torch.empty((need,), dtype=torch.uint8, device="cuda") if need else None
        host = torch.empty((B, Ty, Tx), pin_memory=True)
        s = _lib.stream_ptr()
        p = _lib.ptr

        def scores():
            _lib.check(L.dv_op_mas_scores(p(z), p(m_p), p(logs_p), p(yl), p(xl), B, C, Ty, Tx, p(sc), s))

        def search():
            _lib.check(L.dv_op_mas_path(p(sc), p(yl), p(xl), B, Ty, Tx, p(dur), p(tok), p(scratch), need, s))

        def both():
            scores()
            search()

        def torch_scores():
            return mas_scores(z, m_p, logs_p)

        def torch_route():
            host.copy_(mas_scores(z, m_p, logs_p), non_blocking=True)

        t = {k: timed(f) for k, f in (("scores", scores), ("search", search), ("both", both), ("torch scores", torch_scores),
                                      ("torch scores + copy to host", torch_route))}
        _lib.check(L.dv_op_mas_path_timed(p(sc), p(yl), p(xl), B, Ty, Tx, p(dur), p(tok), p(scratch), need, p(ticks), s))
        torch.cuda.synchronize()
        tk = ticks.cpu().numpy().astype(np.float64)
        share = float(np.median(tk[:, 0] / np.maximum(tk[:, 1], 1)))
        lines.append("B = %d, Tx = %d, Ty = %d (decision bits in %s):" % (B, Tx, Ty, "LDS" if need == 0 else "scratch"))
        lines += ["  %-30s %9.1f" % (k, v) for k, v in t.items()]
        lines.append("  search wave: row loop %.0f %% of the wave's time (median over utterances; %.1f us of %.1f us at the 100 MHz clock)"
                     % (100 * share, float(np.median(tk[:, 0])) / 100, float(np.median(tk[:, 1])) / 100))
    text = "\n".join(lines) + "\n"
    print(text)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "align_bench.txt")
    with open(out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
