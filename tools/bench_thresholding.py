#!/usr/bin/env python3
"""What correcting_x0_fn='dynamic_thresholding' costs around the native denoiser, in ms per complete sampler run:

  thr    DPM_Solver / UniPC(correcting_x0_fn='dynamic_thresholding', ratio 0.995, max 1.0).sample(...) around NativeUNetModel
  plain  the same call without the option (one graph replay)

at the bench shape (B = 8, T = 1024, L = 256, 50-step DPM-Solver++ 2M) and at B = 1, T = 300, L = 150, 30-step UniPC bh2.
In a tree with the thresholding kernels `thr` is one graph replay too, and (thr - plain) / evaluations is the cost of the
feature per evaluation; in a tree without them (--root <checkout of an older commit>, built) `thr` is the stepped path, which
is the comparison "this call before and after".  Runs alternate thr / plain; the figures are the median, minimum and maximum
of --runs timed runs after one warm-up run of each (which plans the shape and captures the graph).  Uses only the public
sampler interface, so the same file measures any checkout.  One JSON line per shape.

Usage: python tools/bench_thresholding.py [--root DIR] [--runs 7] [--shapes bench,b1]"""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout to measure")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--shapes", default="bench,b1")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import diff_vits_amd  # noqa: F401
    from diff_vits_amd import _lib, synth
    from diff_vits_amd.sampler import dpm_solver, uni_pc
    from diff_vits_amd.unet1d.unet_1d_condition import UNet1DConditionModel

    kw = dict(in_channels=208, out_channels=80, block_out_channels=(128, 256, 384, 512), norm_num_groups=8,
              cross_attention_dim=128, attention_head_dim=8, addition_embed_type="text", resnet_time_scale_shift="scale_shift")
    with torch.device("meta"):
        shapes = {k: tuple(v.shape) for k, v in UNet1DConditionModel(**kw).state_dict().items()}
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(shapes, seed=1234).items()}
    m = UNet1DConditionModel(backend="hip", **kw).eval()
    m.load_state_dict(sd)
    m = m.cuda()
    m.hip_engine("bf16x3")
    native_thr = "dv_plan_set_thresholding" in _lib.SIGNATURES
    betas = torch.from_numpy(synth.make_betas())
    thr_kw = dict(correcting_x0_fn="dynamic_thresholding", dynamic_thresholding_ratio=0.995, thresholding_max_val=1.0)
    cases = {"bench": ("dpm", 8, 1024, 256, 50), "b1": ("unipc", 1, 300, 150, 30)}
    for name in args.shapes.split(","):
        family, B, T, L, steps = cases[name]
        x, cond, enc, mask = (torch.from_numpy(a).cuda() for a in synth.make_inputs(B, 80, T, L, seed=4321))
        mod = dpm_solver if family == "dpm" else uni_pc
        ns = mod.NoiseScheduleVP("discrete", betas=betas)
        fn = mod.model_wrapper(mod.NativeUNetModel(m, cond, enc, mask), ns, model_type="x_start")
        make = (lambda **k: mod.DPM_Solver(fn, ns, algorithm_type="dpmsolver++", **k)) if family == "dpm" else \
               (lambda **k: mod.UniPC(fn, ns, variant="bh2", **k))
        solvers = {"thr": make(**thr_kw), "plain": make()}
        times = {k: [] for k in solvers}
        with torch.no_grad():
            for s in solvers.values():
                out = s.sample(x, steps=steps, order=2, skip_type="time_uniform")
                torch.cuda.synchronize()
                assert torch.isfinite(out).all()
            for _ in range(args.runs):
                for k, s in solvers.items():
                    t0 = time.perf_counter()
                    s.sample(x, steps=steps, order=2, skip_type="time_uniform")
                    torch.cuda.synchronize()
                    times[k].append(1e3 * (time.perf_counter() - t0))
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        print(json.dumps(dict(label=args.label, shape=name, solver=family, B=B, T=T, L=L, evaluations=steps, runs=args.runs,
                              thresholded_path="graph" if native_thr else "stepped",
                              thr_ms=round(med["thr"], 3), thr_min_ms=round(min(times["thr"]), 3), thr_max_ms=round(max(times["thr"]), 3),
                              plain_ms=round(med["plain"], 3), plain_min_ms=round(min(times["plain"]), 3),
                              plain_max_ms=round(max(times["plain"]), 3),
                              thr_minus_plain_us_per_evaluation=round(1e3 * (med["thr"] - med["plain"]) / steps, 2))), flush=True)


if __name__ == "__main__":
    main()
