#!/usr/bin/env python3
"""What a KnownFrames correction (mel infilling) costs around the native denoiser, in ms per complete sampler run at the bench
shape (B = 8, T = 1024, L = 256, 50-step DPM-Solver++ 2M):

  known    DPM_Solver(correcting_xt_fn=KnownFrames(...)).sample(...) around NativeUNetModel: one graph replay with one
           elementwise launch per correction point
  plain    the same call without the correction (one graph replay)
  stepped  the same correction as a plain Python closure (x, t, step) -> x: the loop stepped from Python, what a caller had
           before the correction was compiled into the plan

Runs alternate known / plain / stepped; the figures are the median, minimum and maximum of --runs timed runs after one warm-up
run of each (which plans the shape and captures the graphs).  Also printed: the nodes of the two captured graphs and the
correction points of the plan - the expectation is nodes(known) = nodes(plain) + points.  One JSON line.

Usage: python tools/bench_known_frames.py [--runs 7]"""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import diff_vits_amd  # noqa: F401
    from diff_vits_amd import synth
    from diff_vits_amd.sampler import dpm_solver
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
    B, T, L, steps = 8, 1024, 256, 50
    x, cond, enc, mask = (torch.from_numpy(a).cuda() for a in synth.make_inputs(B, 80, T, L, seed=4321))
    ns = dpm_solver.NoiseScheduleVP("discrete", betas=torch.from_numpy(synth.make_betas()))
    fn = dpm_solver.model_wrapper(dpm_solver.NativeUNetModel(m, cond, enc, mask), ns, model_type="x_start")
    keep = torch.zeros(B, T, dtype=torch.bool, device="cuda")
    keep[:, : T // 3] = True                       # a recorded prompt of a third of the utterance is continued
    kf = dpm_solver.KnownFrames(ns, 0.5 * torch.from_numpy(synth.normal(4321, "bench.known", (B, 80, T))).cuda(), keep,
                                torch.from_numpy(synth.normal(4321, "bench.eps", (B, 80, T))).cuda())
    make = lambda **k: dpm_solver.DPM_Solver(fn, ns, algorithm_type="dpmsolver++", **k)
    solvers = {"known": make(correcting_xt_fn=kf), "plain": make(), "stepped": make(correcting_xt_fn=lambda v, t, step: kf(v, t, step))}
    times = {k: [] for k in solvers}
    skw = dict(steps=steps, order=2, skip_type="time_uniform")
    with torch.no_grad():
        outs = {}
        for k, s in solvers.items():
            outs[k] = s.sample(x, **skw)
            torch.cuda.synchronize()
            assert torch.isfinite(outs[k]).all()
        for _ in range(args.runs):
            for k, s in solvers.items():
                t0 = time.perf_counter()
                s.sample(x, **skw)
                torch.cuda.synchronize()
                times[k].append(1e3 * (time.perf_counter() - t0))
    rel = float((outs["known"] - outs["stepped"]).norm() / outs["stepped"].norm())
    nodes = {k: [p.graph_nodes() for plan in solvers[k]._plans.values() for p in plan._per_shape.values() if p.graph_nodes()] for k in ("known", "plain")}
    points = len(next(p for p in solvers["known"]._plans.values() if p.known_frames).known_coefs())
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    rec = dict(B=B, T=T, L=L, steps=steps, runs=args.runs, kept_frames_per_row=int(keep[0].sum()), correction_points=points,
               graph_nodes_known=nodes["known"], graph_nodes_plain=nodes["plain"], known_vs_stepped_rel_l2=rel,
               known_minus_plain_us_per_point=round(1e3 * (med["known"] - med["plain"]) / points, 2))
    for k in solvers:
        rec.update({k + "_ms": round(med[k], 3), k + "_min_ms": round(min(times[k]), 3), k + "_max_ms": round(max(times[k]), 3)})
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
