#!/usr/bin/env python3
"""What classifier-free guidance costs inside the native sampler graph, in ms per complete 50-step DPM-Solver++ 2M run at
T = 1024, L = 256:

  guided  B = 8:  model_wrapper(guidance_type='classifier-free', guidance_scale=2) around NativeUNetModel - one graph replay,
                  the engine at 2B = 16 rows, two elementwise launches per evaluation around the UNet schedule
  plain   B = 16: the unguided run of the same plan at the batch the guided one really evaluates

`--mode plain` uses only the sampler interface every checkout has, so `--root <built checkout of the parent commit>` measures
the parent on the same box; `--mode guided` needs this tree.  The figures are the median, minimum and maximum of --runs timed
runs after one warm-up run (which plans the shape and captures the graph).  `graph_nodes` is COUNTED on the captured graph
(dv_plan_graph_nodes: every kernel launch of the complete loop - head-of-loop chains, evaluations, updates; null in a
checkout without that entry point) and `graph_nodes_per_evaluation` is that count over the evaluations: guided minus plain
at the same engine rows is what guidance adds.  `unet_launches_per_forward` is the engine's own count of one forward
(dv_unet_stats).  One JSON line.

Usage: python tools/bench_guidance.py --mode guided|plain [--root DIR] [--runs 7] [--label TEXT]"""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("guided", "plain"), required=True)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout to measure")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
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
    T, L, steps = 1024, 256, 50
    B = 8 if args.mode == "guided" else 16
    x, cond, enc, mask = (torch.from_numpy(a).cuda() for a in synth.make_inputs(B, 80, T, L, seed=4321))
    ns = dpm_solver.NoiseScheduleVP("discrete", betas=torch.from_numpy(synth.make_betas()))
    native = dpm_solver.NativeUNetModel(m, cond, enc, mask)
    if args.mode == "guided":
        fn = dpm_solver.model_wrapper(native, ns, model_type="x_start", guidance_type="classifier-free", condition=enc,
                                      unconditional_condition=torch.zeros_like(enc), guidance_scale=2.0)
    else:
        fn = dpm_solver.model_wrapper(native, ns, model_type="x_start")
    solver = dpm_solver.DPM_Solver(fn, ns, algorithm_type="dpmsolver++")
    times = []
    with torch.no_grad():
        out = solver.sample(x, steps=steps, order=2, skip_type="time_uniform")
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        for _ in range(args.runs):
            t0 = time.perf_counter()
            solver.sample(x, steps=steps, order=2, skip_type="time_uniform")
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
    eng = m.hip_engine()
    launches = eng.stats()[0]
    nodes = None
    (plan,) = solver._plans.values()
    if hasattr(plan, "graph_nodes"):
        plans = [q for g in plan._guided.values() for q in g._per_shape.values()] if args.mode == "guided" else list(plan._per_shape.values())
        nodes = max(q.graph_nodes() for q in plans)
    print(json.dumps(dict(label=args.label, mode=args.mode, B=B, engine_rows=eng._cur.prepared[0], T=T, L=L, evaluations=steps,
                          runs=args.runs, ms=round(sorted(times)[len(times) // 2], 3), min_ms=round(min(times), 3),
                          max_ms=round(max(times), 3), unet_launches_per_forward=launches, graph_nodes=nodes,
                          graph_nodes_per_evaluation=None if nodes is None else round(nodes / steps, 2))), flush=True)


if __name__ == "__main__":
    main()
