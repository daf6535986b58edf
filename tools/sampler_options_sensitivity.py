"""Host-side sensitivity of the graph option sets (tests/sampler_cases.py GRAPH_OPTION_SETS) before they go to the GPU:
how far the comparison of tests/test_gpu_sampler_options.py moves without any kernel in it.

  plan   : the fp64-compiled plan stepped with torch ops (Plan.run_python) over the oracle denoiser, against the oracle's
           float32 sampler over the same denoiser - the two restatements of the schedule arithmetic
  noise  : the oracle sampler over the oracle denoiser with every output perturbed by Gaussian noise of relative size
           GRAPH_PERTURBATION, against the unperturbed run - what a denoiser error of that size becomes at the end

A set is kept only if both stay within a third of GRAPH_BOUND.  Usage: python tools/sampler_options_sensitivity.py [name ...]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from conftest import oracle_cfg, rel_l2, unet_case  # noqa: E402
from diff_vits_amd import synth  # noqa: E402
from oracle import unet_ref  # noqa: E402
import sampler_cases as sc  # noqa: E402


def main(names):
    kw, sd, *_ = unet_case("cfg1")
    B, T, L = sc.GRAPH_SHAPE
    x, cond, enc, mask = (torch.from_numpy(a) for a in synth.make_inputs(B, 80, T, L, seed=4242, ragged_mask=True))
    model = unet_ref.diffusion_model_fn({k: torch.from_numpy(v) for k, v in sd.items()}, oracle_cfg(kw), cond, enc, mask)
    gen = torch.Generator().manual_seed(99)

    def noisy(xx, t):
        y = model(xx, t)
        n = torch.randn(y.shape, generator=gen)
        return y + n * (sc.GRAPH_PERTURBATION * y.norm() / n.norm())

    print("# %-16s %10s %10s   limit %.2e (a third of %.0e)" % ("option set", "plan", "noise", sc.GRAPH_BOUND / 3, sc.GRAPH_BOUND))
    ok = True
    with torch.no_grad():
        for name, family, ctor, skw in sc.GRAPH_OPTION_SETS:
            if names and name not in names:
                continue
            ctor = dict(ctor)
            sched = ctor.pop("schedule", None)
            solver, _ = sc.make_solver(family, lambda xx, t, **k: model(xx, t), sched, **ctor)
            mirror = solver.sample(x.clone(), **skw)
            okw = dict(algorithm_type=ctor.get("algorithm_type"), variant=ctor.get("variant", "bh2"))
            ref = sc.oracle_sample(family, model, x.clone(), sched, **okw, **skw)
            pert = sc.oracle_sample(family, noisy, x.clone(), sched, **okw, **skw)
            e_plan, e_noise = rel_l2(mirror.numpy(), ref.numpy()), rel_l2(pert.numpy(), ref.numpy())
            good = max(e_plan, e_noise) <= sc.GRAPH_BOUND / 3
            ok &= good
            print("  %-16s %10.3e %10.3e   %s" % (name, e_plan, e_noise, "kept" if good else "OVER"), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
