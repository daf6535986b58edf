"""Host-side choice of the dynamic-thresholding constants of the graph cases (tests/thresholding_cases.py GRAPH_THR_SETS) - the
sibling of tools/sampler_options_sensitivity.py for correcting_x0_fn='dynamic_thresholding'.  On the CPU oracle (oracle sampler
over the oracle denoiser, cfg1 at GRAPH_SHAPE) it prints, per case:

  evals  : in how many evaluations the quantile of |x0| exceeds max_val (the clamp then cuts elements), of how many    - (a)
  effect : thresholded against plain output, to exceed 100 x GRAPH_BOUND                                                - (b)
  plan   : the fp64-compiled plan stepped with torch ops (the mirror, thresholding as its x0 hook) against the oracle
  noise  : the oracle against itself with every denoiser output perturbed by GRAPH_PERTURBATION                          - (c)

A case is kept only if (a) holds in at least half of the evaluations, (b) holds, and plan and noise stay within a third of
GRAPH_BOUND.  Usage: python tools/thresholding_sensitivity.py [ratio max_val]   (default: the constants of the test)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from conftest import oracle_cfg, rel_l2, unet_case  # noqa: E402
from diff_vits_amd import synth  # noqa: E402
from oracle import sampler_ref, unet_ref  # noqa: E402
import sampler_cases as sc  # noqa: E402
import thresholding_cases as tc  # noqa: E402


def main(argv):
    ratio, max_val = (float(argv[0]), float(argv[1])) if len(argv) == 2 else (tc.GRAPH_THR_RATIO, tc.GRAPH_THR_MAX)
    kw, sd, *_ = unet_case("cfg1")
    B, T, L = sc.GRAPH_SHAPE
    x, cond, enc, mask = (torch.from_numpy(a) for a in synth.make_inputs(B, 80, T, L, seed=4242, ragged_mask=True))
    model = unet_ref.diffusion_model_fn({k: torch.from_numpy(v) for k, v in sd.items()}, oracle_cfg(kw), cond, enc, mask)
    gen = torch.Generator().manual_seed(99)

    def noisy(xx, t):
        y = model(xx, t)
        n = torch.randn(y.shape, generator=gen)
        return y + n * (sc.GRAPH_PERTURBATION * y.norm() / n.norm())

    seen = []

    def thr(v, t=None):
        q = torch.quantile(v.abs().reshape(v.shape[0], -1), ratio, dim=1)
        seen.append((float(q.min()), float(q.max()), int((v.abs() > torch.clamp(q, min=max_val).reshape(-1, 1, 1)).sum())))
        return sampler_ref.dynamic_thresholding(v, ratio, max_val)

    print("# dynamic thresholding ratio %g max_val %g; limits: effect > %.1e, plan and noise <= %.2e (a third of %.0e)"
          % (ratio, max_val, 100 * sc.GRAPH_BOUND, sc.GRAPH_BOUND / 3, sc.GRAPH_BOUND))
    ok = True
    with torch.no_grad():
        for name, family, ctor, skw in tc.GRAPH_THR_SETS:
            okw = dict(algorithm_type=ctor.get("algorithm_type"), variant=ctor.get("variant", "bh2"))
            plain = sc.oracle_sample(family, model, x.clone(), None, **okw, **skw)
            del seen[:]
            ref = sc.oracle_sample(family, model, x.clone(), None, x0_fn=thr, **okw, **skw)
            evals = list(seen)
            pert = sc.oracle_sample(family, noisy, x.clone(), None, x0_fn=lambda v, t=None: sampler_ref.dynamic_thresholding(v, ratio, max_val),
                                    **okw, **skw)
            solver, _ = sc.make_solver(family, lambda xx, t, **k: model(xx, t), None, correcting_x0_fn="dynamic_thresholding",
                                       dynamic_thresholding_ratio=ratio, thresholding_max_val=max_val, **ctor)
            mirror = solver.sample(x.clone(), **skw)
            above = [e for e in evals if e[0] > max_val]          # every row's quantile above max_val
            clamped = all(e[2] > 0 for e in above)
            e_eff, e_plan, e_noise = (rel_l2(plain.numpy(), ref.numpy()), rel_l2(mirror.numpy(), ref.numpy()),
                                      rel_l2(pert.numpy(), ref.numpy()))
            good = (2 * len(above) >= len(evals) and clamped and e_eff > 100 * sc.GRAPH_BOUND
                    and max(e_plan, e_noise) <= sc.GRAPH_BOUND / 3)
            ok &= good
            print("  %-14s evals %d of %d above max_val (quantiles %.3f .. %.3f)  effect %.3e  plan %.3e  noise %.3e   %s"
                  % (name, len(above), len(evals), min(e[0] for e in evals), max(e[1] for e in evals), e_eff, e_plan, e_noise,
                     "kept" if good else "OVER"), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
