"""Host-side choice of the constants of the guided graph cases (tests/guidance_cases.py GRAPH_CFG_SETS) - the sibling of
tools/sampler_options_sensitivity.py and tools/thresholding_sensitivity.py for classifier-free guidance.  On the CPU oracle
(oracle sampler over the oracle denoiser, cfg1, T = 75, L = 33) it prints, per case:

  effect : guided against unguided (conditional) oracle output, to exceed 100 x GRAPH_BOUND
  plan   : the fp64-compiled plan stepped with torch ops through the mirror's guided wrapper against the oracle
  noise  : the oracle against itself with BOTH halves of every denoiser output perturbed by GRAPH_PERTURBATION (guidance
           amplifies a denoiser error by up to |1 - g| + |g|)

A case is kept only if the effect holds and plan and noise stay within a third of GRAPH_BOUND; otherwise soften it (smaller g,
larger t_end) or drop it.  Usage: python tools/guidance_sensitivity.py [report file]   (default: profiles/sampler_guidance_host.txt)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from conftest import oracle_cfg, rel_l2, unet_case  # noqa: E402
from oracle import sampler_ref  # noqa: E402
import guidance_cases as gc  # noqa: E402
import sampler_cases as sc  # noqa: E402
import thresholding_cases as tc  # noqa: E402


def main(argv):
    path = argv[0] if argv else os.path.join(ROOT, "profiles", "sampler_guidance_host.txt")
    kw, sd, *_ = unet_case("cfg1")
    sd = {k: torch.from_numpy(v) for k, v in sd.items()}
    cfg = oracle_cfg(kw)
    lines = ["# classifier-free guidance in the sampler graph: host figures of tests/guidance_cases.py GRAPH_CFG_SETS "
             "(tools/guidance_sensitivity.py)",
             "# limits: effect > %.1e, plan and noise <= %.2e (a third of GRAPH_BOUND = %.0e); perturbation %.1e on both halves"
             % (100 * sc.GRAPH_BOUND, sc.GRAPH_BOUND / 3, sc.GRAPH_BOUND, sc.GRAPH_PERTURBATION)]
    print("\n".join(lines), flush=True)
    ok = True
    with torch.no_grad():
        for name, family, ctor, skw, B, g, uncond, thr in gc.GRAPH_CFG_SETS:
            x, cond, enc, mask, uenc, umask = gc.graph_inputs(B, uncond)
            gen = torch.Generator().manual_seed(99)

            def noisy(y):
                n = torch.randn(y.shape, generator=gen)
                return y + n * (sc.GRAPH_PERTURBATION * y.norm() / n.norm())

            x0_fn = (lambda v, t=None: sampler_ref.dynamic_thresholding(v, tc.GRAPH_THR_RATIO, tc.GRAPH_THR_MAX)) if thr else None
            clean = gc.oracle_pair_model(sd, cfg, cond, mask, umask)
            ref = gc.oracle_guided_sample(family, ctor, skw, clean, x, enc, uenc, g, x0_fn)
            plain = gc.oracle_guided_sample(family, ctor, skw, clean, x, enc, uenc, 1.0, x0_fn)
            pert = gc.oracle_guided_sample(family, ctor, skw, gc.oracle_pair_model(sd, cfg, cond, mask, umask, noisy), x, enc, uenc, g,
                                           x0_fn)
            thr_ctor = dict(correcting_x0_fn="dynamic_thresholding", dynamic_thresholding_ratio=tc.GRAPH_THR_RATIO,
                            thresholding_max_val=tc.GRAPH_THR_MAX) if thr else {}
            solver, _, _ = gc.make_guided_solver(family, lambda xx, t, c=None, **k: clean(xx, t, c), enc, uenc, g, **thr_ctor, **ctor)
            mirror = solver.sample(x.clone(), **skw)
            e_eff, e_plan, e_noise = (rel_l2(plain.numpy(), ref.numpy()), rel_l2(mirror.numpy(), ref.numpy()),
                                      rel_l2(pert.numpy(), ref.numpy()))
            good = e_eff > 100 * sc.GRAPH_BOUND and max(e_plan, e_noise) <= sc.GRAPH_BOUND / 3
            ok &= good
            line = ("host  %-14s B %d g %.2f uncond %-6s thr %d  effect %.3e  plan %.3e  noise %.3e   %s"
                    % (name, B, g, uncond, int(thr), e_eff, e_plan, e_noise, "kept" if good else "OVER"))
            print(line, flush=True)
            lines.append(line)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
