#!/usr/bin/env python3
"""tests/golden/sampler_known_frames.npz: the reference's DPM_Solver.sample / UniPC.sample (imported, build container only) with
    correcting_xt_fn = lambda x, t, step: where(keep, alpha(t) * known + sigma(t) * eps, x)
(alpha / sigma: the reference schedule's marginal_alpha / marginal_std) on the cases of tests/known_frames_cases.py - the
frame-mixing analytic stand-in network at x [2, 5, 24], a mask per row (UniPC: row by row, its wrapper only broadcasts at
B = 1).  Per case: `<key>_x` (the reference's final x), `<key>_inter` (what its return_intermediate collects), `<key>_seed` (the synth.normal seed and tags of x / known / eps) and `<key>_kw` (the keywords,
as text); only outputs, seeds and keywords.  Prints, per key, the distance between the corrected and the uncorrected reference
result: it must exceed 100 x the key's tolerance (tests/test_known_frames_cpu.py asserts it).
Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_known_frames.py [--ref /root/reference]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import diff_vits_amd  # noqa: E402,F401
from diff_vits_amd import synth  # noqa: E402
import known_frames_cases as kc  # noqa: E402


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    sys.path.insert(0, args.ref)
    from sampler import dpm_solver as ref_dpm, uni_pc as ref_unipc
    torch.set_grad_enabled(False)
    betas = torch.from_numpy(synth.make_betas())
    out = {}
    for key, (family, ctor, kw) in kc.CASES.items():
        x, known, eps, keep = kc.case_x(key), kc.case_known(key), kc.case_eps(key), kc.case_keep(key)[:, None, :]
        kw = dict(kw)
        method = kw.pop("method", "multistep")
        mod = ref_dpm if family == "dpm" else ref_unipc
        ns = mod.NoiseScheduleVP("discrete", betas=betas)
        fn = mod.model_wrapper(lambda xx, t, **k: kc.kf_model(xx, t), ns, model_type="x_start")

        def hook(v, t, step):
            return torch.where(keep, ns.marginal_alpha(t) * known + ns.marginal_std(t) * eps, v)

        def run(xt_fn):
            if family == "dpm":
                s = ref_dpm.DPM_Solver(fn, ns, algorithm_type=ctor.get("algorithm_type", "dpmsolver++"), correcting_xt_fn=xt_fn)
            else:
                s = ref_unipc.UniPC(fn, ns, variant=ctor["variant"], algorithm_type=ctor.get("algorithm_type", "data_prediction"),
                                    correcting_xt_fn=xt_fn)
            return s.sample(x.clone(), method=method, return_intermediate=True, **kw)

        if family == "unipc":
            # the reference's UniPC 'x_start' wrapper multiplies alpha_t [B] into [B, C, T] (uni_pc.py:189-191): it only
            # broadcasts at B = 1.  UniPC treats every row on its own, so the rows are run one by one and stacked
            rows = []
            for b in range(x.shape[0]):
                x, known, eps, keep = (v[b:b + 1] for v in (kc.case_x(key), kc.case_known(key), kc.case_eps(key), kc.case_keep(key)[:, None, :]))
                rows.append((run(hook), run(None)))
            r, plain = (torch.cat([row[i][0] for row in rows]) for i in (0, 1))
            inter = [torch.cat([row[0][1][k] for row in rows]) for k in range(len(rows[0][0][1]))]
        else:
            (r, inter), (plain, _) = run(hook), run(None)
        out[key + "_x"] = r.numpy()
        out[key + "_inter"] = torch.stack(list(inter)).numpy()
        out[key + "_seed"] = np.array("1234 kf.x.%s kf.known.%s kf.eps.%s" % (key, key, key))
        out[key + "_kw"] = np.array(repr(kc.CASES[key]))
        o, _ = kc.restate(key)
        print("%-12s corrected vs uncorrected reference %.2e   fp64 restatement vs reference %.2e   tolerance %.0e   intermediates %d"
              % (key, rel(plain.numpy(), r.numpy()), rel(o.numpy(), r.numpy()), kc.tolerance(key), len(inter)))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "sampler_known_frames.npz"), **out)


if __name__ == "__main__":
    main()
