#!/usr/bin/env python3
"""tests/golden/sampler_thresholding.npz: the reference's DPM_Solver.sample / UniPC.sample (imported, build container only) with
correcting_x0_fn='dynamic_thresholding' (ratio 0.9, max 0.6) and no correcting_xt_fn, on the analytic stand-in network - the
cases of tests/thresholding_cases.py STANDIN_CASES, which tests/test_gpu_thresholding.py runs through the native loop.
Per case: `<key>_x` (the reference's final x), `<key>_seed` (the synth.normal seed and tag of the start point) and `<key>_kw`
(the keywords, as text); only outputs, seeds and keywords.  The reference accepted every one of these combinations.
Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_sampler_thr.py [--ref /root/reference]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import diff_vits_amd  # noqa: E402,F401
from diff_vits_amd import synth  # noqa: E402
from oracle import sampler_ref  # noqa: E402
import thresholding_cases as tc  # noqa: E402


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
    hook = dict(correcting_x0_fn="dynamic_thresholding", dynamic_thresholding_ratio=tc.THR_RATIO, thresholding_max_val=tc.THR_MAX)
    out = {}
    for key, (family, ctor, kw) in tc.STANDIN_CASES.items():
        x = tc.standin_x(key)
        kw = dict(kw)
        method = kw.pop("method", "multistep")
        if family == "dpm":
            ns = ref_dpm.NoiseScheduleVP("discrete", betas=betas)
            fn = ref_dpm.model_wrapper(lambda xx, t, **k: sampler_ref.standin_model(xx, t), ns, model_type="x_start")
            r = ref_dpm.DPM_Solver(fn, ns, algorithm_type=ctor.get("algorithm_type", "dpmsolver++"), **hook).sample(x.clone(), method=method, **kw)
        else:
            ns = ref_unipc.NoiseScheduleVP("discrete", betas=betas)
            fn = ref_unipc.model_wrapper(lambda xx, t, **k: sampler_ref.standin_model(xx, t), ns, model_type="x_start")
            r = ref_unipc.UniPC(fn, ns, variant=ctor["variant"], algorithm_type=ctor.get("algorithm_type", "data_prediction"),
                                **hook).sample(x.clone(), method="multistep", **kw)
        o, plain = tc.standin_oracle(key), tc.standin_oracle(key, thresholded=False)
        out[key + "_x"] = r.numpy()
        out[key + "_seed"] = np.array("1234 thr." + key)
        out[key + "_kw"] = np.array(repr((family, ctor, tc.STANDIN_CASES[key][2])))
        print("%-14s oracle vs reference %.2e   thresholded vs plain oracle %.2e   tolerance %.0e"
              % (key, rel(o.numpy(), r.numpy()), rel(plain.numpy(), o.numpy()), tc.standin_tolerance(key)))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "sampler_thresholding.npz"), **out)


if __name__ == "__main__":
    main()
