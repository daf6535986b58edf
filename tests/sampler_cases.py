"""Sampler option cases shared by the CPU mirror tests (test_host_mirror.py) and the GPU tests of the native loop
(test_gpu_sampler_options.py): the keys of tests/golden/sampler_options.npz with the keywords that produced them, the
tolerance rule of those keys, and the option sets run through the captured graph."""


# ---- remaining multistep options of DPM_Solver.sample / UniPC.sample (t_start / t_end, denoise_to_zero,
#      return_intermediate) against the reference's outputs (tools/make_golden_sampler_opts.py) -------------------------
OPTION_CASES = {
    "dpm_window": ("dpm", dict(steps=12, order=2, skip_type="time_uniform", t_start=0.8, t_end=0.05)),
    "dpm_dtz_logsnr": ("dpm", dict(steps=8, order=3, skip_type="logSNR", denoise_to_zero=True)),
    "dpm_inter_quad": ("dpm", dict(steps=10, order=2, skip_type="time_quadratic", return_intermediate=True)),
    "dpm_all": ("dpm", dict(steps=9, order=2, skip_type="time_uniform", t_start=0.95, t_end=0.01, denoise_to_zero=True,
                            return_intermediate=True)),
    "unipc_window_dtz": ("unipc", dict(steps=10, order=2, skip_type="time_uniform", t_start=0.9, t_end=0.02, denoise_to_zero=True,
                                        return_intermediate=True)),
    "unipc_o3_logsnr": ("unipc", dict(steps=7, order=3, skip_type="logSNR", t_end=0.004)),
    # continuous-time schedules (NoiseScheduleVP('linear' | 'cosine'); dpm_solver.py knows 'linear' only)
    "dpm_linear": ("dpm", dict(steps=10, order=2, skip_type="time_uniform", schedule=("linear", 0.1, 20.0))),
    "dpm_linear_logsnr_dtz": ("dpm", dict(steps=8, order=3, skip_type="logSNR", denoise_to_zero=True, return_intermediate=True,
                                          schedule=("linear", 0.1, 20.0))),
    "unipc_linear_quad": ("unipc", dict(steps=9, order=2, skip_type="time_quadratic", t_end=0.01, schedule=("linear", 0.2, 15.0))),
    "unipc_cosine": ("unipc", dict(steps=10, order=2, skip_type="time_uniform", return_intermediate=True, schedule=("cosine", 0.1, 20.0))),
    "unipc_cosine_logsnr": ("unipc", dict(steps=8, order=3, skip_type="logSNR", schedule=("cosine", 0.1, 20.0))),
    # algorithm_type='dpmsolver': the multistep updates on the noise prediction (dpm_solver.py:581-592, 841-847, 895-904)
    "dpmn_o1": ("dpm", dict(steps=10, order=1, skip_type="time_uniform", algorithm_type="dpmsolver")),
    "dpmn_o2_dtz": ("dpm", dict(steps=12, order=2, skip_type="time_quadratic", denoise_to_zero=True, return_intermediate=True,
                                algorithm_type="dpmsolver")),
    "dpmn_o3_logsnr": ("dpm", dict(steps=8, order=3, skip_type="logSNR", algorithm_type="dpmsolver")),
    "dpmn_o3_window": ("dpm", dict(steps=20, order=3, skip_type="time_uniform", t_start=0.9, t_end=0.02, algorithm_type="dpmsolver")),
    "dpmn_linear": ("dpm", dict(steps=9, order=2, skip_type="time_uniform", schedule=("linear", 0.1, 20.0), algorithm_type="dpmsolver")),
    # correcting_x0_fn ("thr": dynamic thresholding, ratio 0.9 / max 0.6; "fn": sampler_ref.standin_x0_fix) and correcting_xt_fn
    # (sampler_ref.standin_xt_fix): dpm_solver.py:409-425, 443-444, 1180-1238; uni_pc.py:256-277, 292-293, 615-665
    "dpm_thr_xt": ("dpm", dict(steps=10, order=2, skip_type="time_uniform", denoise_to_zero=True, return_intermediate=True,
                               hooks=("thr", True))),
    "dpm_x0fn": ("dpm", dict(steps=8, order=3, skip_type="logSNR", hooks=("fn", False))),
    "dpmn_thr_xt_dtz": ("dpm", dict(steps=9, order=2, skip_type="time_uniform", denoise_to_zero=True, algorithm_type="dpmsolver",
                                    hooks=("thr", True))),
    "unipc_thr_xt": ("unipc", dict(steps=10, order=2, skip_type="time_uniform", denoise_to_zero=True, return_intermediate=True,
                                   hooks=("thr", True))),
    "unipc_x0fn_o3": ("unipc", dict(steps=8, order=3, skip_type="time_quadratic", hooks=("fn", True))),
    # model_wrapper(guidance_type='classifier-free' | 'classifier', ...) (dpm_solver.py:282-330) on the conditional stand-in
    "dpm_cfg": ("dpm", dict(steps=10, order=2, skip_type="time_uniform", guidance="cfg")),
    "dpm_cfg_scale1": ("dpm", dict(steps=8, order=3, skip_type="logSNR", guidance="cfg1")),
    "dpm_classifier": ("dpm", dict(steps=10, order=2, skip_type="time_quadratic", denoise_to_zero=True, guidance="clf")),
    # solver_type='taylor' (the second-order update's Taylor form, dpm_solver.py:825-829, 848-851)
    "dpm_taylor": ("dpm", dict(steps=10, order=2, skip_type="time_uniform", solver_type="taylor")),
    "dpmn_taylor": ("dpm", dict(steps=12, order=2, skip_type="logSNR", solver_type="taylor", algorithm_type="dpmsolver")),
    # method='singlestep' ("DPM-Solver-fast": the evaluations shared out over outer steps of order <= order) and
    # 'singlestep_fixed' (dpm_solver.py:482-539, 594-794, 1214-1232)
    "dpm_ss_o3": ("dpm", dict(steps=12, order=3, skip_type="time_uniform", method="singlestep")),
    "dpm_ss_o2_logsnr_dtz": ("dpm", dict(steps=9, order=2, skip_type="logSNR", denoise_to_zero=True, return_intermediate=True,
                                         method="singlestep", hooks=(None, True))),
    "dpmn_ss_o3_quad": ("dpm", dict(steps=11, order=3, skip_type="time_quadratic", method="singlestep", algorithm_type="dpmsolver")),
    "dpm_ssfixed_taylor": ("dpm", dict(steps=12, order=3, skip_type="time_uniform", method="singlestep_fixed", solver_type="taylor")),
    "dpmn_ss_taylor_o2": ("dpm", dict(steps=10, order=2, skip_type="time_uniform", method="singlestep", solver_type="taylor",
                                      algorithm_type="dpmsolver")),
    # UniPC(algorithm_type='noise_prediction') (uni_pc.py:266, 448-468, 569-587)
    "unipcn_bh2_o2": ("unipc", dict(steps=10, order=2, skip_type="time_uniform", unipc_algo="noise_prediction")),
    "unipcn_bh1_o3_dtz": ("unipc", dict(steps=9, order=3, skip_type="time_quadratic", denoise_to_zero=True, return_intermediate=True,
                                        unipc_algo="noise_prediction", variant="bh1", hooks=("fn", True))),
    "unipcn_vary_o4": ("unipc", dict(steps=9, order=4, skip_type="time_uniform", unipc_algo="noise_prediction", variant="vary_coeff")),
    # method='adaptive' (dpm_solver.py:906-1010; `steps` is ignored).  Step sizes follow an error estimate: where that estimate
    # is at rounding level (e.g. a first step from t_start < T on this smooth stand-in: E ~ 4e-7) the next step size amplifies the
    # rounding and two float32 / fp64 evaluations of the schedule part ways - the float32 oracle still reproduces the reference
    # bit for bit there; the cases below keep every estimate well above rounding
    "dpm_adaptive_o2": ("dpm", dict(steps=20, order=2, skip_type="time_uniform", method="adaptive")),
    "dpm_adaptive_o3_tight": ("dpm", dict(steps=20, order=3, skip_type="time_uniform", method="adaptive", atol=0.002, rtol=0.02,
                                          denoise_to_zero=True)),
    # (x_start network, order 3, loose tolerance: the accept / reject decisions sit close to E = 1 - the case that exposed the
    # skipped x0 -> noise -> x0 round trip in round 4's adaptive path)
    "dpm_adaptive_o3_loose": ("dpm", dict(steps=20, order=3, skip_type="time_uniform", method="adaptive", atol=0.01)),
    "dpmn_adaptive_o2": ("dpm", dict(steps=20, order=2, skip_type="time_uniform", method="adaptive", algorithm_type="dpmsolver")),
    "dpmn_adaptive_o3_taylor": ("dpm", dict(steps=20, order=3, skip_type="time_uniform", method="adaptive", solver_type="taylor",
                                            algorithm_type="dpmsolver", t_end=0.01)),
    # the other model types of model_wrapper (dpm_solver.py:288-298): the stand-in's output read as noise / v / score
    "dpm_type_noise": ("dpm", dict(steps=10, order=2, skip_type="time_uniform", guidance="type:noise")),
    "dpm_type_v": ("dpm", dict(steps=10, order=3, skip_type="logSNR", guidance="type:v")),
    "dpmn_type_score": ("dpm", dict(steps=10, order=2, skip_type="time_quadratic", guidance="type:score", algorithm_type="dpmsolver")),
}


def option_tolerance(sched, method="multistep", algo="dpmsolver++", ualgo="data_prediction"):
    """Relative-L2 bound of a compiled plan (fp64 tables, float32 updates) against the reference's outputs."""
    # the mirror compiles the loop in fp64; the reference evaluates the continuous schedules' closed forms in float32, where
    # sigma = sqrt(1 - exp(2 log alpha)) loses ~4 digits near t_end (log alpha ~ -5e-5): the agreement is the reference's
    # own rounding there (the float32 oracle reproduces the reference exactly)
    tol = 2e-5 if sched is None else 5e-4
    if method == "adaptive":    # step sizes from error estimates: one more amplification of the schedule's rounding
        tol = max(tol, 2e-4)
    if algo == "dpmsolver" or ualgo == "noise_prediction":     # the noise form: eps = (x - alpha x0) / sigma in float32 amplifies rounding by 1 / sigma at the low-noise end
        tol = max(tol, 1e-4)
    return tol


def native_option_keys():
    """The keys the native plan expresses without Python around it: no correction hooks, no guided / typed wrapper (those take
    the generic noise-prediction path), no data-dependent step sizes."""
    return sorted(k for k, (_, kw) in OPTION_CASES.items()
                  if "hooks" not in kw and "guidance" not in kw and kw.get("method") != "adaptive")


def split_option_case(key):
    """(solver family, schedule, algorithm_type, UniPC algorithm_type, UniPC variant, method, sample() keywords) of a key."""
    solver, kw = OPTION_CASES[key]
    kw = dict(kw)
    sched = kw.pop("schedule", None)
    algo = kw.pop("algorithm_type", "dpmsolver++")
    method = kw.pop("method", "multistep")
    ualgo, variant = kw.pop("unipc_algo", "data_prediction"), kw.pop("variant", "bh2")
    return solver, sched, algo, ualgo, variant, method, kw


# ---- option sets run through the captured graph (dv_sampler_run) on the cfg1 denoiser, B = 2, T = 75, L = 33, against the
#      oracle sampler over the oracle denoiser at the project's 5e-4.  (name, solver family, constructor keywords, sample()
#      keywords.)  steps / t_end are chosen so that the comparison itself stays inside a third of that bound on the host
#      (tools/sampler_options_sensitivity.py, figures in profiles/sampler_options_gpu.txt): the float32 oracle against the
#      fp64-compiled plan on the same denoiser, and the oracle against itself with every denoiser output perturbed by Gaussian
#      noise of relative size 3.5e-5 (the largest forward error of the denoiser on record, GPUTEST_r06.json).  The noise forms
#      amplify both by 1 / sigma at the low-noise end, so they stop at a larger t_end.
GRAPH_BOUND = 5e-4
GRAPH_SHAPE = (2, 75, 33)          # B, T, L
GRAPH_PERTURBATION = 3.5e-5
GRAPH_OPTION_SETS = [
    ("window_dtz", "dpm", {}, dict(steps=8, order=2, skip_type="time_uniform", t_start=0.8, t_end=0.05, denoise_to_zero=True)),
    ("ss_o3_logsnr", "dpm", {}, dict(steps=7, order=3, skip_type="logSNR", method="singlestep", t_end=0.01)),
    # (logSNR grid: on the time_uniform one the third-order Taylor form turns the perturbation into 2.6e-4 - over the limit)
    ("ssfixed_taylor", "dpm", {}, dict(steps=6, order=3, skip_type="logSNR", method="singlestep_fixed", solver_type="taylor",
                                       t_end=0.01)),
    ("dpmn_o2", "dpm", dict(algorithm_type="dpmsolver"), dict(steps=8, order=2, skip_type="time_uniform", t_end=0.1)),
    # (9 steps: with 6 - orders 3, 2, 1 over three long outer steps - the plan's folded float32 coefficients and the oracle's
    # float32 order of operations already part by 2.5e-4 on the host)
    ("dpmn_ss", "dpm", dict(algorithm_type="dpmsolver"), dict(steps=9, order=3, skip_type="time_quadratic", method="singlestep",
                                                              t_end=0.1)),
    ("linear", "dpm", dict(schedule=("linear", 0.1, 20.0)), dict(steps=8, order=2, skip_type="time_uniform", t_end=0.05)),
    ("cosine_unipc_o3", "unipc", dict(schedule=("cosine", 0.1, 20.0)), dict(steps=8, order=3, skip_type="time_uniform", t_end=0.05)),
    ("unipcn_vary_o4", "unipc", dict(algorithm_type="noise_prediction", variant="vary_coeff"),
     dict(steps=8, order=4, skip_type="time_uniform", t_end=0.1)),
]


def make_solver(family, model, schedule=None, **ctor):
    """DPM_Solver / UniPC around `model` (an x0-prediction network (x, t_input), or a NativeUNetModel) as the product builds
    them; returns (solver, noise schedule)."""
    import torch
    from diff_vits_amd import synth
    from diff_vits_amd.sampler import dpm_solver, uni_pc
    mod = dpm_solver if family == "dpm" else uni_pc
    ns = (mod.NoiseScheduleVP("discrete", betas=torch.from_numpy(synth.make_betas())) if schedule is None else
          mod.NoiseScheduleVP(schedule[0], continuous_beta_0=schedule[1], continuous_beta_1=schedule[2]))
    fn = mod.model_wrapper(model, ns, model_type="x_start")
    return (mod.DPM_Solver(fn, ns, **ctor) if family == "dpm" else mod.UniPC(fn, ns, **{"variant": "bh2", **ctor})), ns


def oracle_sample(family, model, x, schedule=None, algorithm_type=None, variant="bh2", **kw):
    """The oracle's sampler (oracle/sampler_ref.py, pinned to the reference at 1e-6) for the same keywords."""
    import torch
    from diff_vits_amd import synth
    from oracle import sampler_ref
    kw = dict(kw)
    args = (kw.pop("steps"), kw.pop("order"), kw.pop("skip_type"))
    betas = torch.from_numpy(synth.make_betas())
    if family == "dpm":
        return sampler_ref.dpm_solver_pp_sample(model, betas, x, *args, schedule=schedule,
                                                algorithm_type=algorithm_type or "dpmsolver++", **kw)
    return sampler_ref.unipc_sample(model, betas, x, *args, variant, schedule=schedule,
                                    algorithm_type=algorithm_type or "data_prediction", **kw)
