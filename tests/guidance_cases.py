"""Cases of the classifier-free guidance tests (test_gpu_guidance.py), shared with the host-side choice of the graph cases'
constants (tools/guidance_sensitivity.py; figures in profiles/sampler_guidance_host.txt)."""
import numpy as np

# ---- the operator (dv_op_cfg_combine): pair [2 rows, n] -> [rows, n]
OP_ROWS = (1, 3)
OP_NUMELS = (1, 2, 3, 255, 256, 257, 4097, 6000)
OP_SCALES = (0.0, 0.5, 2.5, 7.0, -1.0)


def op_data(rows, n):
    """The 2 rows x n predictions of an operator case: unconditional rows first."""
    from diff_vits_amd import synth
    return synth.normal(91, "cfg.pair.%d.%d" % (rows, n), (2 * rows, n)).astype(np.float32)


def op_ref(pair, rows, g):
    """Host emulation of the stated arithmetic: d = c - u in float32, then g * d + u in float64 rounded to float32."""
    u, c = pair[:rows].astype(np.float32), pair[rows:].astype(np.float32)
    d = (c - u).astype(np.float32)
    return (np.float64(np.float32(g)) * d.astype(np.float64) + u.astype(np.float64)).astype(np.float32)


# ---- the captured graph around the real denoiser (cfg1, T = 75, L = 33, ragged prompt mask) under guidance:
#      (name, solver family, constructor keywords, sample() keywords, B, guidance scale, unconditional condition, thresholded).
#      B = 2 is sampler_cases.GRAPH_SHAPE; B = 3 an odd batch, B = 1 the smallest pair (2B = 2); T = 75 is no multiple of 32 at
#      any level.  "zeros": all-zero unconditional states under the conditional mask; "random": a second random encoding with a
#      key mask of its own.
#      Guidance amplifies an error of the denoiser by up to |1 - g| + |g|.  g, steps and t_end are chosen on the host
#      (tools/guidance_sensitivity.py, the procedure of sampler_cases.GRAPH_OPTION_SETS): the float32 oracle against the
#      fp64-compiled plan stepped with torch ops, and the oracle against itself with BOTH halves of every denoiser output
#      perturbed at sampler_cases.GRAPH_PERTURBATION, must stay inside a third of GRAPH_BOUND; the guided and the unguided
#      oracle outputs must differ by more than 100 x GRAPH_BOUND (a graph that dropped the guidance cannot pass).
GRAPH_T, GRAPH_L = 75, 33
GRAPH_CFG_SETS = [
    ("cfg_dpmpp", "dpm", {}, dict(steps=8, order=2, skip_type="time_uniform", t_end=0.05), 2, 2.0, "zeros", False),
    ("cfg_unipc_bh2", "unipc", dict(variant="bh2"), dict(steps=8, order=2, skip_type="time_uniform", t_end=0.05), 3, 2.0, "zeros", False),
    ("cfg_dpmn", "dpm", dict(algorithm_type="dpmsolver"), dict(steps=8, order=2, skip_type="time_uniform", t_end=0.1), 1, 1.5, "zeros",
     False),
    ("cfg_thr_dpmpp", "dpm", {}, dict(steps=8, order=2, skip_type="time_uniform", t_end=0.05), 2, 2.0, "random", True),
]


def graph_set(name):
    return next(s for s in GRAPH_CFG_SETS if s[0] == name)


def graph_inputs(B, uncond):
    """(x, cond, enc, mask, uncond_enc, uncond_mask) as torch CPU tensors."""
    import torch
    from diff_vits_amd import synth
    x, cond, enc, mask = (torch.from_numpy(a) for a in synth.make_inputs(B, 80, GRAPH_T, GRAPH_L, seed=4242, ragged_mask=True))
    if uncond == "zeros":
        return x, cond, enc, mask, torch.zeros_like(enc), mask.clone()
    uenc = torch.from_numpy(synth.normal(4243, "uncond.enc", tuple(enc.shape)))
    umask = torch.ones_like(mask)
    for b in range(B):
        umask[b, GRAPH_L - 3 - 5 * b:] = False
    return x, cond, enc, mask, uenc * umask.unsqueeze(-1), umask


def oracle_pair_model(sd, cfg, cond, mask, umask, perturb=None):
    """The oracle denoiser as the reference's guided wrapper calls it: model(x_in [2B], t_in [2B], c_in [2B, L, D]) with the
    channel-concat condition and the masks repeated, unconditional half first.  `perturb(y)` perturbs the 2B outputs."""
    import torch
    from oracle import unet_ref
    cc, mm = torch.cat([cond, cond]), torch.cat([umask, mask])

    def model(x, t_input, c=None):
        if x.shape[0] == cond.shape[0]:          # guidance_scale == 1: one conditional evaluation
            y = unet_ref.diffusion_model_fn(sd, cfg, cond, c, mask)(x, t_input)
        else:
            y = unet_ref.diffusion_model_fn(sd, cfg, cc, c, mm)(x, t_input)
        return y if perturb is None else perturb(y)
    return model


def oracle_guided_sample(family, ctor, skw, pair_model, x, enc, uenc, g, x0_fn=None):
    """The reference for a graph case.  DPM family: the oracle's sampler with its own `guidance=` (the reference's noise-space
    formula).  UniPC: the oracle's sampler takes no guidance - it runs over an x0 model that evaluates the pair and combines
    it in float64."""
    import torch
    from sampler_cases import oracle_sample
    if family == "dpm":
        guidance = dict(guidance_type="classifier-free", condition=enc, unconditional_condition=uenc, guidance_scale=g)
        return oracle_sample(family, pair_model, x.clone(), None, algorithm_type=ctor.get("algorithm_type"), guidance=guidance,
                             x0_fn=x0_fn, **skw)

    def x0_model(xx, t_input):
        if g == 1.0:
            return pair_model(xx, t_input, enc)
        u, c = pair_model(torch.cat([xx, xx]), torch.cat([t_input, t_input]), torch.cat([uenc, enc])).double().chunk(2)
        return (u + g * (c - u)).float()
    return oracle_sample(family, x0_model, x.clone(), None, algorithm_type=ctor.get("algorithm_type"), variant=ctor.get("variant", "bh2"),
                         x0_fn=x0_fn, **skw)


def make_guided_solver(family, model, enc, uenc, g, schedule=None, **ctor):
    """DPM_Solver / UniPC around model_wrapper(model, guidance_type='classifier-free', ...); `model` a NativeUNetModel or any
    x0 network (x, t_input, cond).  Returns (solver, model_fn, noise schedule)."""
    import torch
    from diff_vits_amd import synth
    from diff_vits_amd.sampler import dpm_solver, uni_pc
    mod = dpm_solver if family == "dpm" else uni_pc
    ns = mod.NoiseScheduleVP("discrete", betas=torch.from_numpy(synth.make_betas()))
    fn = mod.model_wrapper(model, ns, model_type="x_start", guidance_type="classifier-free", condition=enc,
                           unconditional_condition=uenc, guidance_scale=g)
    solver = mod.DPM_Solver(fn, ns, **ctor) if family == "dpm" else mod.UniPC(fn, ns, **{"variant": "bh2", **ctor})
    return solver, fn, ns
