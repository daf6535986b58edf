"""Cases of the known-frame correction tests (test_known_frames_cpu.py, test_gpu_known_frames.py), shared with the generator of
tests/golden/sampler_known_frames.npz (tools/make_golden_known_frames.py): one key per route of the event loop, on the analytic
stand-in network at x [2, 5, 24] with a mask per row, and an fp64 restatement of the corrected loop that can plant faults."""
import numpy as np

# (solver family, constructor keywords, sample() keywords)
CASES = {
    "dpmpp_o2": ("dpm", {}, dict(steps=10, order=2, skip_type="time_uniform")),
    "dpmpp_o3": ("dpm", {}, dict(steps=9, order=3, skip_type="logSNR")),
    "dpmn_o2": ("dpm", dict(algorithm_type="dpmsolver"), dict(steps=10, order=2, skip_type="time_uniform")),
    "dpmpp_ss_o3": ("dpm", {}, dict(steps=11, order=3, skip_type="time_uniform", method="singlestep")),
    "dpmpp_dtz": ("dpm", {}, dict(steps=8, order=2, skip_type="time_quadratic", denoise_to_zero=True)),
    "unipc_bh2": ("unipc", dict(variant="bh2"), dict(steps=10, order=2, skip_type="time_uniform")),
    "unipcn_bh2": ("unipc", dict(variant="bh2", algorithm_type="noise_prediction"), dict(steps=9, order=3, skip_type="time_uniform")),
}
SHAPE = (2, 5, 24)
FAULTS = ("no_start", "start_early", "shift", "row0_both", "sigma_prev")


def kf_model(x, t_input):
    """The analytic stand-in network (oracle.sampler_ref.standin_model) behind a fixed mix of neighbouring frames.  The plain
    stand-in is elementwise: no kept frame would ever influence another frame, every kept frame is overwritten by the next
    correction, and a correction at the wrong point of the loop would leave the result unchanged."""
    import torch
    from oracle import sampler_ref
    return sampler_ref.standin_model(0.75 * x + 0.5 * torch.roll(x, 1, dims=-1), t_input)


def _normal(tag, key):
    import torch
    from diff_vits_amd import synth
    return torch.from_numpy(synth.normal(1234, "kf.%s.%s" % (tag, key), SHAPE))


def case_x(key):
    return _normal("x", key)


def case_known(key):
    return 0.8 * _normal("known", key)


def case_eps(key):
    return _normal("eps", key)


def case_keep(key=None):
    """bool [2, 24]: row 0 keeps a prefix, row 1 an interior span that starts and ends off the 4-frame grid."""
    import torch
    keep = torch.zeros(SHAPE[0], SHAPE[2], dtype=torch.bool)
    keep[0, :9] = True
    keep[1, 5:14] = True
    return keep


def tolerance(key):
    from sampler_cases import option_tolerance
    family, ctor, kw = CASES[key]
    algo = ctor.get("algorithm_type", "dpmsolver++") if family == "dpm" else "dpmsolver++"
    ualgo = ctor.get("algorithm_type", "data_prediction") if family == "unipc" else "data_prediction"
    return option_tolerance(None, kw.get("method", "multistep"), algo, ualgo)


def mirror_solver(key, model=None, corrected=True, known_frames=None):
    """(solver, noise schedule, the KnownFrames or None) of this package's mirror for a key."""
    from sampler_cases import make_solver
    from diff_vits_amd.sampler import dpm_solver
    family, ctor, kw = CASES[key]
    solver, ns = make_solver(family, kf_model if model is None else model, None, **ctor)
    kf = None
    if corrected:
        kf = known_frames or dpm_solver.KnownFrames(ns, case_known(key), case_keep(key), case_eps(key))
        solver.correcting_xt_fn = kf
    return solver, ns, kf


def plain_plan(key):
    """The compiled plan of a key (no correction bound)."""
    solver, _, _ = mirror_solver(key, corrected=False)
    family, ctor, kw = CASES[key]
    kw = dict(kw)
    args = (kw.pop("steps"), kw.pop("order"), kw.pop("skip_type"), True, None, None, kw.pop("denoise_to_zero", False))
    return solver._plan(*args, **({"method": kw["method"]} if "method" in kw else {}))


def restate(key, fault=None, corrected=True):
    """The corrected loop of a key restated in fp64 from the plan's events and float32 coefficient rows: (final x, the list the
    reference's return_intermediate collects), float64.  alpha / sigma of a correction come from the mirror's schedule at the
    grid point in fp64.  `fault` plants one of FAULTS."""
    import torch
    plan = plain_plan(key)
    _, ns, _ = mirror_solver(key, corrected=False)
    x = case_x(key).double()
    known, eps, keep = case_known(key).double(), case_eps(key).double(), case_keep(key)[:, None, :]
    if fault == "shift":
        keep = torch.roll(keep, 1, dims=-1)
    elif fault == "row0_both":
        keep = keep[:1].expand_as(keep)
    single = CASES[key][2].get("method", "multistep") != "multistep"
    ts = plan.timesteps

    def coef(k):
        t = torch.tensor([float(ts[min(k, len(ts) - 1)])], dtype=torch.float64)
        return float(ns.marginal_alpha(t)[0]), float(ns.marginal_std(t)[0])

    def fix(v, k):
        if not corrected:
            return v
        a, s = coef(k)
        if fault == "sigma_prev" and k > 0:
            s = coef(k - 1)[1]
        return torch.where(keep, a * known + s * eps, v)

    hist, xp, inter = [None] * plan.n_slots, None, []
    step, seen, pending = 0, False, False

    def finish_start(v):
        if single:
            return v
        if fault not in ("no_start", "start_early"):
            v = fix(v, 0)
        inter.append(v)
        return v

    for typ, src, eidx, dst, ci, s0, s1, s2, s3 in plan.events.tolist():
        if pending and not (typ == 1 and dst >= 2):
            x, pending = finish_start(x), False
        if typ == 0:
            if not seen and fault == "start_early" and not single:
                x = fix(x, 0)
            v = x if src == 0 else xp
            hist[dst] = kf_model(v, torch.full((v.shape[0],), float(plan.t_input[eidx]), dtype=torch.float64))
            pending, seen = pending or not seen, True
            continue
        c = plan.coefs[ci].astype(np.float64)
        base = x if src == 0 else xp
        if c[7] != 0.0:
            out = (base - c[1] * hist[s0]) / c[0]
        else:
            out = c[0] * base
            for k, s in enumerate((s0, s1, s2, s3)):
                if s >= 0:
                    out = out + c[1 + k] * hist[s]
        if dst == 0:
            step += 1
            x = fix(out, step)
            inter.append(x)
        elif dst == 1:
            xp = out
        else:
            hist[dst - 2] = out
    if pending:
        x = finish_start(x)
    return x, inter
