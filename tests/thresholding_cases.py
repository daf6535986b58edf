"""Cases of the dynamic-thresholding tests (test_gpu_thresholding.py), shared with the generator of
tests/golden/sampler_thresholding.npz (tools/make_golden_sampler_thr.py) and the host-side choice of the graph cases' constants
(tools/thresholding_sensitivity.py)."""
import numpy as np

# the project's hook constants (sampler_cases.OPTION_CASES "thr": ratio 0.9, max 0.6)
THR_RATIO, THR_MAX = 0.9, 0.6

# ---- stand-in network through the native loop: (solver family, constructor keywords, sample() keywords).  Thresholding is the
#      only correction (no correcting_xt_fn): every evaluation in the data forms, the final denoise_to_zero one in the noise forms.
STANDIN_CASES = {
    "dpmpp_o2": ("dpm", {}, dict(steps=10, order=2, skip_type="time_uniform")),
    "dpmpp_ss_o3": ("dpm", {}, dict(steps=12, order=3, skip_type="time_uniform", method="singlestep")),
    "dpmn_dtz": ("dpm", dict(algorithm_type="dpmsolver"), dict(steps=9, order=2, skip_type="time_uniform", denoise_to_zero=True)),
    "unipc_bh2": ("unipc", dict(variant="bh2"), dict(steps=10, order=2, skip_type="time_uniform")),
    "unipcn_dtz": ("unipc", dict(variant="bh2", algorithm_type="noise_prediction"),
                   dict(steps=10, order=2, skip_type="time_uniform", denoise_to_zero=True)),
}


def standin_x(key):
    """Start point of a stand-in case (the reference's UniPC wrapper only broadcasts at B = 1)."""
    import torch
    from diff_vits_amd import synth
    return torch.from_numpy(synth.normal(1234, "thr." + key, (2 if STANDIN_CASES[key][0] == "dpm" else 1, 5, 24)))


def standin_mask(key, nfe):
    """The evaluations whose data prediction the reference thresholds (dpm_solver.py:433-445, 541-545; uni_pc.py:279-293)."""
    family, ctor, kw = STANDIN_CASES[key]
    data_form = ctor.get("algorithm_type", "dpmsolver++" if family == "dpm" else "data_prediction") in ("dpmsolver++", "data_prediction")
    return tuple(data_form or (bool(kw.get("denoise_to_zero")) and e == nfe - 1) for e in range(nfe))


def standin_tolerance(key):
    from sampler_cases import option_tolerance
    family, ctor, kw = STANDIN_CASES[key]
    algo = ctor.get("algorithm_type", "dpmsolver++") if family == "dpm" else "dpmsolver++"
    ualgo = ctor.get("algorithm_type", "data_prediction") if family == "unipc" else "data_prediction"
    return option_tolerance(None, kw.get("method", "multistep"), algo, ualgo)


def standin_oracle(key, thresholded=True, ratio=THR_RATIO, max_val=THR_MAX):
    """The oracle's sampler over the stand-in network, with sampler_ref.dynamic_thresholding as its correcting_x0_fn."""
    from oracle import sampler_ref
    from sampler_cases import oracle_sample
    family, ctor, kw = STANDIN_CASES[key]
    x0_fn = (lambda v, t=None: sampler_ref.dynamic_thresholding(v, ratio, max_val)) if thresholded else None
    return oracle_sample(family, sampler_ref.standin_model, standin_x(key), None, algorithm_type=ctor.get("algorithm_type"),
                         variant=ctor.get("variant", "bh2"), x0_fn=x0_fn, **kw)


# ---- the captured graph around the real denoiser (sampler_cases.GRAPH_SHAPE, cfg1, ragged prompt mask): 8 steps, order 2,
#      t_end = 0.05.  ratio / max_val are chosen on the CPU oracle (tools/thresholding_sensitivity.py; figures in
#      profiles/sampler_options_gpu.txt) so that (a) the quantile exceeds max_val in at least half of the evaluations,
#      (b) thresholded and plain oracle outputs differ by more than 100 x GRAPH_BOUND and (c) the oracle against itself with
#      the denoiser output perturbed by GRAPH_PERTURBATION stays inside a third of GRAPH_BOUND.
GRAPH_THR_RATIO, GRAPH_THR_MAX = 0.9, 0.5
GRAPH_THR_SETS = [
    ("thr_dpmpp", "dpm", {}, dict(steps=8, order=2, skip_type="time_uniform", t_end=0.05)),
    ("thr_unipc_bh2", "unipc", dict(variant="bh2"), dict(steps=8, order=2, skip_type="time_uniform", t_end=0.05)),
]


# ---- the operator: rows x n, ratios, data
OP_SHAPES = [(1, 1), (3, 2), (2, 3), (2, 255), (2, 256), (2, 257), (3, 4097), (2, 6000), (2, 204800)]
OP_RATIOS = (0.0, 1.0, 0.5, 0.9, 0.995)
OP_SPLIT_FROM = 2048          # elements of a row per workgroup (THR_ELEMS_PER_WG in csrc/kernels_thresh.hip): longer rows are split
OP_DATA = ("normal", "equal", "dups", "special", "floor")
DENORM_MIN = float(np.float32(1e-45))


def rank_of(ratio, n):
    """(floor, ceil, weight) of torch.quantile's rank for a float32 input: q is a float32 tensor, the product one float32 product."""
    r = np.float32(ratio) * np.float32(n - 1)
    lo = int(np.floor(r))
    return lo, int(np.ceil(r)), float(np.float32(r - np.float32(lo)))


def integer_rank_ratio(n):
    """A ratio (interior where the row has one) whose rank ratio * (n - 1) is an exact integer in float32."""
    mid = (n - 1) // 2
    for k in sorted(range(n), key=lambda k: (k in (0, n - 1), abs(k - mid))):
        q = k / (n - 1) if n > 1 else 0.0
        lo, hi, w = rank_of(q, n)
        if w == 0.0 and lo == k:
            return q
    raise AssertionError(n)


def op_max_val(kind):
    # "floor": above every element (s = max_val); "special": the smallest positive float32, so that denormal order statistics count
    return {"floor": 10.0, "special": DENORM_MIN}.get(kind, 1e-3)


def op_data(kind, rows, n):
    """x [rows, n] float32 of a data kind (every row its own values)."""
    from diff_vits_amd import synth
    x = synth.normal(77, "thr.%s.%d.%d" % (kind, rows, n), (rows, n)).astype(np.float32)
    if kind in ("normal", "floor"):
        return x
    if kind == "equal":
        return np.repeat(np.float32([-1.25, 0.5, 3.0])[:rows, None], n, axis=1) if rows <= 3 else None
    perm = np.argsort(synth.normal(78, "thr.perm.%d.%d" % (rows, n), (rows, n)), axis=1)
    out = np.empty_like(x)
    for r in range(rows):
        if kind == "dups":            # more than n / 2 copies of one magnitude (either sign) around the median rank
            v = np.sort(np.abs(x[r]))
            lo = n // 5
            m = n // 2 + 1 if n > 2 else n
            v[lo:lo + m] = np.float32(0.5 + r)
            v[:lo] *= np.float32(0.4) / max(v[:lo].max(), np.float32(1)) if lo else 1
            v[lo + m:] = np.float32(0.5 + r) + np.float32(0.25) + v[lo + m:]
            v *= np.where(x[r] < 0, np.float32(-1), np.float32(1))
        else:                         # "special": +-0, denormals, the smallest normal, one large value
            k = np.arange(n)
            v = np.where(k % 3 == 0, np.float32(0.0), (k % 977 + 1).astype(np.float32) * np.float32(DENORM_MIN)).astype(np.float32)
            v[k % 7 == 3] = np.float32(1.1754944e-38)
            v = np.where(x[r] < 0, -v, v).astype(np.float32)
            v[n // 2] = np.float32(-1e30)
        out[r] = v[perm[r]]
    return out
