"""Dynamic thresholding inside the native sampler loop (csrc/kernels_thresh.hip, dv_plan_set_thresholding, the routing of
DPM_Solver / UniPC), against references that do not share its code:

  1. dv_op_dynamic_threshold against oracle.sampler_ref.dynamic_thresholding (torch.quantile) on CPU float32: s to the bit
     where the interpolation weight is 0, within 1 ulp elsewhere; the output within 2 ulp;
  2. dv_sampler_run_custom_rows around the analytic stand-in network on plans with thresholding, against the reference's outputs
     (tests/golden/sampler_thresholding.npz) and the oracle's sampler;
  3. the captured graph around the real denoiser with correcting_x0_fn='dynamic_thresholding', against the oracle sampler over
     the oracle denoiser with the same hook - Plan.run_python raises, so the run cannot have been stepped;
  4. which runs go native and which stay stepped.

Every GPU test prints its figures before it asserts; with DVITS_SAMPLER_OPTIONS_REPORT=<file> they are appended to that file."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import thresholding_cases as tc
from conftest import oracle_cfg, rel_l2, unet_case
from diff_vits_amd import synth
from oracle import sampler_ref
from sampler_cases import GRAPH_BOUND, GRAPH_SHAPE, make_solver, oracle_sample

DV_ERR_INVALID = -1


def _report(line):
    print(line)
    path = os.environ.get("DVITS_SAMPLER_OPTIONS_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _ordered(a):
    """float32 -> int64 that orders like the floats and counts representable values between them (ulp distances)."""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def _ulps(a, b):
    return np.abs(_ordered(a) - _ordered(b))


# ============================================================================ 1. the operator against torch on the host
_REF = {}


def _op_ratios(n):
    return tc.OP_RATIOS + (tc.integer_rank_ratio(n),)


def _op_ref(kind, rows, n, ratio):
    """(x, s, y) of the CPU reference, computed once per case."""
    key = (kind, rows, n, ratio)
    if key not in _REF:
        x = torch.from_numpy(tc.op_data(kind, rows, n))
        mv = tc.op_max_val(kind)
        s = torch.maximum(torch.quantile(x.abs().reshape(rows, -1), ratio, dim=1), torch.full((rows,), mv))
        _REF[key] = (x, s.numpy(), sampler_ref.dynamic_thresholding(x, ratio, mv).numpy())
    return _REF[key]


def _op_cases():
    return [(kind, rows, n) for rows, n in tc.OP_SHAPES for kind in tc.OP_DATA]


def _run_op(x_host, ratio, max_val):
    from diff_vits_amd import _lib as L
    x = x_host.clone().cuda().contiguous()
    s = torch.full((x.shape[0],), -7.0, device="cuda")
    L.check(L.lib().dv_op_dynamic_threshold(L.ptr(x), x.shape[0], x.shape[1], ratio, max_val, L.ptr(s), L.stream_ptr()),
            "dv_op_dynamic_threshold")
    return x.cpu().numpy(), s.cpu().numpy()


def test_operator_cases_cover_the_paths():
    """Host only: the parametrisation reaches every row phase of the float4 path, a single-workgroup row and a split row, exact
    and interpolated ranks; and the data rows are not degenerate - the CPU reference clamps some elements and leaves some."""
    ns = [n for _, n in tc.OP_SHAPES]
    assert {n % 4 for n in ns} == {0, 1, 2, 3}
    assert any(rows >= 3 and n % 4 == 1 for rows, n in tc.OP_SHAPES)           # rows then start at every 16-byte phase
    assert min(ns) == 1 and any(1 < n <= tc.OP_SPLIT_FROM for n in ns) and any(n > 16 * tc.OP_SPLIT_FROM for n in ns)
    assert {255, 256, 257} <= set(ns)
    for n in ns:
        q = tc.integer_rank_ratio(n)
        assert tc.rank_of(q, n)[2] == 0.0 and tc.rank_of(0.0, n)[2] == 0.0 and tc.rank_of(1.0, n)[2] == 0.0
        if n > 2:
            assert 0.0 < q < 1.0
    assert any(tc.rank_of(q, n)[2] != 0.0 for n in ns for q in tc.OP_RATIOS)
    # (the non-degeneracy claim is for the median, ratio 0.5, of rows with at least three elements: at ratio 0 every element of
    # a row is clamped and at ratio 1 none, by construction, and a row of one or two elements has no interior)
    for rows, n in tc.OP_SHAPES:
        if n < 3:
            continue
        for kind in ("normal", "dups", "special"):
            x, s, y = _op_ref(kind, rows, n, 0.5)
            over = np.abs(x.numpy()) > s[:, None]
            assert over.any(axis=1).all() and (~over).any(axis=1).all(), (kind, rows, n)
        x, s, y = _op_ref("floor", rows, n, 0.9)
        assert (s == np.float32(tc.op_max_val("floor"))).all()
        x, s, y = _op_ref("dups", rows, n, 0.5)                                  # the duplicates straddle the rank
        lo, hi, _ = tc.rank_of(0.5, n)
        v = np.sort(np.abs(x.numpy()), axis=1)
        assert (v[:, lo] == v[:, hi]).all() and ((v == v[:, lo:lo + 1]).sum(axis=1) > n // 2).all()
    x, _, _ = _op_ref("special", 3, 4097, 0.5)
    a = np.abs(x.numpy())
    assert (a == 0).any() and np.signbit(x.numpy()[a == 0]).any() and ((a > 0) & (a < 1.1754944e-38)).any() and (a == np.float32(1e30)).any()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,rows,n", _op_cases())
def test_operator_vs_torch_quantile(kind, rows, n):
    for ratio in _op_ratios(n):
        x, s_ref, y_ref = _op_ref(kind, rows, n, ratio)
        mv = tc.op_max_val(kind)
        y, s = _run_op(x, ratio, mv)
        y2, s2 = _run_op(x, ratio, mv)
        w = tc.rank_of(ratio, n)[2]
        exact = w == 0.0 or kind in ("equal", "floor")
        ds, dy = int(_ulps(s, s_ref).max()), int(_ulps(y, y_ref).max())
        _report("op       %-8s %d x %-7d ratio %-22r w %.6f  s %d ulp (%s)  out %d ulp" % (kind, rows, n, ratio, w, ds,
                                                                                         "exact" if exact else "<= 1", dy))
        assert np.array_equal(s, s2) and np.array_equal(y, y2), "two calls differ"
        assert not np.isnan(s).any() and not np.isnan(y).any()
        assert ds <= (0 if exact else 1), (kind, rows, n, ratio, s, s_ref)
        assert dy <= 2, (kind, rows, n, ratio, dy)


@pytest.mark.gpu
def test_operator_nan_row_becomes_nan_and_leaves_the_others():
    rows, n = 3, 4097
    x, _, _ = _op_ref("normal", rows, n, 0.9)
    clean, s_clean = _run_op(x, 0.9, 1e-3)
    bad = x.clone()
    bad[1, 1234] = float("nan")
    y, s = _run_op(bad, 0.9, 1e-3)
    want = sampler_ref.dynamic_thresholding(bad, 0.9, 1e-3).numpy()
    assert np.isnan(want[1]).all() and not np.isnan(want[[0, 2]]).any()          # torch: the whole row
    assert np.isnan(s[1]) and np.isnan(y[1]).all()
    assert np.array_equal(y[[0, 2]], clean[[0, 2]]) and np.array_equal(s[[0, 2]], s_clean[[0, 2]])


def test_operator_refuses_bad_arguments_before_any_launch():
    """Host only: every check comes before the first HIP call."""
    from diff_vits_amd import _lib as L
    buf = np.zeros(16, dtype=np.float32)
    p = C.c_void_p(buf.ctypes.data)
    f = L.lib().dv_op_dynamic_threshold
    nan, inf = float("nan"), float("inf")
    for args in [(p, 2, 8, -0.1, 1.0), (p, 2, 8, 1.5, 1.0), (p, 2, 8, nan, 1.0), (p, 2, 8, 0.5, 0.0), (p, 2, 8, 0.5, -1.0),
                 (p, 2, 8, 0.5, inf), (p, 2, 8, 0.5, nan), (p, 0, 8, 0.5, 1.0), (p, 2, 0, 0.5, 1.0), (p, 2, 2 ** 31, 0.5, 1.0),
                 (None, 2, 8, 0.5, 1.0)]:
        assert f(*args, None, None) == DV_ERR_INVALID, args
        assert b"dv_op_dynamic_threshold" in L.lib().dv_last_error()
    assert not buf.any()


# ============================================================================ 2. the stand-in network through the native loop
def _standin_plan(key, thresholded=True):
    from diff_vits_amd.sampler._plan import Plan
    family, ctor, kw = tc.STANDIN_CASES[key]
    solver, _ = make_solver(family, lambda xx, t, **k: sampler_ref.standin_model(xx, t), None, **ctor)
    kw = dict(kw)
    args = (kw.pop("steps"), kw.pop("order"), kw.pop("skip_type"), True, None, None, kw.pop("denoise_to_zero", False))
    plain = solver._plan(*args, **({"method": kw["method"]} if "method" in kw else {}))
    if not thresholded:
        return plain
    return Plan(*plain._args[:11], thresholding=(tc.THR_RATIO, tc.THR_MAX, tc.standin_mask(key, plain.nfe)))


def _run_custom_rows(plan, x_host, entry="dv_sampler_run_custom_rows"):
    """dv_sampler_run_custom_rows on a device copy of x_host [rows, ...]; the callback stages through the host and evaluates
    the oracle's stand-in network there.  Returns (return code, x)."""
    from diff_vits_amd import _lib as L
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    x = x_host.clone().cuda().contiguous()
    n, shape = x.numel(), tuple(x_host.shape)

    def cb(user, xptr, t_in, optr, stream):
        try:
            torch.cuda.synchronize()
            host = np.empty(n, dtype=np.float32)
            if hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), C.c_void_p(xptr), n * 4, 2) != 0:
                return 1
            t = torch.full((shape[0],), t_in, dtype=torch.float32)
            out = np.ascontiguousarray(sampler_ref.standin_model(torch.from_numpy(host).reshape(shape), t).numpy(), dtype=np.float32)
            return 0 if hip.hipMemcpy(C.c_void_p(optr), out.ctypes.data_as(C.c_void_p), n * 4, 1) == 0 else 1
        except Exception as exc:        # (an exception cannot cross the C frame)
            print("stand-in callback failed:", exc)
            return 2

    cfn = L.MODEL_FN(cb)
    if entry == "dv_sampler_run_custom":
        rc = L.lib().dv_sampler_run_custom(plan.handle, cfn, None, L.ptr(x), n, None)
    else:
        rc = L.lib().dv_sampler_run_custom_rows(plan.handle, cfn, None, L.ptr(x), shape[0], n, None)
    torch.cuda.synchronize()
    return rc, x.cpu()


def test_standin_cases_need_the_thresholding(gold):
    """Host only: per case the oracle's thresholded and plain results differ by more than 100 x the case's tolerance (a loop
    that skipped the thresholding cannot pass), the goldens are the oracle's, and the masks are the two rules."""
    g = gold("sampler_thresholding.npz")
    assert {k[:-2] for k in g.files if k.endswith("_x")} == set(tc.STANDIN_CASES)
    for key in tc.STANDIN_CASES:
        tol = tc.standin_tolerance(key)
        thr, plain = tc.standin_oracle(key), tc.standin_oracle(key, thresholded=False)
        assert rel_l2(plain.numpy(), thr.numpy()) > 100 * tol, key
        assert rel_l2(thr.numpy(), g[key + "_x"]) < 1e-6, key
        plan = _standin_plan(key)
        mask = plan.thresholding[2]
        assert len(mask) == plan.nfe
        if key.endswith("_dtz"):
            assert mask == (False,) * (plan.nfe - 1) + (True,)
        else:
            assert all(mask)
    assert {tc.standin_tolerance(k) for k in tc.STANDIN_CASES} == {2e-5, 1e-4}


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(tc.STANDIN_CASES))
def test_standin_with_thresholding_through_the_native_loop(key, gold):
    want = gold("sampler_thresholding.npz")[key + "_x"]
    tol = tc.standin_tolerance(key)
    rc, got = _run_custom_rows(_standin_plan(key), tc.standin_x(key))
    assert rc == 0
    e_ref, e_orc = rel_l2(got.numpy(), want), rel_l2(got.numpy(), tc.standin_oracle(key).numpy())
    _report("thr-standin %-14s gpu vs reference %.3e  vs oracle %.3e  tol %.0e" % (key, e_ref, e_orc, tol))
    assert e_ref < tol and e_orc < tol, (key, e_ref, e_orc, tol)


@pytest.mark.gpu
def test_rows_form_without_thresholding_equals_the_plain_form():
    plan = _standin_plan("dpmpp_o2", thresholded=False)
    x = tc.standin_x("dpmpp_o2")
    rc1, a = _run_custom_rows(plan, x)
    rc2, b = _run_custom_rows(plan, x, entry="dv_sampler_run_custom")
    assert rc1 == 0 and rc2 == 0 and torch.equal(a, b)


def test_run_custom_refuses_a_thresholded_plan():
    """Host only (refused before the first HIP call): the form without a row count cannot threshold per row."""
    from diff_vits_amd import _lib as L
    plan = _standin_plan("dpmpp_o2")
    buf = np.zeros(240 + 4, dtype=np.float32)
    addr = buf.ctypes.data + (-buf.ctypes.data % 16)
    called = []
    cfn = L.MODEL_FN(lambda *a: called.append(1) or 1)
    assert L.lib().dv_sampler_run_custom(plan.handle, cfn, None, C.c_void_p(addr), 240, None) == DV_ERR_INVALID
    assert b"dv_sampler_run_custom_rows" in L.lib().dv_last_error()
    assert L.lib().dv_sampler_run_custom_rows(plan.handle, cfn, None, C.c_void_p(addr), 7, 240, None) == DV_ERR_INVALID      # 240 % 7
    assert not called


def test_plan_set_thresholding_validates():
    from diff_vits_amd import _lib as L
    plan = _standin_plan("dpmpp_o2", thresholded=False)
    f = L.lib().dv_plan_set_thresholding
    for ratio, mv in [(1.5, 1.0), (float("nan"), 1.0), (0.5, 0.0), (0.5, -2.0), (0.5, float("inf")), (0.5, float("nan"))]:
        assert f(plan.handle, ratio, mv, None) == DV_ERR_INVALID, (ratio, mv)
    assert f(plan.handle, 0.5, 1.0, None) == 0 and f(plan.handle, -1.0, 0.0, None) == 0      # on (every evaluation), off again
    with pytest.raises(ValueError):
        plan.set_thresholding((0.9, 0.6, (True,)))


# ============================================================================ 3. the captured graph around the real denoiser
@pytest.fixture(scope="module")
def cfg1():
    from diff_vits_amd.unet1d.unet_1d_condition import UNet1DConditionModel
    from oracle import unet_ref
    kw, sd, *_ = unet_case("cfg1")
    m = UNet1DConditionModel(backend="hip", **kw).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.cuda()
    m.hip_engine("bf16x3")
    B, T, L = GRAPH_SHAPE
    x, cond, enc, mask = (torch.from_numpy(a) for a in synth.make_inputs(B, 80, T, L, seed=4242, ragged_mask=True))
    oracle = unet_ref.diffusion_model_fn({k: torch.from_numpy(v) for k, v in sd.items()}, oracle_cfg(kw), cond, enc, mask)
    return m, x, cond, enc, mask, oracle


_THR_CTOR = dict(correcting_x0_fn="dynamic_thresholding", dynamic_thresholding_ratio=tc.GRAPH_THR_RATIO,
                 thresholding_max_val=tc.GRAPH_THR_MAX)


def _graph_oracle(family, ctor, skw, oracle, x, cache={}):
    key = (family, tuple(sorted(skw.items())))
    if key not in cache:
        fn = lambda v, t=None: sampler_ref.dynamic_thresholding(v, tc.GRAPH_THR_RATIO, tc.GRAPH_THR_MAX)
        with torch.no_grad():
            cache[key] = oracle_sample(family, oracle, x.clone(), None, variant=ctor.get("variant", "bh2"), x0_fn=fn, **skw)
    return cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("name", [s[0] for s in tc.GRAPH_THR_SETS])
def test_graph_path_with_dynamic_thresholding_vs_oracle(name, cfg1, monkeypatch):
    """DPM_Solver / UniPC(correcting_x0_fn='dynamic_thresholding') around NativeUNetModel: one captured graph (the stepped loop
    raises), twice bit-equal, against the oracle's sampler over the oracle's denoiser with the same hook.
    Without the feature the run is stepped and the monkeypatched Plan.run_python raises."""
    from diff_vits_amd.sampler import _plan, dpm_solver
    m, x, cond, enc, mask, oracle = cfg1
    _, family, ctor, skw = next(s for s in tc.GRAPH_THR_SETS if s[0] == name)

    def stepped(*a, **k):
        raise AssertionError("dynamic thresholding left the native graph path")
    monkeypatch.setattr(_plan.Plan, "run_python", stepped)
    native = dpm_solver.NativeUNetModel(m, cond.cuda(), enc.cuda(), mask.cuda())
    solver, _ = make_solver(family, native, None, **_THR_CTOR, **ctor)
    with torch.no_grad():
        out1 = solver.sample(x.cuda(), **skw)
        out2 = solver.sample(x.cuda(), **skw)
    ref = _graph_oracle(family, ctor, skw, oracle, x)
    err = rel_l2(out1.cpu().numpy(), ref.numpy())
    _report("thr-graph %-16s gpu %.3e  bound %.0e" % (name, err, GRAPH_BOUND))
    assert torch.equal(out1, out2)
    assert m.hip_engine().handover_status()[1] == 0
    assert err < GRAPH_BOUND, (name, err)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [s[0] for s in tc.GRAPH_THR_SETS])
def test_stepped_path_with_intermediates_agrees_with_the_graph(name, cfg1):
    """return_intermediate=True keeps the stepped loop (torch.quantile around the native UNet): its final x against the oracle
    and against the graph's, each within GRAPH_BOUND; a plain run of the same solver object uses another plan handle; switching
    the thresholding off on the plan drops its graph - the next replay is the plain run's, bit for bit."""
    from diff_vits_amd.sampler import dpm_solver
    m, x, cond, enc, mask, oracle = cfg1
    _, family, ctor, skw = next(s for s in tc.GRAPH_THR_SETS if s[0] == name)
    native = dpm_solver.NativeUNetModel(m, cond.cuda(), enc.cuda(), mask.cuda())
    solver, _ = make_solver(family, native, None, **_THR_CTOR, **ctor)
    plain_solver, _ = make_solver(family, native, None, **ctor)
    with torch.no_grad():
        graph = solver.sample(x.cuda(), **skw)
        stepped, inter = solver.sample(x.cuda(), return_intermediate=True, **skw)
        plain = plain_solver.sample(x.cuda(), **skw)
    ref = _graph_oracle(family, ctor, skw, oracle, x)
    e_step, e_both = rel_l2(stepped.cpu().numpy(), ref.numpy()), rel_l2(stepped.cpu().numpy(), graph.cpu().numpy())
    e_plain = rel_l2(plain.cpu().numpy(), graph.cpu().numpy())
    _report("thr-graph %-16s stepped vs oracle %.3e  stepped vs graph %.3e  plain vs graph %.3e  bound %.0e"
            % (name, e_step, e_both, e_plain, GRAPH_BOUND))
    assert len(inter) == skw["steps"] + 1
    assert e_step < GRAPH_BOUND and e_both < GRAPH_BOUND
    assert e_plain > 100 * GRAPH_BOUND                         # the thresholding is in the graph
    thr_plans = [p for k, p in solver._plans.items() if p.thresholding is not None]
    plain_plans = [p for k, p in solver._plans.items() if p.thresholding is None]
    assert len(thr_plans) == 1 and len(plain_plans) == 1       # (the stepped run uses the plain plan: its hook is Python's)
    assert thr_plans[0].handle.value != plain_plans[0].handle.value
    # off: the plan object the graph run used (its per-shape copy holds the captured graph) replays as a plain plan
    for p in list(thr_plans[0]._per_shape.values()):
        p.set_thresholding(None)
    with torch.no_grad():
        off = native.run_plan(thr_plans[0], x.cuda())
    assert torch.equal(off, plain)


# ============================================================================ 4. routing on the host
class _Recorder:
    """A NativeUNetModel stand-in for the routing rules: records run_plan calls; as a callable it is the analytic network."""

    def __new__(cls):
        from diff_vits_amd.sampler._plan import NativeUNetModel

        class R(NativeUNetModel):
            def __init__(self):
                self.calls = []

            def __call__(self, x, t_input, **kw):
                return sampler_ref.standin_model(x, t_input)

            def run_plan(self, plan, x):
                self.calls.append(plan)
                return x
        return R()


@pytest.mark.parametrize("family", ["dpm", "unipc"])
def test_cpu_and_hooked_runs_stay_stepped_and_equal_the_plain_hook(family):
    """Host only: on a CPU tensor - with or without the other hooks - run_plan is never called, and the string option gives what
    the same thresholding passed as a callable gives (today's stepped path)."""
    x = tc.standin_x("dpmpp_o2" if family == "dpm" else "unipc_bh2")
    skw = dict(steps=8, order=2, skip_type="time_uniform", denoise_to_zero=True)
    fn = ((lambda v, t: sampler_ref.dynamic_thresholding(v, tc.THR_RATIO, tc.THR_MAX)) if family == "dpm" else
          (lambda v: sampler_ref.dynamic_thresholding(v, tc.THR_RATIO, tc.THR_MAX)))
    thr = dict(correcting_x0_fn="dynamic_thresholding", dynamic_thresholding_ratio=tc.THR_RATIO, thresholding_max_val=tc.THR_MAX)
    for extra, call in [({}, {}), (dict(correcting_xt_fn=sampler_ref.standin_xt_fix), {}), ({}, dict(return_intermediate=True))]:
        rec = _Recorder()
        a = make_solver(family, rec, None, **thr, **extra)[0].sample(x.clone(), **skw, **call)
        b = make_solver(family, rec, None, correcting_x0_fn=fn, **extra)[0].sample(x.clone(), **skw, **call)
        a, b = (a[0], b[0]) if call else (a, b)
        assert not rec.calls
        assert torch.equal(a, b)
        want = oracle_sample(family, sampler_ref.standin_model, x.clone(), None,
                             x0_fn=lambda v, t=None: sampler_ref.dynamic_thresholding(v, tc.THR_RATIO, tc.THR_MAX),
                             xt_fn=extra.get("correcting_xt_fn"), **skw)
        assert rel_l2(a.numpy(), want.numpy()) < 2e-5


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["dpm", "unipc"])
def test_routing_of_cuda_runs(family):
    """On a CUDA tensor: the string option alone goes to run_plan with a thresholded plan (mask by the algorithm's rule), a plain
    run of the same solver with another plan; an xt hook, a callable x0 hook or return_intermediate never reach run_plan."""
    import types
    x = tc.standin_x("dpmpp_o2" if family == "dpm" else "unipc_bh2").cuda()
    skw = dict(steps=8, order=2, skip_type="time_uniform", denoise_to_zero=True)
    thr = dict(correcting_x0_fn="dynamic_thresholding", dynamic_thresholding_ratio=tc.THR_RATIO, thresholding_max_val=tc.THR_MAX)
    noise_algo = dict(algorithm_type="dpmsolver" if family == "dpm" else "noise_prediction")
    for algo, want_mask in [({}, (True,) * 9), (noise_algo, (False,) * 8 + (True,))]:
        rec = _Recorder()
        rec.unet = types.SimpleNamespace(backend="hip")
        solver = make_solver(family, rec, None, **thr, **algo)[0]
        solver.sample(x, **skw)
        assert len(rec.calls) == 1 and rec.calls[0].thresholding == (tc.THR_RATIO, tc.THR_MAX, want_mask)
        solver.sample(x, **dict(skw, denoise_to_zero=False))
        assert len(rec.calls) == 2
        if algo:      # the noise forms threshold the denoise_to_zero evaluation only: without it the plain plan runs
            assert rec.calls[1].thresholding is None
        else:
            assert rec.calls[1].thresholding == (tc.THR_RATIO, tc.THR_MAX, (True,) * 8)
        solver.sample(x, return_intermediate=True, **skw)
        assert len(rec.calls) == 2
        assert len({p.handle.value for p in solver._plans.values()}) == len(solver._plans)
    fn = ((lambda v, t: sampler_ref.dynamic_thresholding(v, tc.THR_RATIO, tc.THR_MAX)) if family == "dpm" else
          (lambda v: sampler_ref.dynamic_thresholding(v, tc.THR_RATIO, tc.THR_MAX)))
    for ctor in (dict(thr, correcting_xt_fn=sampler_ref.standin_xt_fix), dict(correcting_x0_fn=fn)):
        rec = _Recorder()
        rec.unet = types.SimpleNamespace(backend="hip")
        make_solver(family, rec, None, **ctor)[0].sample(x, **skw)
        assert not rec.calls
    rec = _Recorder()
    rec.unet = types.SimpleNamespace(backend="hip")
    plain = make_solver(family, rec, None)[0]
    plain.sample(x, **skw)
    assert len(rec.calls) == 1 and rec.calls[0].thresholding is None
