"""Classifier-free guidance inside the native sampler loop (csrc/kernels_guide.hip, dv_plan_set_guidance, the routing of
model_wrapper / DPM_Solver / UniPC, NaturalSpeech2.sample_from_prior(guidance_scale=)), against references that do not share
its code:

  1. dv_op_cfg_combine against a host emulation of the stated arithmetic (float32 difference, float64 product-and-add rounded
     to float32): at most 1 ulp apart, twice bit-equal, a NaN stays in its row;
  2. the captured graph around the real denoiser under guidance, against the oracle sampler over the oracle denoiser -
     Plan.run_python raises, so the run cannot have been stepped;
  3. the stepped guided route over the two-condition stand-in against the reference's own outputs
     (tests/golden/sampler_options.npz: dpm_cfg, dpm_cfg_scale1) - with a NativeUNetModel behind the wrapper, whose record must
     not make the stepped loop call the raw model;
  4. which runs go native and which stay stepped;
  5. NaturalSpeech2.sample_from_prior on the HIP backend against the torch backend of this package.

Every GPU test prints its figures before it asserts; with DVITS_SAMPLER_OPTIONS_REPORT=<file> they are appended to that file."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import guidance_cases as gc
import thresholding_cases as tc
from conftest import oracle_cfg, rel_l2, unet_case
from diff_vits_amd import synth
from oracle import sampler_ref
from sampler_cases import GRAPH_BOUND, GRAPH_SHAPE, OPTION_CASES, option_tolerance

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


# ============================================================================ 1. the operator against the host emulation
def _run_op(pair_host, rows, g):
    from diff_vits_amd import _lib as L
    pair = torch.from_numpy(pair_host).cuda().contiguous()
    out = torch.full((rows, pair.shape[1]), -7.0, device="cuda")
    L.check(L.lib().dv_op_cfg_combine(L.ptr(pair), L.ptr(out), rows, pair.shape[1], g, L.stream_ptr()), "dv_op_cfg_combine")
    return out.cpu().numpy()


def test_operator_cases_cover_the_phases():
    """Host only: the row lengths cover all four n % 4 phases, a single element, lengths around one workgroup's float4 stride
    and more than one workgroup; with three rows of n % 4 == 1 the rows start at every 16-byte phase; the emulation is not
    degenerate (the scales change the result, and the float32 difference is not exact everywhere)."""
    assert {n % 4 for n in gc.OP_NUMELS} == {0, 1, 2, 3}
    assert 1 in gc.OP_NUMELS and {255, 256, 257} <= set(gc.OP_NUMELS) and max(gc.OP_NUMELS) > 4 * 256
    assert 3 in gc.OP_ROWS and 1 in gc.OP_ROWS
    for n in (n for n in gc.OP_NUMELS if n % 4 == 1):
        assert {(r * n) % 4 for r in range(2 * 3)} == {0, 1, 2, 3}, n           # u and c rows of a 3-row pair
    assert set(gc.OP_SCALES) == {0.0, 0.5, 2.5, 7.0, -1.0}
    pair = gc.op_data(3, 4097)
    refs = [gc.op_ref(pair, 3, g) for g in gc.OP_SCALES]
    assert np.array_equal(refs[0], pair[:3])                                       # g = 0: the unconditional rows
    assert all(not np.array_equal(refs[0], r) for r in refs[1:])
    d32 = (pair[3:] - pair[:3]).astype(np.float32).astype(np.float64)
    assert (d32 != pair[3:].astype(np.float64) - pair[:3].astype(np.float64)).any()


@pytest.mark.gpu
@pytest.mark.parametrize("rows", gc.OP_ROWS)
@pytest.mark.parametrize("n", gc.OP_NUMELS)
def test_operator_vs_host_emulation(rows, n):
    pair = gc.op_data(rows, n)
    for g in gc.OP_SCALES:
        want = gc.op_ref(pair, rows, g)
        got, got2 = _run_op(pair, rows, g), _run_op(pair, rows, g)
        d = int(_ulps(got, want).max())
        _report("cfg-op   %d x %-5d g %-5r  %d ulp" % (rows, n, g, d))
        assert np.array_equal(got, got2), "two calls differ"
        assert not np.isnan(got).any()
        assert d <= 1, (rows, n, g, d)


@pytest.mark.gpu
def test_operator_nan_stays_in_its_row():
    rows, n = 3, 4097
    pair = gc.op_data(rows, n)
    clean = _run_op(pair, rows, 2.5)
    bad = pair.copy()
    bad[1, :] = np.nan                     # the unconditional prediction of row 1 ...
    bad[rows + 2, 17] = np.nan             # ... and one element of the conditional prediction of row 2
    got = _run_op(bad, rows, 2.5)
    assert np.isnan(got[1]).all()
    assert np.isnan(got[2, 17]) and np.isnan(got[2]).sum() == 1
    assert np.array_equal(got[0], clean[0])
    keep = np.arange(n) != 17
    assert np.array_equal(got[2, keep], clean[2, keep])


def _offset_view(n, off, fill=None):
    """n floats on the GPU that start `off` floats behind a 16-byte boundary (a view into a larger allocation; the floats
    around it hold a canary)."""
    buf = torch.full((n + 8,), 123.0, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + n]
    if fill is not None:
        v.copy_(torch.from_numpy(fill).reshape(-1))
    return buf, v


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 5, 255, 257, 4097])
def test_operator_at_every_destination_and_source_phase(n):
    """The destination's head (out 1, 2, 3 floats behind a 16-byte boundary) and sources at other phases than the destination:
    the same bits as the aligned call, nothing written outside out."""
    from diff_vits_amd import _lib as L
    rows, g = 3, 2.5
    pair = gc.op_data(rows, n)
    want = _run_op(pair, rows, g)
    for out_off in range(4):
        for in_off in range(4):
            _, src = _offset_view(2 * rows * n, in_off, pair)
            obuf, out = _offset_view(rows * n, out_off)
            L.check(L.lib().dv_op_cfg_combine(C.c_void_p(src.data_ptr()), C.c_void_p(out.data_ptr()), rows, n, g, L.stream_ptr()),
                    "dv_op_cfg_combine")
            assert np.array_equal(out.cpu().numpy().reshape(rows, n), want), (n, out_off, in_off)
            rest = torch.cat([obuf[:out_off], obuf[out_off + rows * n:]])
            assert bool((rest == 123.0).all()), (n, out_off, in_off)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 5, 255, 256, 257, 4097, 6001])
def test_pair_in_operator_at_every_phase(n):
    """k_cfg_pair_in through dv_op_cfg_pair_in: both halves of out equal the input for every length phase (the second half
    then starts at every 4-byte phase), every destination and source offset; nothing written outside out."""
    from diff_vits_amd import _lib as L
    x = synth.normal(92, "cfg.in.%d" % n, (n,)).astype(np.float32)
    for out_off in range(4):
        for in_off in range(4):
            _, src = _offset_view(n, in_off, x)
            obuf, out = _offset_view(2 * n, out_off)
            L.check(L.lib().dv_op_cfg_pair_in(C.c_void_p(src.data_ptr()), C.c_void_p(out.data_ptr()), n, L.stream_ptr()),
                    "dv_op_cfg_pair_in")
            got = out.cpu().numpy()
            assert np.array_equal(got[:n], x) and np.array_equal(got[n:], x), (n, out_off, in_off)
            rest = torch.cat([obuf[:out_off], obuf[out_off + 2 * n:]])
            assert bool((rest == 123.0).all()), (n, out_off, in_off)


def test_pair_in_operator_refuses_bad_arguments_before_any_launch():
    """Host only."""
    from diff_vits_amd import _lib as L
    src, dst = np.zeros(16, dtype=np.float32), np.zeros(32, dtype=np.float32)
    p, o = C.c_void_p(src.ctypes.data), C.c_void_p(dst.ctypes.data)
    f = L.lib().dv_op_cfg_pair_in
    for args in [(None, o, 8), (p, None, 8), (p, o, 0), (p, o, -4), (p, o, 2 ** 41), (C.c_void_p(src.ctypes.data + 1), o, 8),
                 (p, C.c_void_p(dst.ctypes.data + 2), 8)]:
        assert f(*args, None) == DV_ERR_INVALID, args
        assert b"dv_op_cfg_pair_in" in L.lib().dv_last_error()
    assert not dst.any()


def test_operator_refuses_bad_arguments_before_any_launch():
    """Host only: every check comes before the first HIP call."""
    from diff_vits_amd import _lib as L
    src, dst = np.zeros(32, dtype=np.float32), np.zeros(16, dtype=np.float32)
    p, o = C.c_void_p(src.ctypes.data), C.c_void_p(dst.ctypes.data)
    f = L.lib().dv_op_cfg_combine
    for args in [(None, o, 2, 8, 1.0), (p, None, 2, 8, 1.0), (p, o, 0, 8, 1.0), (p, o, -1, 8, 1.0), (p, o, 2, 0, 1.0),
                 (p, o, 2, 2 ** 31, 1.0), (p, o, 2, 8, float("nan")), (p, o, 2, 8, float("inf")),
                 (C.c_void_p(src.ctypes.data + 2), o, 2, 8, 1.0)]:
        assert f(*args, None) == DV_ERR_INVALID, args
        assert b"dv_op_cfg_combine" in L.lib().dv_last_error()
    assert not dst.any()


def _standin_plan(guidance=None):
    from diff_vits_amd.sampler._plan import Plan
    return Plan(0, synth.make_betas(), 10, 2, "time_uniform", True, guidance=guidance)


def test_plan_set_guidance_validates_and_copies_carry_it():
    """Host only."""
    from diff_vits_amd import _lib as L
    plan = _standin_plan()
    f = L.lib().dv_plan_set_guidance
    for scale in (float("nan"), float("inf"), -float("inf")):
        assert f(plan.handle, scale, 1) == DV_ERR_INVALID, scale
        assert b"dv_plan_set_guidance" in L.lib().dv_last_error()
    assert f(None, 2.0, 1) == DV_ERR_INVALID
    assert f(plan.handle, 2.0, 1) == 0 and f(plan.handle, -1.0, 1) == 0 and f(plan.handle, 0.0, 1) == 0
    assert f(plan.handle, float("nan"), 0) == 0                      # off: the scale is ignored
    assert plan.guidance is None
    guided = plan.with_guidance(2.5)
    assert guided is plan.with_guidance(2.5) and guided is not plan and guided.handle.value != plan.handle.value
    assert guided.guidance == 2.5 and plan.guidance is None and plan.with_guidance(3.0) is not guided
    assert np.array_equal(guided.coefs, plan.coefs) and np.array_equal(guided.events, plan.events)
    first, second = guided.for_shape("a"), guided.for_shape("b")
    assert first is guided and second is not guided and second.guidance == 2.5
    assert plan.for_shape("a") is plan and plan.for_shape("b").guidance is None
    thr = _standin_plan()
    thr.set_thresholding((0.9, 0.6, None))
    both = thr.with_guidance(2.0)
    assert both.thresholding == (0.9, 0.6, None) and both.guidance == 2.0
    both.set_thresholding(None)                                      # (changing one option keeps the other)
    assert both.guidance == 2.0 and both.for_shape("a").for_shape("b").guidance == 2.0
    thr.set_thresholding((0.8, 0.7, None))                           # the parent changes: its siblings are made anew
    fresh = thr.with_guidance(2.0)
    assert fresh is not both and fresh.thresholding == (0.8, 0.7, None) and fresh.guidance == 2.0
    assert plan.graph_nodes() == 0 and guided.graph_nodes() == 0    # nothing captured on the host


def test_run_custom_refuses_a_guided_plan():
    """Host only (refused before the first HIP call): the callback form has no pair of conditions."""
    from diff_vits_amd import _lib as L
    plan = _standin_plan(guidance=2.5)
    buf = np.zeros(240 + 4, dtype=np.float32)
    addr = buf.ctypes.data + (-buf.ctypes.data % 16)
    called = []
    cfn = L.MODEL_FN(lambda *a: called.append(1) or 1)
    assert L.lib().dv_sampler_run_custom(plan.handle, cfn, None, C.c_void_p(addr), 240, None) == DV_ERR_INVALID
    assert b"guidance" in L.lib().dv_last_error()
    assert L.lib().dv_sampler_run_custom_rows(plan.handle, cfn, None, C.c_void_p(addr), 2, 240, None) == DV_ERR_INVALID
    assert b"guidance" in L.lib().dv_last_error()
    assert not called and not buf.any()


# ============================================================================ 2. the captured graph around the real denoiser
@pytest.fixture(scope="module")
def cfg1():
    from diff_vits_amd.unet1d.unet_1d_condition import UNet1DConditionModel
    kw, sd, *_ = unet_case("cfg1")
    m = UNet1DConditionModel(backend="hip", **kw).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.cuda()
    m.hip_engine("bf16x3")
    return m, {k: torch.from_numpy(v) for k, v in sd.items()}, oracle_cfg(kw)


_THR_CTOR = dict(correcting_x0_fn="dynamic_thresholding", dynamic_thresholding_ratio=tc.GRAPH_THR_RATIO,
                 thresholding_max_val=tc.GRAPH_THR_MAX)


def _graph_oracle(name, sd, ocfg, cache={}):
    """The oracle's guided result of a set, computed once."""
    if name not in cache:
        _, family, ctor, skw, B, g, uncond, thr = gc.graph_set(name)
        x, cond, enc, mask, uenc, umask = gc.graph_inputs(B, uncond)
        x0_fn = (lambda v, t=None: sampler_ref.dynamic_thresholding(v, tc.GRAPH_THR_RATIO, tc.GRAPH_THR_MAX)) if thr else None
        with torch.no_grad():
            cache[name] = gc.oracle_guided_sample(family, ctor, skw, gc.oracle_pair_model(sd, ocfg, cond, mask, umask), x, enc, uenc, g,
                                                  x0_fn)
    return cache[name]


def _native(m, B, uncond):
    from diff_vits_amd.sampler import dpm_solver
    x, cond, enc, mask, uenc, umask = gc.graph_inputs(B, uncond)
    native = dpm_solver.NativeUNetModel(m, cond.cuda(), enc.cuda(), mask.cuda(), uncond_mask=None if uncond == "zeros" else umask.cuda())
    return native, x, enc, uenc


def test_graph_sets_cover_the_shapes():
    """Host only: the shapes and options the graph test has to reach."""
    sets = gc.GRAPH_CFG_SETS
    assert GRAPH_SHAPE == (2, gc.GRAPH_T, gc.GRAPH_L) and {s[4] for s in sets} == {1, 2, 3}
    assert all(gc.GRAPH_T % 32 != 0 and (gc.GRAPH_T // d) % 32 != 0 for d in (1, 2, 4, 8))
    assert any(s[1] == "unipc" and s[2].get("variant") == "bh2" and s[3]["order"] == 2 for s in sets)
    assert any(s[1] == "dpm" and not s[2] and s[3]["order"] == 2 for s in sets)
    assert any(s[2].get("algorithm_type") == "dpmsolver" for s in sets) and any(s[7] for s in sets)
    assert any(s[6] == "random" for s in sets) and all(s[5] != 1.0 for s in sets)
    x, cond, enc, mask, uenc, umask = gc.graph_inputs(2, "random")
    assert not torch.equal(mask, umask) and not torch.equal(enc, uenc)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [s[0] for s in gc.GRAPH_CFG_SETS])
def test_graph_path_with_guidance_vs_oracle(name, cfg1, monkeypatch):
    """model_wrapper(guidance_type='classifier-free') around NativeUNetModel: one captured graph (the stepped loop raises),
    twice bit-equal, against the oracle's sampler over the oracle's denoiser (DPM family: the oracle's own guided noise
    formula; UniPC: the pair combined in float64).  Without the feature the run is stepped and the monkeypatched
    Plan.run_python raises."""
    from diff_vits_amd.sampler import _plan
    m, sd, ocfg = cfg1
    _, family, ctor, skw, B, g, uncond, thr = gc.graph_set(name)

    def stepped(*a, **k):
        raise AssertionError("classifier-free guidance left the native graph path")
    monkeypatch.setattr(_plan.Plan, "run_python", stepped)
    native, x, enc, uenc = _native(m, B, uncond)
    solver, _, _ = gc.make_guided_solver(family, native, enc.cuda(), uenc.cuda(), g, **(_THR_CTOR if thr else {}), **ctor)
    with torch.no_grad():
        out1 = solver.sample(x.cuda(), **skw)
        out2 = solver.sample(x.cuda(), **skw)
    ref = _graph_oracle(name, sd, ocfg)
    err = rel_l2(out1.cpu().numpy(), ref.numpy())
    _report("cfg-graph %-14s B %d g %.2f  gpu %.3e  bound %.0e" % (name, B, g, err, GRAPH_BOUND))
    assert torch.equal(out1, out2)
    assert m.hip_engine().handover_status()[1] == 0
    assert m.hip_engine()._cur.prepared[0] == 2 * B                 # the engine ran the pair
    assert err < GRAPH_BOUND, (name, err)


# ============================================================================ 3. the stepped guided route against the reference's goldens
class _StandinNative:
    """A NativeUNetModel whose network is the oracle's two-condition stand-in: model_wrapper records it for the native route,
    and a stepped run must still go through the guided noise prediction."""

    def __new__(cls):
        from diff_vits_amd.sampler._plan import NativeUNetModel

        class R(NativeUNetModel):
            def __init__(self):
                self.calls = []
                self.unet = types.SimpleNamespace(backend="hip")

            def __call__(self, x, t_input, cond=None, **kw):
                return sampler_ref.standin_cond_model(x, t_input, cond)

            def run_plan(self, plan, x, guidance=None):
                self.calls.append((plan, guidance))
                return x
        return R()


def _golden_case(key):
    family, kw = OPTION_CASES[key]
    kw = dict(kw)
    scale = {"cfg": 2.5, "cfg1": 1.0}[kw.pop("guidance")]
    B = 2
    x = torch.from_numpy(synth.normal(1234, "opts." + key, (B, 5, 24)))
    cond = torch.from_numpy(synth.normal(4321, "cond." + key, (B, 5, 1)))
    return family, kw, scale, x, cond


@pytest.mark.parametrize("key", ["dpm_cfg", "dpm_cfg_scale1"])
def test_stepped_guided_route_reproduces_the_reference(key, gold):
    """Host only.  CPU tensors: the wrapper's record must not short-circuit the stepped loop to the raw model (that would drop
    the guidance and the condition) - the result is the reference's; a guided plan stepped by hand gives the same."""
    from diff_vits_amd.sampler._plan import sample_with_plan
    want = gold("sampler_options.npz")[key + "_x"]
    family, kw, scale, x, cond = _golden_case(key)
    tol = option_tolerance(None)
    rec = _StandinNative()
    solver, fn, ns = gc.make_guided_solver(family, rec, cond, torch.zeros_like(cond), scale)
    assert getattr(fn, "_dv", None) is None and fn._dv_cfg["guidance_scale"] == scale
    out = solver.sample(x.clone(), **kw)
    plain = gc.make_guided_solver(family, lambda xx, t, *c, **k: sampler_ref.standin_cond_model(xx, t, *c), cond,
                                  torch.zeros_like(cond), scale)[0].sample(x.clone(), **kw)
    unguided = gc.make_guided_solver(family, rec, torch.zeros_like(cond), torch.zeros_like(cond), 1.0)[0].sample(x.clone(), **kw)
    assert not rec.calls
    assert torch.equal(out, plain)                                               # today's generic result, bit for bit
    assert rel_l2(out.numpy(), want) < tol
    assert rel_l2(unguided.numpy(), want) > 100 * tol                            # (the condition matters: dropping it cannot pass)
    plan = solver._plan(kw["steps"], kw["order"], kw["skip_type"], True).with_guidance(2.5)
    by_hand = sample_with_plan(plan, fn, ns, x.clone())
    assert torch.equal(by_hand, out)


# ============================================================================ 4. routing
@pytest.mark.parametrize("family", ["dpm", "unipc"])
def test_cpu_intermediate_and_hooked_runs_stay_stepped(family):
    """Host only: CPU tensors, return_intermediate=True and a callable hook never reach run_plan and equal the generic result
    of the same wrapper around a plain callable."""
    B = 2 if family == "dpm" else 1
    x = torch.from_numpy(synth.normal(1234, "cfg.route." + family, (B, 5, 24)))
    cond = torch.from_numpy(synth.normal(4321, "cfg.route.cond." + family, (B, 5, 1)))
    skw = dict(steps=8, order=2, skip_type="time_uniform")
    plain_net = lambda xx, t, *c, **k: sampler_ref.standin_cond_model(xx, t, *c)
    for extra, call in [({}, {}), ({}, dict(return_intermediate=True)), (dict(correcting_xt_fn=sampler_ref.standin_xt_fix), {}),
                        (dict(correcting_x0_fn=(lambda v, t: 0.98 * v) if family == "dpm" else (lambda v: 0.98 * v)), {})]:
        rec = _StandinNative()
        a = gc.make_guided_solver(family, rec, cond, torch.zeros_like(cond), 2.5, **extra)[0].sample(x.clone(), **skw, **call)
        b = gc.make_guided_solver(family, plain_net, cond, torch.zeros_like(cond), 2.5, **extra)[0].sample(x.clone(), **skw, **call)
        a, b = (a[0], b[0]) if call else (a, b)
        assert not rec.calls
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["dpm", "unipc"])
def test_routing_of_cuda_runs(family):
    """On a CUDA tensor a classifier-free wrapper around a NativeUNetModel goes to run_plan with its record - with the
    thresholded plan where the solver has the string option; intermediates, hooks, model kwargs, another model type and
    classifier guidance never do."""
    B = 2 if family == "dpm" else 1
    x = torch.from_numpy(synth.normal(1234, "cfg.route." + family, (B, 5, 24))).cuda()
    cond = torch.from_numpy(synth.normal(4321, "cfg.route.cond." + family, (B, 5, 1))).cuda()
    zero = torch.zeros_like(cond)
    skw = dict(steps=8, order=2, skip_type="time_uniform")
    rec = _StandinNative()
    solver = gc.make_guided_solver(family, rec, cond, zero, 2.5)[0]
    solver.sample(x, **skw)
    assert len(rec.calls) == 1 and rec.calls[0][1]["guidance_scale"] == 2.5 and rec.calls[0][0].thresholding is None
    assert rec.calls[0][1]["condition"] is cond and rec.calls[0][1]["unconditional_condition"] is zero
    solver.sample(x, return_intermediate=True, **skw)
    assert len(rec.calls) == 1
    thr = dict(correcting_x0_fn="dynamic_thresholding", dynamic_thresholding_ratio=tc.THR_RATIO, thresholding_max_val=tc.THR_MAX)
    rec = _StandinNative()
    gc.make_guided_solver(family, rec, cond, zero, 2.5, **thr)[0].sample(x, **skw)
    assert len(rec.calls) == 1 and rec.calls[0][0].thresholding == (tc.THR_RATIO, tc.THR_MAX, (True,) * 8)
    for extra in (dict(correcting_xt_fn=sampler_ref.standin_xt_fix), dict(thr, correcting_xt_fn=sampler_ref.standin_xt_fix)):
        rec = _StandinNative()
        gc.make_guided_solver(family, rec, cond, zero, 2.5, **extra)[0].sample(x, **skw)
        assert not rec.calls
    from diff_vits_amd.sampler import dpm_solver, uni_pc
    mod = dpm_solver if family == "dpm" else uni_pc
    ns = mod.NoiseScheduleVP("discrete", betas=torch.from_numpy(synth.make_betas()))
    make = (lambda fn: mod.DPM_Solver(fn, ns)) if family == "dpm" else (lambda fn: mod.UniPC(fn, ns, variant="bh2"))
    cfg_kw = dict(guidance_type="classifier-free", condition=cond, unconditional_condition=zero, guidance_scale=2.5)
    for wkw in (dict(cfg_kw, model_type="noise"), dict(cfg_kw, model_type="x_start", model_kwargs={"k": 1}),
                dict(model_type="x_start", guidance_type="classifier", condition=cond, guidance_scale=1.5,
                     classifier_fn=sampler_ref.standin_classifier)):
        rec = _StandinNative()
        make(mod.model_wrapper(rec, ns, **wkw)).sample(x, **skw)
        assert not rec.calls, wkw


@pytest.mark.gpu
def test_scale_one_runs_the_unguided_graph_at_B(cfg1, monkeypatch):
    """guidance_scale == 1 (and: no unconditional condition): the reference evaluates once, conditionally - the unguided graph
    with `condition` as the encoder states, the engine at B rows, bit-equal to the unguided wrapper around a model that holds
    that condition."""
    from diff_vits_amd.sampler import _plan, dpm_solver
    from sampler_cases import make_solver
    m, sd, ocfg = cfg1
    B = GRAPH_SHAPE[0]
    _, family, ctor, skw, *_ = gc.graph_set("cfg_dpmpp")
    x, cond, enc, mask, uenc, umask = gc.graph_inputs(B, "random")
    other = torch.from_numpy(synth.normal(4244, "other.enc", tuple(enc.shape))).cuda()      # what the model object holds: unused
    native = dpm_solver.NativeUNetModel(m, cond.cuda(), other, mask.cuda(), uncond_mask=umask.cuda())
    want = make_solver(family, dpm_solver.NativeUNetModel(m, cond.cuda(), enc.cuda(), mask.cuda()), None)[0].sample(x.cuda(), **skw)

    def stepped(*a, **k):
        raise AssertionError("a scale-1 guided wrapper left the native graph path")
    monkeypatch.setattr(_plan.Plan, "run_python", stepped)
    with torch.no_grad():
        for scale, u in ((1.0, uenc.cuda()), (2.0, None)):
            solver = gc.make_guided_solver(family, native, enc.cuda(), u, scale)[0]
            out = solver.sample(x.cuda(), **skw)
            assert m.hip_engine()._cur.prepared[0] == B
            assert all(p.guidance is None and not p._guided for p in solver._plans.values())
            assert torch.equal(out, want), (scale, rel_l2(out.cpu().numpy(), want.cpu().numpy()))


@pytest.mark.gpu
def test_guided_graph_holds_two_launches_more_per_evaluation(cfg1):
    """Counted on the captured graphs (dv_plan_graph_nodes): the guided graph at B = 2 against the unguided graph of the same
    plan at the batch the guided one evaluates (B = 4) - two nodes more per evaluation, one more per run (the condition)."""
    from diff_vits_amd.sampler import dpm_solver
    from sampler_cases import make_solver
    m, sd, ocfg = cfg1
    _, family, ctor, skw, B, g, uncond, thr = gc.graph_set("cfg_dpmpp")
    native, x, enc, uenc = _native(m, B, uncond)
    x4, cond4, enc4, mask4, *_ = gc.graph_inputs(2 * B, uncond)
    with torch.no_grad():
        solver = gc.make_guided_solver(family, native, enc.cuda(), uenc.cuda(), g, **ctor)[0]
        solver.sample(x.cuda(), **skw)
        plain = make_solver(family, dpm_solver.NativeUNetModel(m, cond4.cuda(), enc4.cuda(), mask4.cuda()), None, **ctor)[0]
        plain.sample(x4.cuda(), **skw)
    (gp,) = solver._plans.values()
    (pp,) = plain._plans.values()
    n_guided = max(p.graph_nodes() for p in gp._guided[g]._per_shape.values())
    n_plain = max(p.graph_nodes() for p in pp._per_shape.values())
    _report("cfg-graph nodes: guided B %d %d, unguided B %d %d, evaluations %d" % (B, n_guided, 2 * B, n_plain, gp.nfe))
    assert gp.graph_nodes() == 0                                   # the solver's own plan captured nothing
    assert n_plain > gp.nfe and n_guided == n_plain + 2 * gp.nfe + 1


@pytest.mark.gpu
def test_guided_run_without_condition_is_a_clear_error(cfg1):
    m, sd, ocfg = cfg1
    native, x, enc, uenc = _native(m, 1, "zeros")
    solver = gc.make_guided_solver("dpm", native, None, uenc.cuda(), 2.0)[0]
    with pytest.raises(ValueError, match="condition"):
        solver.sample(x.cuda(), steps=4, order=2)


@pytest.mark.gpu
def test_guided_and_unguided_runs_keep_their_own_graphs_and_stepped_agrees(cfg1):
    """One model object, guided and unguided runs interleaved: different plan handles, each run bit-equal to a fresh run of
    its own kind; the stepped guided run (return_intermediate=True: NativeUNetModel called with the pair) agrees with the
    graph within GRAPH_BOUND."""
    from sampler_cases import make_solver
    m, sd, ocfg = cfg1
    name = "cfg_thr_dpmpp"
    _, family, ctor, skw, B, g, uncond, thr = gc.graph_set(name)
    native, x, enc, uenc = _native(m, B, uncond)
    with torch.no_grad():
        solver = gc.make_guided_solver(family, native, enc.cuda(), uenc.cuda(), g, **ctor)[0]
        plain_solver = make_solver(family, native, None, **ctor)[0]
        guided1 = solver.sample(x.cuda(), **skw)
        plain1 = plain_solver.sample(x.cuda(), **skw)
        guided2 = solver.sample(x.cuda(), **skw)
        plain2 = plain_solver.sample(x.cuda(), **skw)
        fresh_native, *_ = _native(m, B, uncond)
        guided_fresh = gc.make_guided_solver(family, fresh_native, enc.cuda(), uenc.cuda(), g, **ctor)[0].sample(x.cuda(), **skw)
        plain_fresh = make_solver(family, fresh_native, None, **ctor)[0].sample(x.cuda(), **skw)
        stepped, inter = solver.sample(x.cuda(), return_intermediate=True, **skw)
    e_step = rel_l2(stepped.cpu().numpy(), guided1.cpu().numpy())
    e_eff = rel_l2(plain1.cpu().numpy(), guided1.cpu().numpy())
    _report("cfg-graph %-14s stepped vs graph %.3e  unguided vs guided %.3e  bound %.0e" % (name, e_step, e_eff, GRAPH_BOUND))
    assert torch.equal(guided1, guided2) and torch.equal(guided1, guided_fresh)
    assert torch.equal(plain1, plain2) and torch.equal(plain1, plain_fresh)
    assert e_eff > 100 * GRAPH_BOUND                               # the guidance is in the graph
    (plan,) = solver._plans.values()
    assert plan.guidance is None and list(plan._guided) == [g]
    handles = {p.handle.value for p in plan._guided[g]._per_shape.values()} | {plan.handle.value}
    handles |= {p.handle.value for sp in plain_solver._plans.values() for p in sp._per_shape.values()}
    assert len(handles) >= 3                                       # the solver's plan, its guided sibling, the plain solver's
    assert len(inter) == skw["steps"] + 1
    assert e_step < GRAPH_BOUND


# ============================================================================ 5. the product surface
def _ns2(gold, backend):
    from test_prompt_cpu import diffusion_state_dict, sample_case
    g, cfg, NaturalSpeech2, content, refer, noise = sample_case(gold)
    m = NaturalSpeech2(cfg, backend=backend).eval()
    m.diff_model.load_state_dict({k: torch.from_numpy(v) for k, v in diffusion_state_dict(cfg["diffusion_encoder"]).items()})
    return g, m.cuda(), content, refer, noise


# guidance of the product test: |1 - g| + |g| = 2 times the denoiser's recorded forward error (sampler_cases.GRAPH_PERTURBATION,
# 3.5e-5) per evaluation leaves the comparison well inside test_gpu_prompt.py's bound for sample()
PRODUCT_SCALE, PRODUCT_BOUND = 1.5, 5e-4


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["unipc", "dpmsolver"])
def test_sample_from_prior_with_guidance_hip_vs_torch_backend(method, gold, monkeypatch):
    """NaturalSpeech2.sample_from_prior(guidance_scale=, negative_refer=): the HIP backend (one graph: the stepped loop raises
    while it runs) against the torch backend of this package (the mirror's generic guided path), under the bound
    test_gpu_prompt.py uses for sample(); without a negative prompt too; with the defaults the output is bit-identical to a
    call without the new keywords."""
    from diff_vits_amd.sampler import _plan
    g, m_hip, content, refer, noise = _ns2(gold, "hip")
    _, m_ref, *_ = _ns2(gold, "torch")
    B, L = refer.shape[0], refer.shape[2]
    neg = torch.from_numpy(synth.normal(1234, "ns2.negative", (B, 100, L - 3))).cuda()
    neg_len = torch.full((B,), L - 5, dtype=torch.long).cuda()
    args = (torch.from_numpy(content).cuda(), torch.from_numpy(refer).cuda(), torch.from_numpy(g["text_lengths"]).cuda(),
            torch.from_numpy(g["spec_lengths"]).cuda(), None, method)
    kw = dict(noise=torch.from_numpy(noise).cuda())
    refs = [m_ref.sample_from_prior(*args, **kw, guidance_scale=PRODUCT_SCALE, negative_refer=neg, negative_lengths=neg_len)[1],
            m_ref.sample_from_prior(*args, **kw, guidance_scale=PRODUCT_SCALE)[1]]
    plain_ref = m_ref.sample_from_prior(*args, **kw)[1]
    base = m_hip.sample_from_prior(*args, **kw)[1]
    real = _plan.Plan.run_python

    def stepped(*a, **k):
        raise AssertionError("the guided product run left the native graph path")
    monkeypatch.setattr(_plan.Plan, "run_python", stepped)
    outs = [m_hip.sample_from_prior(*args, **kw, guidance_scale=PRODUCT_SCALE, negative_refer=neg, negative_lengths=neg_len)[1],
            m_hip.sample_from_prior(*args, **kw, guidance_scale=PRODUCT_SCALE)[1]]
    again = m_hip.sample_from_prior(*args, **kw, guidance_scale=PRODUCT_SCALE, negative_refer=neg, negative_lengths=neg_len)[1]
    default = m_hip.sample_from_prior(*args, **kw, guidance_scale=1.0, negative_refer=None)[1]
    monkeypatch.setattr(_plan.Plan, "run_python", real)
    errs = [rel_l2(o.cpu().numpy(), r.cpu().numpy()) for o, r in zip(outs, refs)]
    e_eff = rel_l2(plain_ref.cpu().numpy(), refs[0].cpu().numpy())
    _report("cfg-product %-9s negative prompt %.3e  zero states %.3e  bound %.0e  (guided vs plain %.3e)"
            % (method, errs[0], errs[1], PRODUCT_BOUND, e_eff))
    assert torch.equal(default, base)
    assert torch.equal(again, outs[0])
    assert e_eff > 100 * PRODUCT_BOUND and not torch.equal(refs[0], refs[1])
    assert max(errs) < PRODUCT_BOUND, errs
