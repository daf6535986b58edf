"""Known-frame correction inside the native sampler loop (csrc/kernels_known.hip, dv_plan_set_known_frames, the routing of
DPM_Solver / UniPC with a KnownFrames, NaturalSpeech2.sample_from_prior(known_mel=, known_mask=)):

  1. dv_op_known_frames against the float32 torch expression on the host, bit for bit, at the edges of both routes of the kernel;
  2. dv_sampler_run_custom_rows around the stand-in network of known_frames_cases on every key, against the reference's outputs
     (tests/golden/sampler_known_frames.npz);
  3. the captured graph around the real denoiser against the same solver stepped, the graph's node count, replay, switching off;
  4. together with in-graph thresholding, guidance and enrolled voices;
  5. the product surface, HIP backend against torch backend.

Every test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

import guidance_cases as gc
import known_frames_cases as kc
import thresholding_cases as tc
from conftest import rel_l2, unet_case
from diff_vits_amd import synth
from sampler_cases import GRAPH_BOUND, GRAPH_SHAPE, make_solver

pytestmark = pytest.mark.gpu

DV_ERR_INVALID = -1
ULP = 2.0 ** -23


# ============================================================================ 1. the operator
OP_SHAPES = [(1, 1, 1), (1, 5, 3), (2, 5, 23), (2, 5, 24), (3, 80, 99), (3, 80, 300), (8, 80, 4096)]
OP_ALPHA, OP_SIGMA = 0.8372, 0.5469


def _op_masks(rows, T):
    rnd = torch.from_numpy(synth.normal(91, "kf.op.mask.%d.%d" % (rows, T), (rows, T))) > 0.3
    if T >= 12:           # every branch of a 4-frame group, whatever was drawn: all kept, none kept, some kept
        rnd[0, :12] = torch.tensor([1, 1, 1, 1, 0, 0, 0, 0, 0, 1, 1, 0], dtype=torch.bool)
    return {"zero": torch.zeros(rows, T, dtype=torch.bool), "one": torch.ones(rows, T, dtype=torch.bool), "random": rnd}


def test_operator_shapes_reach_both_routes_and_the_grid_stride():
    """Host arithmetic only: T % 4 == 0 and T % 4 != 0, one block and several, and one shape with more quads than one trip of
    the largest grid (2048 blocks of 256) covers; the random masks are mixed and differ per row."""
    assert {T % 4 == 0 for _, _, T in OP_SHAPES} == {True, False}
    assert any(r * c * T <= 256 for r, c, T in OP_SHAPES) and any(256 < r * c * T < 2048 * 256 for r, c, T in OP_SHAPES)
    r, c, T = OP_SHAPES[-1]
    assert T % 4 == 0 and r * c * T // 4 > 2048 * 256
    for r, c, T in OP_SHAPES[2:]:
        keep = _op_masks(r, T)["random"]
        assert 0 < int(keep.sum()) < r * T and not torch.equal(keep[0], keep[-1])
        if T % 4 == 0:
            quads = keep.reshape(r, T // 4, 4).sum(-1)
            assert (quads == 0).any() and (quads == 4).any() and ((quads > 0) & (quads < 4)).any()       # every branch of a quad


@pytest.mark.parametrize("shape", OP_SHAPES)
def test_operator_is_the_torch_expression_bit_for_bit(shape):
    from diff_vits_amd import _lib as L
    rows, ch, T = shape
    x, known, eps = (torch.from_numpy(synth.normal(91, "kf.op.%s.%d.%d.%d" % (n, rows, ch, T), shape)) for n in ("x", "known", "eps"))
    a, s = float(np.float32(OP_ALPHA)), float(np.float32(OP_SIGMA))
    value = a * known + s * eps                                                  # float32: three roundings
    dk, de = known.cuda(), eps.cuda()
    for name, keep in _op_masks(rows, T).items():
        want = torch.where(keep[:, None, :], value, x)
        dx, dm = x.cuda().contiguous(), keep.to(torch.uint8).cuda()
        L.check(L.lib().dv_op_known_frames(L.ptr(dx), L.ptr(dk), L.ptr(de), L.ptr(dm), rows, ch, T, OP_ALPHA, OP_SIGMA, L.stream_ptr()),
                "dv_op_known_frames")
        got = dx.cpu()
        print("op %-14s mask %-6s kept %d of %d frames  equal %s" % (shape, name, int(keep.sum()), rows * T, torch.equal(got, want)))
        assert torch.equal(got, want), (shape, name)
        if name == "zero":
            assert torch.equal(got, x)


def test_operator_takes_the_scalar_route_for_unaligned_views():
    """T % 4 == 0 but x one float off the 16-byte grid: the same result through the other kernel."""
    from diff_vits_amd import _lib as L
    rows, ch, T = 2, 5, 24
    x, known, eps = (torch.from_numpy(synth.normal(91, "kf.op.%s.%d.%d.%d" % (n, rows, ch, T), (rows, ch, T))) for n in ("x", "known", "eps"))
    keep = _op_masks(rows, T)["random"]
    a, s = float(np.float32(OP_ALPHA)), float(np.float32(OP_SIGMA))
    want = torch.where(keep[:, None, :], a * known + s * eps, x)
    buf = torch.zeros(rows * ch * T + 1, device="cuda")
    dx = buf[1:].view(rows, ch, T)
    dx.copy_(x)
    assert dx.data_ptr() % 16 == 4
    dk, de, dm = known.cuda(), eps.cuda(), keep.to(torch.uint8).cuda()
    L.check(L.lib().dv_op_known_frames(C.c_void_p(dx.data_ptr()), L.ptr(dk), L.ptr(de), L.ptr(dm), rows, ch, T, OP_ALPHA, OP_SIGMA,
                                       L.stream_ptr()), "dv_op_known_frames")
    assert torch.equal(dx.cpu(), want) and float(buf[0]) == 0.0


# ============================================================================ 2. the stand-in network through the native loop
def _run_custom_rows(plan, x_host, entry="dv_sampler_run_custom_rows"):
    """dv_sampler_run_custom_rows on a device copy of x_host [rows, ...]; the callback stages through the host and evaluates
    known_frames_cases.kf_model there.  Returns (return code, x)."""
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
            out = np.ascontiguousarray(kc.kf_model(torch.from_numpy(host).reshape(shape), t).numpy(), dtype=np.float32)
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


def _bound_standin_plan(key):
    """A plan of the key with the case's known / eps / keep bound; returns (plan, the device tensors it reads)."""
    from diff_vits_amd.sampler._plan import Plan
    plan = Plan(*kc.plain_plan(key)._args[:13], known_frames=True)
    bufs = (kc.case_known(key).cuda(), kc.case_eps(key).cuda(), kc.case_keep(key).to(torch.uint8).cuda())
    plan.bind_known_frames(*bufs)
    return plan, bufs


@pytest.mark.parametrize("key", sorted(kc.CASES))
def test_standin_with_known_frames_through_the_native_loop(key, gold):
    want = gold("sampler_known_frames.npz")[key + "_x"]
    tol = kc.tolerance(key)
    plan, bufs = _bound_standin_plan(key)
    rc, got = _run_custom_rows(plan, kc.case_x(key))
    assert rc == 0
    err = rel_l2(got.numpy(), want)
    print("kf-standin %-12s gpu vs reference %.3e  tol %.0e" % (key, err, tol))
    assert err < tol, (key, err, tol)


def test_run_custom_refuses_a_plan_with_known_frames():
    plan, bufs = _bound_standin_plan("dpmpp_o2")
    x = kc.case_x("dpmpp_o2")
    rc, got = _run_custom_rows(plan, x, entry="dv_sampler_run_custom")
    assert rc == DV_ERR_INVALID and torch.equal(got, x)
    plan.bind_known_frames(None, None, None)
    rc, off = _run_custom_rows(plan, x, entry="dv_sampler_run_custom")
    rc2, plain = _run_custom_rows(kc.plain_plan("dpmpp_o2"), x)
    assert rc == 0 and rc2 == 0 and torch.equal(off, plain)


# ============================================================================ 3. the captured graph around the real denoiser
@pytest.fixture(scope="module")
def cfg1():
    from diff_vits_amd.unet1d.unet_1d_condition import UNet1DConditionModel
    kw, sd, *_ = unet_case("cfg1")
    m = UNet1DConditionModel(backend="hip", **kw).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.cuda()
    m.hip_engine("bf16x3")
    return m


def _graph_known(ns, shape, tag="a"):
    """A KnownFrames for x of `shape`: a prefix in row 0, interior spans (off the 4-frame grid) in the others."""
    from diff_vits_amd.sampler import dpm_solver
    B, _, T = shape
    known = 0.5 * torch.from_numpy(synth.normal(4242, "kf.graph.known." + tag, shape))
    eps = torch.from_numpy(synth.normal(4242, "kf.graph.eps." + tag, shape))
    keep = torch.zeros(B, T, dtype=torch.bool)
    off = 0 if tag == "a" else 7
    keep[0, :T // 3 + off] = True
    for b in range(1, B):
        keep[b, 21 + b + off:T - 24 + b] = True
    return dpm_solver.KnownFrames(ns, known.cuda(), keep.cuda(), eps.cuda())


def _kept_frames_check(out, kf, plan):
    a, s = (float(v) for v in plan.known_coefs()[-1])
    keep = kf.keep.expand_as(out)
    ak, se = a * kf.known, s * kf.noise
    excess = ((out - (ak + se)).abs() - 4 * ULP * (ak.abs() + se.abs()))[keep]
    return float(excess.max())


def _nodes(plan):
    return [p.graph_nodes() for p in plan._per_shape.values()]


_SKW = dict(steps=8, order=2, skip_type="time_uniform", t_end=0.05)


@pytest.mark.parametrize("family", ["dpm", "unipc"])
def test_graph_with_known_frames_vs_the_stepped_solver(family, cfg1, monkeypatch):
    from diff_vits_amd.sampler import _plan, dpm_solver
    m = cfg1
    B, T, L = GRAPH_SHAPE
    x, cond, enc, mask = (torch.from_numpy(a) for a in synth.make_inputs(B, 80, T, L, seed=4242, ragged_mask=True))
    native = dpm_solver.NativeUNetModel(m, cond.cuda(), enc.cuda(), mask.cuda())
    solver, ns = make_solver(family, native, None)
    plain_solver, _ = make_solver(family, native, None)
    kf = _graph_known(ns, x.shape)
    solver.correcting_xt_fn = kf
    real = _plan.Plan.run_python

    def stepped(*a, **k):
        raise AssertionError("the known-frame correction left the native graph path")
    monkeypatch.setattr(_plan.Plan, "run_python", stepped)
    with torch.no_grad():
        out = solver.sample(x.cuda(), **_SKW)
        out_again = solver.sample(x.cuda(), **_SKW)
        plain = plain_solver.sample(x.cuda(), **_SKW)
    monkeypatch.setattr(_plan.Plan, "run_python", real)
    with torch.no_grad():
        ref, inter = solver.sample(x.cuda(), return_intermediate=True, **_SKW)
    kf_plans = [p for p in solver._plans.values() if p.known_frames]
    assert len(kf_plans) == 1 and len(solver._plans) == 2          # (the stepped run uses the plain plan: its hook is Python's)
    plan = kf_plans[0]
    (plain_plan,) = plain_solver._plans.values()
    err, eff = rel_l2(out.cpu().numpy(), ref.cpu().numpy()), rel_l2(plain.cpu().numpy(), out.cpu().numpy())
    excess = _kept_frames_check(out, kf, plan)
    n_rows = len(plan.known_coefs())
    print("kf-graph %-5s graph vs stepped %.3e  bound %.0e  corrected vs plain %.3e  kept frames over their bound by %.3e  nodes %s plain %s rows %d"
          % (family, err, GRAPH_BOUND, eff, excess, _nodes(plan), _nodes(plain_plan), n_rows))
    assert torch.equal(out, out_again)
    assert m.hip_engine().handover_status()[1] == 0
    assert eff > 100 * GRAPH_BOUND                                 # the correction is in the graph
    assert err < GRAPH_BOUND
    assert excess <= 0.0
    assert n_rows == _SKW["steps"] + 1 and len(inter) == n_rows
    assert len(_nodes(plan)) == 1 and len(_nodes(plain_plan)) == 1 and _nodes(plain_plan)[0] > 0
    assert _nodes(plan)[0] == _nodes(plain_plan)[0] + n_rows       # one launch per correction point, exactly
    assert {p.handle.value for p in plan._per_shape.values()}.isdisjoint(p.handle.value for p in plain_plan._per_shape.values())

    # a second utterance of the same shape, other known frames and another mask: the graph is replayed
    handles, builds = [p.handle.value for p in plan._per_shape.values()], m.hip_engine().plan_builds
    kf2 = _graph_known(ns, x.shape, tag="b")
    assert not torch.equal(kf2.keep, kf.keep)
    solver.correcting_xt_fn = kf2
    with torch.no_grad():
        out2 = solver.sample(x.cuda(), **_SKW)
        ref2, _ = solver.sample(x.cuda(), return_intermediate=True, **_SKW)
    err2 = rel_l2(out2.cpu().numpy(), ref2.cpu().numpy())
    print("kf-graph %-5s second utterance: graph vs stepped %.3e" % (family, err2))
    assert err2 < GRAPH_BOUND and _kept_frames_check(out2, kf2, plan) <= 0.0 and not torch.equal(out2, out)
    assert [p.handle.value for p in plan._per_shape.values()] == handles and m.hip_engine().plan_builds == builds
    assert _nodes(plan)[0] == _nodes(plain_plan)[0] + n_rows

    # switched off on the plan that holds the graph: the next run is the plain plan's, bit for bit
    for p in list(plan._per_shape.values()):
        p.bind_known_frames(None, None, None)
    with torch.no_grad():
        off = native.run_plan(plan, x.cuda())
    assert torch.equal(off, plain)


def test_sampler_run_refuses_known_frames_of_another_shape(cfg1):
    from diff_vits_amd import _lib as L
    from diff_vits_amd.sampler import dpm_solver
    m = cfg1
    B, T, Lk = GRAPH_SHAPE
    x, cond, enc, mask = (torch.from_numpy(a).cuda() for a in synth.make_inputs(B, 80, T, Lk, seed=4242, ragged_mask=True))
    native = dpm_solver.NativeUNetModel(m, cond, enc, mask)
    solver, ns = make_solver("dpm", native, None)
    with torch.no_grad():
        want = solver.sample(x, **_SKW)
    (plan,) = solver._plans.values()
    (p,) = plan._per_shape.values()
    bufs = (torch.zeros(B, 80, T - 1, device="cuda"), torch.zeros(B, 80, T - 1, device="cuda"), torch.zeros(B, T - 1, dtype=torch.uint8, device="cuda"))
    p.bind_known_frames(*bufs)
    xb = x.clone()
    rc = L.lib().dv_sampler_run(p.handle, m.hip_engine().handle, L.ptr(xb), L.ptr(cond), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == DV_ERR_INVALID and b"known frames" in L.lib().dv_last_error() and torch.equal(xb, x)
    p.bind_known_frames(None, None, None)
    with torch.no_grad():
        assert torch.equal(solver.sample(x, **_SKW), want)


# ============================================================================ 4. combinations
_THR_CTOR = dict(correcting_x0_fn="dynamic_thresholding", dynamic_thresholding_ratio=tc.GRAPH_THR_RATIO,
                 thresholding_max_val=tc.GRAPH_THR_MAX)


def _native_then_stepped(solver, x, monkeypatch):
    """(graph result - the stepped loop raises while it runs -, stepped result) of one solver."""
    from diff_vits_amd.sampler import _plan
    real = _plan.Plan.run_python

    def stepped(*a, **k):
        raise AssertionError("the run left the native graph path")
    monkeypatch.setattr(_plan.Plan, "run_python", stepped)
    with torch.no_grad():
        out = solver.sample(x, **_SKW)
    monkeypatch.setattr(_plan.Plan, "run_python", real)
    with torch.no_grad():
        ref, _ = solver.sample(x, return_intermediate=True, **_SKW)
    return out, ref


def test_known_frames_with_in_graph_thresholding(cfg1, monkeypatch):
    from diff_vits_amd.sampler import dpm_solver
    m = cfg1
    B, T, L = GRAPH_SHAPE
    x, cond, enc, mask = (torch.from_numpy(a).cuda() for a in synth.make_inputs(B, 80, T, L, seed=4242, ragged_mask=True))
    native = dpm_solver.NativeUNetModel(m, cond, enc, mask)
    solver, ns = make_solver("dpm", native, None, **_THR_CTOR)
    kf = _graph_known(ns, x.shape)
    solver.correcting_xt_fn = kf
    out, ref = _native_then_stepped(solver, x, monkeypatch)
    with torch.no_grad():
        only_thr = make_solver("dpm", native, None, **_THR_CTOR)[0].sample(x, **_SKW)
        only_kf_solver = make_solver("dpm", native, None)[0]
        only_kf_solver.correcting_xt_fn = kf
        only_kf = only_kf_solver.sample(x, **_SKW)
    plan = next(p for p in solver._plans.values() if p.known_frames)
    err = rel_l2(out.cpu().numpy(), ref.cpu().numpy())
    e_thr, e_kf = rel_l2(only_kf.cpu().numpy(), out.cpu().numpy()), rel_l2(only_thr.cpu().numpy(), out.cpu().numpy())
    print("kf+thr   graph vs stepped %.3e  bound %.0e  without thresholding %.3e  without known frames %.3e" % (err, GRAPH_BOUND, e_thr, e_kf))
    assert plan.thresholding is not None and all(plan.thresholding[2])
    assert err < GRAPH_BOUND and _kept_frames_check(out, kf, plan) <= 0.0
    assert e_thr > 100 * GRAPH_BOUND and e_kf > 100 * GRAPH_BOUND          # both corrections are in the graph


def test_known_frames_with_guidance(cfg1, monkeypatch):
    """B rows of x (and of known / eps / keep), 2B rows in the network."""
    m = cfg1
    _, family, ctor, skw, B, g, uncond, _ = gc.graph_set("cfg_dpmpp")
    from diff_vits_amd.sampler import dpm_solver
    x, cond, enc, mask, uenc, umask = gc.graph_inputs(B, uncond)
    native = dpm_solver.NativeUNetModel(m, cond.cuda(), enc.cuda(), mask.cuda())
    solver, _, ns = gc.make_guided_solver(family, native, enc.cuda(), uenc.cuda(), g, **ctor)
    kf = _graph_known(ns, x.shape)
    solver.correcting_xt_fn = kf
    out, ref = _native_then_stepped(solver, x.cuda(), monkeypatch)
    with torch.no_grad():
        unguided_solver = make_solver(family, native, None, **ctor)[0]
        unguided_solver.correcting_xt_fn = kf
        unguided = unguided_solver.sample(x.cuda(), **_SKW)
    plan = next(p for p in solver._plans.values() if p.known_frames)
    guided_plan = plan._guided[g]
    err, eff = rel_l2(out.cpu().numpy(), ref.cpu().numpy()), rel_l2(unguided.cpu().numpy(), out.cpu().numpy())
    print("kf+cfg   graph vs stepped %.3e  bound %.0e  guided vs unguided %.3e  x rows %d" % (err, GRAPH_BOUND, eff, B))
    assert guided_plan.known_frames and guided_plan.guidance == g
    assert err < GRAPH_BOUND and _kept_frames_check(out, kf, guided_plan) <= 0.0
    assert eff > 100 * GRAPH_BOUND
    assert m.hip_engine().handover_status()[1] == 0


def test_known_frames_with_enrolled_voices():
    """Voices cannot be stepped: the run with bound voices against the `refer` route (set_cond on the same prompts), bit for bit."""
    import test_gpu_voices as tv
    from diff_vits_amd.sampler import dpm_solver
    m = tv.make_unet()
    eng = m.hip_engine()
    P, Pm = tv.prompts("P")
    x, cond, _ = tv.inputs(tv.B, tv.T)
    eng.prepare(tv.B, tv.T, tv.L)
    voices = eng.enroll(P, m._bias_from_mask(Pm, torch.float32))
    nm = dpm_solver.NativeUNetModel(m, cond, P, Pm)
    solver, ns = make_solver("dpm", nm, None)
    kf = _graph_known(ns, x.shape)
    solver.correcting_xt_fn = kf
    skw = dict(steps=3, order=2, skip_type="time_uniform", method="multistep")
    with torch.no_grad():
        mel_ref = solver.sample(x, **skw)
        nm.voices = voices
        mel_v = solver.sample(x, **skw)
        nm.voices = None
        solver.correcting_xt_fn = None
        plain = solver.sample(x, **skw)
    torch.cuda.synchronize()
    plan = next(p for p in solver._plans.values() if p.known_frames)
    print("kf+voices equal %s  corrected vs plain %.3e" % (torch.equal(mel_v, mel_ref), rel_l2(plain.cpu().numpy(), mel_ref.cpu().numpy())))
    assert torch.isfinite(mel_ref).all() and torch.equal(mel_v, mel_ref)
    assert _kept_frames_check(mel_v, kf, plan) <= 0.0 and not torch.equal(plain, mel_ref)
    assert len(_nodes(plan)) == 1                                  # one graph for both routes


# ============================================================================ 5. the product surface
PRODUCT_BOUND = 5e-4        # tests/test_gpu_prompt.py: sample() on the HIP backend against the reference


def _ns2(gold, backend):
    from test_prompt_cpu import diffusion_state_dict, sample_case
    g, cfg, NaturalSpeech2, content, refer, noise = sample_case(gold)
    m = NaturalSpeech2(cfg, backend=backend).eval()
    m.diff_model.load_state_dict({k: torch.from_numpy(v) for k, v in diffusion_state_dict(cfg["diffusion_encoder"]).items()})
    return g, m.cuda(), content, refer, noise


@pytest.mark.parametrize("method", ["unipc", "dpmsolver"])
def test_sample_from_prior_with_known_mel_hip_vs_torch_backend(method, gold, monkeypatch):
    from diff_vits_amd.sampler import _plan
    g, m_hip, content, refer, noise = _ns2(gold, "hip")
    _, m_ref, *_ = _ns2(gold, "torch")
    B, D, T = noise.shape
    known = 0.5 * torch.from_numpy(synth.normal(1234, "ns2.known", (B, D, T))).cuda()
    mask = torch.zeros(B, T, dtype=torch.bool)
    mask[:, 3:T // 2 + 1] = True
    mask = mask.cuda()
    args = (torch.from_numpy(content).cuda(), torch.from_numpy(refer).cuda(), torch.from_numpy(g["text_lengths"]).cuda(),
            torch.from_numpy(g["spec_lengths"]).cuda(), None, method)
    kw = dict(noise=torch.from_numpy(noise).cuda())
    ref = m_ref.sample_from_prior(*args, **kw, known_mel=known, known_mask=mask)[1]
    ref_raw = m_ref.sample_from_prior(*args, **kw, known_mel=known, known_mask=mask, paste_known=False)[1]
    base = m_hip.sample_from_prior(*args, **kw)[1]
    real = _plan.Plan.run_python

    def stepped(*a, **k):
        raise AssertionError("the product run with known frames left the native graph path")
    monkeypatch.setattr(_plan.Plan, "run_python", stepped)
    out = m_hip.sample_from_prior(*args, **kw, known_mel=known, known_mask=mask)[1]
    raw = m_hip.sample_from_prior(*args, **kw, known_mel=known, known_mask=mask, paste_known=False)[1]
    none_kept = m_hip.sample_from_prior(*args, **kw, known_mel=known, known_mask=torch.zeros_like(mask))[1]
    after = m_hip.sample_from_prior(*args, **kw)[1]
    monkeypatch.setattr(_plan.Plan, "run_python", real)
    keep = mask[:, None, :].expand_as(out)
    err, err_raw = rel_l2(out.cpu().numpy(), ref.cpu().numpy()), rel_l2(raw.cpu().numpy(), ref_raw.cpu().numpy())
    eff = rel_l2(base.cpu().numpy(), out.cpu().numpy())
    print("kf-product %-9s hip vs torch backend %.3e (unpasted %.3e)  bound %.0e  corrected vs plain %.3e" % (method, err, err_raw, PRODUCT_BOUND, eff))
    assert torch.equal(out[keep], known[keep]) and torch.equal(ref[keep], known[keep])
    assert not torch.equal(raw[keep], known[keep]) and torch.equal(raw[~keep], out[~keep])
    assert torch.equal(none_kept, base) and torch.equal(after, base)
    assert eff > 100 * PRODUCT_BOUND
    assert err < PRODUCT_BOUND and err_raw < PRODUCT_BOUND
    with pytest.raises(ValueError):
        m_hip.sample_from_prior(*args, **kw, known_mel=known)
    with pytest.raises(ValueError):
        m_hip.sample_from_prior(*args, **kw, known_mel=known[:, :, :-1], known_mask=mask)
