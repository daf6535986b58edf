"""GPU: the native sampler loop (run_events in csrc/sampler.hip, k_lincomb / k_lincomb_tail in csrc/kernels_misc.hip, the
hipGraph capture of dv_sampler_run) for every option the compiled plan expresses, against references that do not share its code:

  1. dv_sampler_run_custom around the analytic stand-in network, against the reference's outputs (tests/golden/
     sampler_options.npz) for every key the native plan expresses - and a host-only meta-test that those keys reach every route
     of the event loop;
  2. the element-count edges of the update kernels (tail only, every remainder mod 4, the grid-stride loop), the reuse of one
     plan's buffers across element counts, and the refusal of a misaligned x;
  3. the captured graph around the real denoiser with option sets, against the oracle sampler over the oracle denoiser.

Every test prints its figures before it asserts; with DVITS_SAMPLER_OPTIONS_REPORT=<file> they are appended to that file as
well (profiles/sampler_options_gpu.txt is such a record)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import oracle_cfg, rel_l2, unet_case
from diff_vits_amd import synth
from oracle import sampler_ref
from sampler_cases import (GRAPH_BOUND, GRAPH_OPTION_SETS, GRAPH_SHAPE, OPTION_CASES, make_solver, native_option_keys, option_tolerance,
                           oracle_sample, split_option_case)

DV_ERR_INVALID = -1


def _report(line):
    print(line)
    path = os.environ.get("DVITS_SAMPLER_OPTIONS_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _standin(xx, t, **kw):
    return sampler_ref.standin_model(xx, t)


def _plan_of(solver, steps, order, skip_type, t_start=None, t_end=None, denoise_to_zero=False, solver_type="dpmsolver",
             method="multistep"):
    """The plan DPM_Solver.sample / UniPC.sample compile for these keywords (their own cache entry)."""
    if hasattr(solver, "algorithm_type"):         # DPM_Solver
        return solver._plan(steps, order, skip_type, True, t_start, t_end, denoise_to_zero, solver_type, method)
    assert method == "multistep" and solver_type == "dpmsolver"
    return solver._plan(steps, order, skip_type, True, t_start, t_end, denoise_to_zero)


def _option_case(key):
    """(solver, plan, x, sample() keywords, tolerance) of a key of sampler_options.npz."""
    family, sched, algo, ualgo, variant, method, kw = split_option_case(key)
    kw.pop("return_intermediate", None)           # (the final x is compared; the plan is the same)
    ctor = dict(algorithm_type=algo) if family == "dpm" else dict(algorithm_type=ualgo, variant=variant)
    solver, _ = make_solver(family, _standin, sched, **ctor)
    x = torch.from_numpy(synth.normal(1234, "opts." + key, (2 if family == "dpm" else 1, 5, 24)))
    kw = dict(kw, method=method)
    return solver, _plan_of(solver, **kw), x, kw, option_tolerance(sched, method, algo, ualgo)


def _run_custom(plan, x_host, calls=None):
    """dv_sampler_run_custom on a device copy of x_host with a callback that stages through the host and evaluates the oracle's
    stand-in network there (the pattern of test_native_sampler_standin_custom_model)."""
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
            if calls is not None:
                calls.append(t_in)
            return 0 if hip.hipMemcpy(C.c_void_p(optr), out.ctypes.data_as(C.c_void_p), n * 4, 1) == 0 else 1
        except Exception as exc:        # (an exception cannot cross the C frame)
            print("stand-in callback failed:", exc)
            return 2

    cfn = L.MODEL_FN(cb)
    L.check(L.lib().dv_sampler_run_custom(plan.handle, cfn, None, L.ptr(x), n, None), "dv_sampler_run_custom")
    torch.cuda.synchronize()
    return x.cpu()


# ============================================================================ 1. stand-in network against the reference goldens
def test_the_native_option_keys_are_the_24_without_python_hooks(gold):
    g = gold("sampler_options.npz")
    keys = native_option_keys()
    assert len(keys) == 24, keys
    assert all(k + "_x" in g.files for k in keys)
    assert {k[:-2] for k in g.files if k.endswith("_x")} == set(OPTION_CASES)      # (42 keys: 24 + 7 with hooks, 6 guided / typed, 5 adaptive)


@pytest.mark.gpu
@pytest.mark.parametrize("key", native_option_keys())
def test_option_goldens_through_the_native_loop(key, gold):
    """dv_sampler_run_custom on the plan the product compiles for the key's keywords, against the reference's final x, at the
    tolerance test_sampler_options_match_reference applies to the key; the host mirror (Plan.run_python) beside it."""
    want = gold("sampler_options.npz")[key + "_x"]
    solver, plan, x, kw, tol = _option_case(key)
    calls = []
    got = _run_custom(plan, x, calls)
    mirror = solver.sample(x.clone(), **kw)
    e_gpu, e_cpu = rel_l2(got.numpy(), want), rel_l2(mirror.numpy(), want)
    _report("standin  %-24s gpu %.3e  cpu-mirror %.3e  tol %.0e" % (key, e_gpu, e_cpu, tol))
    assert len(calls) == plan.nfe
    assert np.array_equal(np.asarray(calls), plan.t_input)      # the callback sees the plan's per-evaluation time (t itself on a continuous schedule)
    assert e_gpu < tol, (key, e_gpu, tol)


# Solver ids the 24 keys do not reach: every UniPC key of sampler_options.npz without hooks runs 'bh2' except unipcn_vary_o4, and
# the one 'bh1' noise key (unipcn_bh1_o3_dtz) carries correction hooks.  'bh1' / 'vary_coeff' on the data prediction have
# reference outputs in sampler_standin.npz; for 'bh1' on the noise prediction the unipcn_bh1_o3_dtz keywords run without the hooks
# against the oracle (pinned to the reference at 1e-6 by test_sampler_options_match_reference).
EXTRA_SOLVER_CASES = {
    "unipc_s12_o5_bh1": dict(variant="bh1", steps=12, order=5, skip_type="time_uniform"),
    "unipc_s12_o4_vary_coeff": dict(variant="vary_coeff", steps=12, order=4, skip_type="time_uniform"),
    "unipcn_bh1_o3_dtz_nohooks": dict(variant="bh1", algorithm_type="noise_prediction", steps=9, order=3, skip_type="time_quadratic",
                                      denoise_to_zero=True),
}


def _extra_case(name, gold):
    kw = dict(EXTRA_SOLVER_CASES[name])
    ctor = dict(variant=kw.pop("variant"), algorithm_type=kw.pop("algorithm_type", "data_prediction"))
    solver, _ = make_solver("unipc", _standin, None, **ctor)
    if name.endswith("_nohooks"):
        x = torch.from_numpy(synth.normal(1234, "opts.unipcn_bh1_o3_dtz", (1, 5, 24)))
        want = oracle_sample("unipc", sampler_ref.standin_model, x.clone(), None, **ctor, **kw).numpy()
    else:
        g = gold("sampler_standin.npz")
        x, want = torch.from_numpy(g["x_sampler"][:1]), g[name + "_x"]
    return solver, _plan_of(solver, **kw), x, kw, want, option_tolerance(None, "multistep", "dpmsolver++", ctor["algorithm_type"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(EXTRA_SOLVER_CASES))
def test_solver_ids_outside_the_option_goldens_through_the_native_loop(name, gold):
    solver, plan, x, kw, want, tol = _extra_case(name, gold)
    got = _run_custom(plan, x)
    mirror = solver.sample(x.clone(), **kw)
    e_gpu, e_cpu = rel_l2(got.numpy(), want), rel_l2(mirror.numpy(), want)
    _report("standin  %-24s gpu %.3e  cpu-mirror %.3e  tol %.0e" % (name, e_gpu, e_cpu, tol))
    assert e_gpu < tol, (name, e_gpu, tol)


def test_selected_keys_reach_every_route_of_the_event_loop(gold):
    """Host only (the plan tables are compiled on the host): the keys of section 1 contain every route run_events and the two
    update kernels have - so a wrong slot index or branch there cannot hide behind the choice of cases."""
    seen = set()
    solvers, skips, scheds, methods = set(), set(), set(), set()
    for key in native_option_keys():
        family, sched, algo, ualgo, variant, method, kw = split_option_case(key)
        plan = _option_case(key)[1]
        solvers.add(plan._args[0])
        skips.add(kw["skip_type"])
        scheds.add("discrete" if sched is None else sched[0])
        methods.add(method)
        rows = plan.events.tolist()
        for typ, src, eidx, dst, coef, *slots in rows:
            c = plan.coefs[coef] if typ == 1 else None
            if typ == 0:
                seen.add("eval src=%d" % src)
                assert 0 <= dst < plan.n_slots
                continue
            assert all(s < plan.n_slots for s in slots)
            seen.add("comb dst=%s" % (dst if dst < 2 else ">=2"))
            if c[7] != 0:
                seen.add("coef7 src=%d" % src)
                assert dst >= 2 and slots[0] == dst - 2 and slots[1:] == [-1, -1, -1]      # in place on its own slot
                continue
            if all(s >= 0 for s in slots):
                seen.add("four slots")
                assert len(set(slots)) == 4
            if src == 1:
                seen.add("continued from x_pred")
                assert c[0] == 1.0
        if kw.get("denoise_to_zero"):
            typ, src, eidx, dst, coef, *slots = rows[-1]
            c = plan.coefs[coef]
            assert rows[-2][0] == 0 and typ == 1 and dst == 0 and c[0] == 0.0 and c[1] == 1.0 and not c[2:].any()
            assert slots == [rows[-2][3], -1, -1, -1]
            seen.add("denoise_to_zero row")
    assert seen >= {"eval src=0", "eval src=1", "comb dst=0", "comb dst=1", "comb dst=>=2", "coef7 src=0", "coef7 src=1",
                    "four slots", "continued from x_pred", "denoise_to_zero row"}, seen
    assert skips == {"time_uniform", "time_quadratic", "logSNR"}
    assert scheds == {"discrete", "linear", "cosine"}
    assert methods == {"multistep", "singlestep", "singlestep_fixed"}
    # DV_SOLVER_*: 0 dpmsolver++, 1-3 UniPC bh1 / bh2 / vary_coeff, 4 dpmsolver, 5 / 6 their Taylor forms, 7-9 UniPC on the noise
    assert solvers == {0, 2, 4, 5, 6, 8, 9}
    extra = {_extra_case(name, gold)[1]._args[0] for name in EXTRA_SOLVER_CASES}
    assert solvers | extra == set(range(10))


# ============================================================================ 2. element-count edges of the update kernels
# numel 3: k_lincomb_tail alone (no vector launch); 6 / 21 / 115: remainders 2 / 1 / 3 behind a vector launch; 2 200 003: above the
# 2048 x 256 float4 the grid is capped at (2 097 152 elements), remainder 3 - the grid-stride loop and the tail in one case
EDGE_SHAPES = {3: (1, 3), 6: (2, 3), 21: (1, 3, 7), 115: (1, 5, 23), 2200003: (1, 2200003)}
# a plain plan, a noise-form plan (the coef[7] branch, written in place into a history slot) and singlestep plans (x_pred as source
# and destination; in the noise form the in-place conversion reads x_pred): both branches of both kernels
EDGE_PLANS = {
    "dpmpp": ({}, dict(steps=4, order=2, skip_type="time_uniform")),
    "dpmn": (dict(algorithm_type="dpmsolver"), dict(steps=4, order=2, skip_type="time_uniform")),
    "ss_o3": ({}, dict(steps=4, order=3, skip_type="time_uniform", method="singlestep")),
    "dpmn_ss_o2": (dict(algorithm_type="dpmsolver"), dict(steps=4, order=2, skip_type="time_uniform", method="singlestep")),
}


def _edge_case(numel, plan_name):
    ctor, kw = EDGE_PLANS[plan_name]
    solver, _ = make_solver("dpm", _standin, None, **ctor)
    x = torch.from_numpy(synth.normal(77, "edge.%d" % numel, EDGE_SHAPES[numel]))
    tol = option_tolerance(None, kw.get("method", "multistep"), ctor.get("algorithm_type", "dpmsolver++"))
    return solver, _plan_of(solver, **kw), x, ctor, kw, tol


def test_edge_shapes_cover_every_remainder_and_the_grid_stride_loop():
    assert {n % 4 for n in EDGE_SHAPES} == {1, 2, 3} and min(EDGE_SHAPES) < 4
    big = max(EDGE_SHAPES)
    assert big // 4 > 2048 * 256 and big % 4 == 3
    assert all(int(np.prod(s)) == n for n, s in EDGE_SHAPES.items())
    for name in EDGE_PLANS:
        plan = _edge_case(3, name)[1]
        assert plan.nfe <= 4
        c7 = any(plan.coefs[r[4]][7] != 0 for r in plan.events.tolist() if r[0] == 1)
        assert c7 == ("algorithm_type" in EDGE_PLANS[name][0])


@pytest.mark.gpu
@pytest.mark.parametrize("plan_name", sorted(EDGE_PLANS))
@pytest.mark.parametrize("numel", sorted(EDGE_SHAPES))
def test_update_kernels_at_element_count_edges(numel, plan_name):
    """Every element against the oracle's sampler on the host around the same stand-in (the last ones are the tail kernel's)."""
    solver, plan, x, ctor, kw, tol = _edge_case(numel, plan_name)
    got = _run_custom(plan, x)
    want = oracle_sample("dpm", sampler_ref.standin_model, x.clone(), None, algorithm_type=ctor.get("algorithm_type"), **kw)
    err = rel_l2(got.numpy(), want.numpy())
    g, w = got.numpy().reshape(-1).astype(np.float64), want.numpy().reshape(-1).astype(np.float64)
    # per element, so that one stale or skipped element of 2.2 M cannot vanish in the norm: the values are O(1) (tanh-bounded
    # data predictions), an untouched element would be off by O(1)
    worst = float(np.abs(g - w).max() / np.abs(w).max())
    tail = float(np.abs(g[-(numel % 4):] - w[-(numel % 4):]).max() / np.abs(w).max())
    _report("edges    numel %-8d %-10s gpu %.3e  worst element %.3e  tail %.3e  tol %.0e" % (numel, plan_name, err, worst, tail, tol))
    assert err < tol, (numel, plan_name, err)
    assert worst < 10 * tol and tail < 10 * tol, (numel, plan_name, worst, tail)


@pytest.mark.gpu
def test_one_plan_reused_across_element_counts_equals_fresh_plans():
    """plan_buffers drops the graph and reallocates x_pred and the history slots when numel changes: A, B, A on one plan, each
    bit-equal to a fresh plan at that numel (the noise-form singlestep plan: x_pred and every slot are live)."""
    from diff_vits_amd.sampler._plan import Plan
    _, plan, _, _, _, _ = _edge_case(21, "dpmn_ss_o2")
    for numel in (21, 115, 21, 2200003, 6):
        x = torch.from_numpy(synth.normal(77, "edge.%d" % numel, EDGE_SHAPES[numel]))
        reused = _run_custom(plan, x)
        fresh = _run_custom(Plan(*plan._args), x)
        assert torch.equal(reused, fresh), numel


def test_run_custom_refuses_a_misaligned_x():
    """k_lincomb moves x as float4: an x_inout off the 16-byte grid is refused before anything is launched (the check comes
    before the first HIP call, so this needs no GPU; the callback never runs)."""
    from diff_vits_amd import _lib as L
    plan = _edge_case(6, "dpmpp")[1]
    buf = np.zeros(16, dtype=np.float32)
    called = []
    cfn = L.MODEL_FN(lambda *a: called.append(1) or 1)
    for off in range(1, 4):
        addr = buf.ctypes.data + 4 * ((off - buf.ctypes.data // 4) % 4)      # address = 4 * off (mod 16)
        assert addr % 16 == 4 * off
        rc = L.lib().dv_sampler_run_custom(plan.handle, cfn, None, C.c_void_p(addr), 6, None)
        assert rc == DV_ERR_INVALID and b"16-byte aligned" in L.lib().dv_last_error()
    assert not called


# ============================================================================ 3. the captured graph with options
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


@pytest.mark.gpu
@pytest.mark.parametrize("name", [s[0] for s in GRAPH_OPTION_SETS])
def test_graph_path_with_options_vs_oracle(name, cfg1, monkeypatch):
    """DPM_Solver.sample / UniPC.sample around NativeUNetModel (dv_sampler_run: captured once, replayed) on the padded row
    space with a ragged prompt mask, against the oracle's sampler over the oracle's denoiser; twice, bit-equal."""
    from diff_vits_amd.sampler import _plan, dpm_solver
    m, x, cond, enc, mask, oracle = cfg1
    _, family, ctor, skw = next(s for s in GRAPH_OPTION_SETS if s[0] == name)
    ctor = dict(ctor)
    sched = ctor.pop("schedule", None)

    def stepped(*a, **k):
        raise AssertionError("the option set left the native graph path")
    monkeypatch.setattr(_plan.Plan, "run_python", stepped)
    native = dpm_solver.NativeUNetModel(m, cond.cuda(), enc.cuda(), mask.cuda())
    solver, _ = make_solver(family, native, sched, **ctor)
    with torch.no_grad():
        out1 = solver.sample(x.cuda(), **skw)
        out2 = solver.sample(x.cuda(), **skw)
        ref = oracle_sample(family, oracle, x.clone(), sched, algorithm_type=ctor.get("algorithm_type"),
                            variant=ctor.get("variant", "bh2"), **skw)
    err = rel_l2(out1.cpu().numpy(), ref.numpy())
    _report("graph    %-24s gpu %.3e  bound %.0e" % (name, err, GRAPH_BOUND))
    assert torch.equal(out1, out2)
    assert m.hip_engine().handover_status()[1] == 0
    assert err < GRAPH_BOUND, (name, err)


@pytest.mark.gpu
def test_sampler_run_refuses_a_misaligned_x(cfg1):
    from diff_vits_amd import _lib as L
    m = cfg1[0]
    plan = _edge_case(6, "dpmpp")[1]
    x = torch.zeros(2 * 80 * 75 + 4, device="cuda")
    assert x.data_ptr() % 16 == 0
    for off in range(1, 4):
        rc = L.lib().dv_sampler_run(plan.handle, m.hip_engine().handle, L.ptr(x[off:]), None, None)
        assert rc == DV_ERR_INVALID and b"16-byte aligned" in L.lib().dv_last_error()
