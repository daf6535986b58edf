"""Known-frame correction (KnownFrames as correcting_xt_fn) on the host: the mirror, stepped, against the reference's outputs
(tests/golden/sampler_known_frames.npz, tools/make_golden_known_frames.py) at the tolerance of the hook keys of the same family
(sampler_cases.option_tolerance); the condition that makes those comparisons mean something; an fp64 restatement of the loop;
planted faults the golden comparison catches; the table the native plan exposes; argument validation."""
import numpy as np
import pytest
import torch

import known_frames_cases as kc
from conftest import rel_l2
from sampler_cases import option_tolerance

KEYS = sorted(kc.CASES)
MULTISTEP = [k for k in KEYS if kc.CASES[k][2].get("method", "multistep") == "multistep"]
_MIRROR = {}
# The native plan and the mirror's schedule both hold log alpha as the float32 cumulative sum the reference stores - one summed
# in order with the C library's logf, one by torch.cumsum - and part by a few float32 ulps of it, which is the relative distance
# of the two alphas.  The bound is the one the project applies to a compiled plan against the reference on this schedule.
TABLE_REL = option_tolerance(None)


def _mirror(key):
    """(final x, intermediates) of the mirror stepped with a KnownFrames, computed once per key."""
    if key not in _MIRROR:
        solver, _, _ = kc.mirror_solver(key)
        x, inter = solver.sample(kc.case_x(key), return_intermediate=True, **kc.CASES[key][2])
        _MIRROR[key] = (x, torch.stack(inter))
    return _MIRROR[key]


def _golden_distance(x, inter, g, key):
    """Largest relative L2 distance to the golden over the final x and every intermediate."""
    d = [rel_l2(np.asarray(x), g[key + "_x"])]
    gi = g[key + "_inter"]
    assert len(inter) == len(gi), (key, len(inter), len(gi))
    d += [rel_l2(np.asarray(a), b) for a, b in zip(inter, gi)]
    return max(d)


def test_cases_cover_every_route_of_the_event_loop(gold):
    g = gold("sampler_known_frames.npz")
    assert {k[:-2] for k in g.files if k.endswith("_x")} == set(kc.CASES)
    fam = {k: kc.CASES[k] for k in KEYS}
    assert any(f == "dpm" and kw["order"] == 2 and not c and "method" not in kw for f, c, kw in fam.values())
    assert any(f == "dpm" and kw["order"] == 3 and not c and "method" not in kw for f, c, kw in fam.values())
    assert any(c.get("algorithm_type") == "dpmsolver" for f, c, kw in fam.values())
    assert any(kw.get("method") == "singlestep" for f, c, kw in fam.values())
    assert any(kw.get("denoise_to_zero") for f, c, kw in fam.values())
    assert any(f == "unipc" and c.get("variant") == "bh2" and "algorithm_type" not in c for f, c, kw in fam.values())
    assert any(f == "unipc" and c.get("algorithm_type") == "noise_prediction" for f, c, kw in fam.values())
    keep = kc.case_keep()
    assert keep.shape == (2, 24) and not torch.equal(keep[0], keep[1])
    assert keep[0, :9].all() and not keep[0, 9:].any()                                # a prefix
    lo, hi = int(keep[1].nonzero()[0]), int(keep[1].nonzero()[-1]) + 1
    assert keep[1, lo:hi].all() and int(keep[1].sum()) == hi - lo and lo % 4 and hi % 4 and lo > 0 and hi < 24     # an interior span off the 4-grid
    for k in KEYS:
        assert g[k + "_x"].shape == kc.SHAPE


@pytest.mark.parametrize("key", KEYS)
def test_corrected_result_is_far_from_the_uncorrected_one(key, gold):
    """Every key's corrected reference result differs from the uncorrected run by at least 100 x the tolerance applied to it:
    no comparison below can pass with the correction missing."""
    g = gold("sampler_known_frames.npz")
    solver, _, _ = kc.mirror_solver(key, corrected=False)
    plain = solver.sample(kc.case_x(key), **kc.CASES[key][2])
    d = rel_l2(plain.numpy(), g[key + "_x"])
    print("%-12s corrected vs uncorrected %.3e  tolerance %.0e" % (key, d, kc.tolerance(key)))
    assert d >= 100 * kc.tolerance(key)


@pytest.mark.parametrize("key", KEYS)
def test_mirror_with_known_frames_matches_the_reference(key, gold):
    g = gold("sampler_known_frames.npz")
    x, inter = _mirror(key)
    d = _golden_distance(x, inter, g, key)
    print("%-12s mirror vs reference %.3e  tolerance %.0e" % (key, d, kc.tolerance(key)))
    assert d < kc.tolerance(key)
    keep = kc.case_keep(key)[:, None, :].expand(kc.SHAPE)
    plan = kc.plain_plan(key)
    # the kept frames end as alpha_0 known + sigma_0 eps of the last correction point: the plan's row against the mirror's
    # schedule (TABLE_REL apart at most) plus the roundings of a sum of two float32 products
    a, s = (float(v) for v in plan.known_coefs()[-1])
    mag = abs(a * kc.case_known(key)) + abs(s * kc.case_eps(key))
    assert ((x - (a * kc.case_known(key) + s * kc.case_eps(key))).abs() <= (TABLE_REL + 4 * 2.0 ** -23) * mag)[keep].all()


@pytest.mark.parametrize("key", KEYS)
def test_fp64_restatement_agrees_with_the_mirror(key, gold):
    x, inter = _mirror(key)
    rx, rinter = kc.restate(key)
    # (without a fault the restatement passes the comparison the planted faults must fail)
    assert _golden_distance(rx.numpy(), [v.numpy() for v in rinter], gold("sampler_known_frames.npz"), key) < kc.tolerance(key)
    assert len(rinter) == len(inter)
    d = max([rel_l2(x.numpy(), rx.numpy())] + [rel_l2(a.numpy(), b.numpy()) for a, b in zip(inter, rinter)])
    print("%-12s mirror vs fp64 restatement %.3e" % (key, d))
    assert d < kc.tolerance(key)


def _fault_cases():
    out = []
    for key in KEYS:
        for fault in kc.FAULTS:
            if fault in ("no_start", "start_early") and key not in MULTISTEP:
                continue          # (the singlestep methods do not correct their start point)
            out.append((key, fault))
    return out


@pytest.mark.parametrize("key,fault", _fault_cases())
def test_planted_faults_are_caught_by_the_golden_comparison(key, fault, gold):
    g = gold("sampler_known_frames.npz")
    x, inter = kc.restate(key, fault=fault)
    d = _golden_distance(x.numpy(), [v.numpy() for v in inter], g, key)
    print("%-12s %-12s distance to the reference %.3e  tolerance %.0e" % (key, fault, d, kc.tolerance(key)))
    assert d > kc.tolerance(key)


@pytest.mark.parametrize("key", KEYS)
def test_plan_table_is_the_schedule_at_the_points_of_the_hook(key):
    """dv_plan_known_coefs: one row per call of the hook in Plan.run_python, (alpha, sigma) of the mirror's schedule at that
    call's t, as floats."""
    solver, ns, _ = kc.mirror_solver(key, corrected=False)
    calls = []
    solver.correcting_xt_fn = lambda x, t, step: calls.append((float(t), step)) or x
    solver.sample(kc.case_x(key), **kc.CASES[key][2])
    rows = kc.plain_plan(key).known_coefs()
    assert rows.shape == (len(calls), 2) and rows.dtype == np.float32
    single = key not in MULTISTEP
    assert [s for _, s in calls] == list(range(len(calls)))
    assert len(calls) == len(kc.plain_plan(key).timesteps) - (1 if single else 0) + (1 if kc.CASES[key][2].get("denoise_to_zero") else 0)
    for (t, _), (a, s) in zip(calls, rows):
        t64 = torch.tensor([t], dtype=torch.float64)
        for got, want in ((a, float(ns.marginal_alpha(t64)[0])), (s, float(ns.marginal_std(t64)[0]))):
            assert abs(float(got) - want) <= TABLE_REL * want, (key, t, got, want)


def test_known_frames_validates_shapes():
    from diff_vits_amd.sampler import dpm_solver, uni_pc
    assert dpm_solver.KnownFrames is uni_pc.KnownFrames
    _, ns, _ = kc.mirror_solver("dpmpp_o2", corrected=False)
    known, keep = kc.case_known("dpmpp_o2"), kc.case_keep()
    KF = dpm_solver.KnownFrames
    a, b = KF(ns, known, keep, kc.case_eps("dpmpp_o2")), KF(ns, known, keep[:, None, :], kc.case_eps("dpmpp_o2"))
    x, t = kc.case_x("dpmpp_o2"), torch.tensor(0.5)
    assert torch.equal(a(x, t, 3), b(x, t, 3))
    assert not torch.equal(KF(ns, known, keep).noise, KF(ns, known, keep).noise)        # drawn at construction
    fixed = KF(ns, known, keep)
    assert torch.equal(fixed(x, t, 0), fixed(x, t, 1))                                   # ... once
    for bad in [dict(known=known[0]), dict(keep=keep[:1]), dict(keep=keep[:, :-1]), dict(keep=keep.float()),
                dict(keep=keep[:, None, None, :]), dict(noise=known[:, :, :-1]), dict(noise=known[:1])]:
        kw = dict(known=known, keep=keep, noise=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            KF(ns, kw["known"], kw["keep"], kw["noise"])
    with pytest.raises(ValueError):
        a(x[:, :, :-1], t, 0)


def test_plan_set_known_frames_validates_on_the_host():
    """Host only: refused before any HIP call; NULL switches off; a plan with the correction is refused by the form without rows."""
    import ctypes as C
    from diff_vits_amd import _lib as L
    plan = kc.plain_plan("dpmpp_o2")
    f = L.lib().dv_plan_set_known_frames
    buf = np.zeros(256, dtype=np.float32)
    p = C.c_void_p(buf.ctypes.data + (-buf.ctypes.data % 16))
    for args in [(p, None, p, 2, 5, 24), (p, p, None, 2, 5, 24), (p, p, p, 0, 5, 24), (p, p, p, 2, 0, 24), (p, p, p, 2, 5, 0),
                 (p, p, p, 2 ** 11, 2 ** 10, 2 ** 10)]:
        assert f(plan.handle, *args) == -1, args
    assert f(plan.handle, p, p, p, 2, 5, 24) == 0
    called = []
    cfn = L.MODEL_FN(lambda *a: called.append(1) or 1)
    assert L.lib().dv_sampler_run_custom(plan.handle, cfn, None, p, 240, None) == -1
    assert b"dv_sampler_run_custom_rows" in L.lib().dv_last_error()
    assert L.lib().dv_sampler_run_custom_rows(plan.handle, cfn, None, p, 3, 240, None) == -1          # rows do not match
    assert L.lib().dv_sampler_run_custom_rows(plan.handle, cfn, None, p, 2, 248, None) == -1          # nor the size
    assert not called
    assert f(plan.handle, None, None, None, 0, 0, 0) == 0
    assert L.lib().dv_op_known_frames(None, p, p, p, 2, 5, 24, 1.0, 0.0, None) == -1
    assert L.lib().dv_op_known_frames(p, p, p, p, 2, 5, 24, float("nan"), 0.0, None) == -1
