"""Native posterior encoder, layer by layer and frame by frame (dv_qenc_*, csrc/kernels_wn.hip): every probe and z / m / logs of
every case of tests/qenc_cases.py, with g and without, against the float32 torch reference on the valid frames:
  whole tensor < 2e-4, every frame < 1e-3, localisation < 3 x the largest ratio the float32 reference shows against float64 on these
  very cases (qenc_cases.localisation_bound), every padding frame exactly zero;
  every layerN.acts also in isolation: against the float64 activations of the engine's OWN layer input, every frame below the bound
  the host emulation of the documented arithmetic gives for that input (qenc_cases.acts_bound: about 2.6e-5).
Without a tolerance: two forwards are identical, replacing one utterance leaves the others' valid frames bit-equal, a forward replayed
from a captured graph equals the eager one, probe raises without keep mode, n_layers + 4 launches in both modes.
DVITS_PARITY_REPORT=1 writes profiles/parity_localisation_qenc_hip.txt."""
import os

import numpy as np
import pytest
import torch

import parity_metrics as pm
import qenc_cases as qc

pytestmark = pytest.mark.gpu

TENSOR_BOUND, FRAME_BOUND = 2e-4, pm.FRAME_BOUND
N_LAUNCH = qc.CFG["n_layers"] + 4
_REPORT = []


@pytest.fixture(scope="module")
def module():
    return qc.make_module(backend="hip").cuda()


@pytest.fixture(scope="module")
def loc_bound():
    return qc.localisation_bound()[0]


@pytest.fixture(scope="module")
def weights():
    return qc.make_weights()


def _dev(a):
    return None if a is None else torch.from_numpy(np.asarray(a)).cuda()


def _run(module, name, with_g, keep, monkeypatch):
    monkeypatch.setenv("DVITS_KEEP_INTERMEDIATES", "1" if keep else "0")
    eng = module.hip_engine()
    eng._prepared = None                                         # the keep flag is read at prepare time
    y, lengths, g, noise = qc.make_inputs(name)
    z, m, logs, mask = module(_dev(y), _dev(lengths), _dev(g) if with_g else None, noise=_dev(noise))
    torch.cuda.synchronize()
    return eng, (z, m, logs), mask


def _check(label, got, want, lengths, loc_bound):
    """got / want channels-last [B, T, C]; the criteria of the module docstring."""
    got, want = got.detach().cpu(), want.detach().cpu()
    rows = qc.valid_rows(lengths)
    for b in range(len(lengths)):
        assert not got[b, lengths[b]:].any(), "%s: padding frame of utterance %d is not zero" % (label, b)
    n = [lengths[b] for b in rows]
    sv = pm.split_valid(got[rows], want[rows], n)
    fe = pm.frame_errors(sv["got"], sv["want"])
    loc = fe["worst"] / max(fe["rel_l2"], 1e-300)
    line = "%-28s tensor %.3e  worst frame %.3e  localisation %.2f" % (label, fe["rel_l2"], fe["worst"], loc)
    print(line)
    _REPORT.append(line)
    assert fe["rel_l2"] < TENSOR_BOUND and fe["worst"] < FRAME_BOUND and loc < loc_bound, pm.describe(label, got[rows], want[rows], n)


@pytest.mark.parametrize("with_g", [True, False], ids=["g", "no_g"])
@pytest.mark.parametrize("name", list(qc.CASES))
def test_every_probe_and_output(module, loc_bound, weights, name, with_g, monkeypatch):
    lengths = qc.CASES[name][1]
    eng, outs, mask = _run(module, name, with_g, True, monkeypatch)
    assert eng.stats()[0] == N_LAUNCH
    ref, z, m, logs = qc.case_reference(name, with_g, torch.float32)
    tag = "%s/%s " % (name, "g" if with_g else "-")
    got = {k: eng.probe(k) for k in qc.probe_names()}
    for k in qc.probe_names():
        _check(tag + k, got[k], ref[k], lengths, loc_bound)
    g = qc.make_inputs(name)[2] if with_g else None
    for i in range(qc.CFG["n_layers"]):
        x_in = got["pre" if i == 0 else "layer%d.x" % (i - 1)].numpy()
        want = qc.acts_in_isolation(weights, i, x_in, lengths, g, emulate=False)
        bound = qc.acts_bound(qc.acts_in_isolation(weights, i, x_in, lengths, g, emulate=True), want, lengths)
        worst = qc.acts_errors(got["layer%d.acts" % i].numpy().astype(np.float64), want, lengths)[0]
        line = "%-28s in isolation: worst frame %.3e, bound %.3e" % (tag + "layer%d.acts" % i, worst, bound)
        print(line)
        _REPORT.append(line)
        assert worst < bound, line
    for k, got, want in zip(("z", "m", "logs"), outs, (z, m, logs)):
        _check(tag + k, got.transpose(1, 2), want.transpose(1, 2), lengths, loc_bound)
    assert mask.shape == (len(lengths), 1, qc.CASES[name][0]) and int(mask.sum()) == sum(lengths)
    if os.environ.get("DVITS_PARITY_REPORT") == "1":
        path = os.path.join(os.path.dirname(__file__), "..", "profiles", "parity_localisation_qenc_hip.txt")
        with open(path, "w") as f:
            f.write("native posterior encoder vs the float32 torch reference, valid frames (tests/test_gpu_qenc_layerwise.py)\n"
                    "localisation bound %.2f = 3 x the reference's own largest ratio\n" % loc_bound + "\n".join(_REPORT) + "\n")


def test_production_plan_matches_keep_mode_and_repeats(module, monkeypatch):
    _, kept, _ = _run(module, "ragged", True, True, monkeypatch)
    kept = [t.clone() for t in kept]
    eng, a, _ = _run(module, "ragged", True, False, monkeypatch)
    assert eng.stats()[0] == N_LAUNCH
    a = [t.clone() for t in a]
    _, b, _ = _run(module, "ragged", True, False, monkeypatch)
    for x, y, k in zip(a, b, kept):
        assert torch.equal(x, y) and torch.equal(x, k)
    with pytest.raises(RuntimeError, match="DVITS_KEEP_INTERMEDIATES"):
        eng.probe("pre")


def test_replacing_one_utterance_leaves_the_others(module, monkeypatch):
    monkeypatch.setenv("DVITS_KEEP_INTERMEDIATES", "0")
    module.hip_engine()._prepared = None
    y, lengths, g, noise = qc.make_inputs("ragged")
    base = module(_dev(y), _dev(lengths), _dev(g), noise=_dev(noise))[:3]
    base = [t.clone() for t in base]
    y2, g2 = y.copy(), g.copy()
    y2[1], g2[1] = -2.0 * y[1], g[1][::-1]
    other = module(_dev(y2), _dev(lengths), _dev(g2), noise=_dev(noise))[:3]
    for x, o in zip(base, other):
        for b in (0, 2):
            assert torch.equal(x[b, :, :lengths[b]], o[b, :, :lengths[b]])
        assert not torch.equal(x[1], o[1])


def test_graph_replay_equals_eager(module, monkeypatch):
    monkeypatch.setenv("DVITS_KEEP_INTERMEDIATES", "0")
    module.hip_engine()._prepared = None
    y, lengths, g, noise = (_dev(a) for a in qc.make_inputs("two_bm_plus_1"))
    eager = [t.clone() for t in module(y, lengths, g, noise=noise)[:3]]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
        out = module.hip_engine().forward(y, lengths, g, noise)
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for e, r in zip(eager, out):
        assert torch.equal(e, r)
