"""The posterior encoder's opt-in native backend, the parts that need no GPU: the switches validate their values, backend=None is
today's path bit for bit with today's state-dict keys, backend='hip' refuses CPU tensors (never a fall-back), and the float32
reference of tests/qenc_cases.py stays inside a third of the GPU tests' bounds against float64 on every case
(DVITS_PARITY_REPORT=1 writes profiles/parity_localisation_qenc_ref.txt)."""
import os

import numpy as np
import pytest
import torch

import parity_metrics as pm
import qenc_cases as qc
from diff_vits_amd import tts_infer
from diff_vits_amd.model3 import VITS, WN, PosteriorEncoder, sequence_mask


def test_backend_values_are_validated():
    for bad in ("torch", "cuda", "", 0):
        with pytest.raises(ValueError, match="backend"):
            PosteriorEncoder(100, 128, 256, 5, 1, 16, 256, backend=bad)
        with pytest.raises(ValueError, match="posterior_backend"):
            VITS(11, 513, aligner=True, posterior_backend=bad)
    assert PosteriorEncoder(100, 16, 32, 5, 1, 2, 0, backend="hip").backend == "hip"
    v = VITS(11, 513, aligner=True, posterior_backend="hip")
    assert v.enc_q.backend == "hip" and v.native_posterior_calls == 0
    assert VITS(11, 513, aligner=True).enc_q.backend is None and VITS(11, 513).native_posterior_calls == 0
    with pytest.raises(ValueError, match="posterior_backend"):
        tts_infer.build_model({"data": {"window_size": 1024}, "vits": {}}, 11, posterior_backend="torch")


def test_none_path_is_todays_path_bit_for_bit():
    sd = qc.make_weights()
    m = qc.make_module(sd)
    assert set(m.state_dict()) == set(sd) == set(qc.make_module(sd, backend="hip").state_dict())
    y, lengths, g, noise = (torch.from_numpy(a) for a in qc.make_inputs("ragged"))
    with torch.no_grad():
        z, mq, logs, mask = m(y, lengths, g.unsqueeze(-1), noise=noise)
        # the parent's forward, restated from its three lines
        x_mask = torch.unsqueeze(sequence_mask(lengths, y.size(2)), 1).to(y.dtype)
        h = WN.forward(m.enc, m.pre(y) * x_mask, x_mask, g=g.unsqueeze(-1))
        m2, logs2 = torch.split(m.proj(h) * x_mask, m.out_channels, dim=1)
        z2 = (m2 + noise * torch.exp(logs2)) * x_mask
    assert torch.equal(z, z2) and torch.equal(mq, m2) and torch.equal(logs, logs2) and torch.equal(mask, x_mask)
    assert m.native_calls == 0


def test_hip_backend_refuses_cpu_tensors():
    m = qc.make_module(backend="hip")
    y, lengths, g, noise = (torch.from_numpy(a) for a in qc.make_inputs("t5"))
    with pytest.raises(RuntimeError, match="needs GPU tensors; got x on cpu"):
        m(y, lengths, g.unsqueeze(-1), noise=noise)
    assert m.native_calls == 0


def test_float32_reference_stays_inside_a_third_of_the_bounds():
    bound, lines, worst_tensor, worst_frame = qc.localisation_bound()
    print("largest localisation ratio of the float32 reference: %.2f" % (bound / 3))
    if os.environ.get("DVITS_PARITY_REPORT") == "1":
        path = os.path.join(os.path.dirname(__file__), "..", "profiles", "parity_localisation_qenc_ref.txt")
        with open(path, "w") as f:
            f.write("float32 torch PosteriorEncoder vs the same in float64, valid frames, every case of tests/qenc_cases.py\n"
                    "largest localisation ratio %.2f; the GPU bound is 3 x this = %.2f (qenc_cases.localisation_bound)\n"
                    % (bound / 3, bound) + "\n".join(lines) + "\n")
    assert worst_tensor < TENSOR_BOUND / 3 and worst_frame < pm.FRAME_BOUND / 3 and np.isfinite(bound)


# ---- the host emulation of the kernel's arithmetic: the acts bound, and the faults the criteria must see ------------------------
TENSOR_BOUND = 2e-4
FAULT_CASES = ("batch4",)       # five tiles per utterance, a full-length utterance in front of another, three ragged ends


_SD = []


def _weights():
    if not _SD:
        _SD.append(qc.make_weights())
    return _SD[0]


def _figures(got, want, lengths):
    rows = qc.valid_rows(lengths)
    n = [lengths[b] for b in rows]
    sv = pm.split_valid(np.asarray(got)[rows], np.asarray(want)[rows], n)
    fe = pm.frame_errors(sv["got"], sv["want"])
    return fe["rel_l2"], fe["worst"], fe["worst"] / max(fe["rel_l2"], 1e-300)


def _pairs(run, ref):
    """(name, got, want) channels-last for every probe and z / m / logs, in schedule order."""
    out = [(k, run[0][k], ref[0][k].numpy()) for k in qc.probe_names()]
    return out + [(k, np.swapaxes(a, 1, 2), b.transpose(1, 2).numpy()) for k, a, b in zip(("z", "m", "logs"), run[1:], ref[1:])]


def _first_seen(sd, name, fault, loc_bound):
    """Run the emulation of case `name` (with g) with `fault` planted; -> {criterion: first probe that exceeds it} under the GPU
    test's criteria: whole tensor, every frame, localisation (against the float32 reference), and for layerN.acts the bound in
    isolation (against the float64 activations of the run's own layer input)."""
    y, lengths, g, noise = qc.make_inputs(name)
    lengths = [int(v) for v in lengths]
    run = qc.emulate_forward(sd, y, lengths, g, noise, emulate=True, fault=fault)
    seen = {}
    for k, got, want in _pairs(run, qc.case_reference(name, True, torch.float32)):
        t, f, loc = _figures(got, want, lengths)
        for crit, bad in (("tensor", t >= TENSOR_BOUND), ("frame", f >= pm.FRAME_BOUND), ("localisation", loc >= loc_bound)):
            if bad:
                seen.setdefault(crit, k)
    L = qc.CFG["n_layers"]
    for i in (range(L) if fault is None else (0, L - 1)):            # (a planted fault sits in every layer: the first and the last say it)
        x_in = run[0]["pre" if i == 0 else "layer%d.x" % (i - 1)]
        want = qc.acts_in_isolation(sd, i, x_in, lengths, g, emulate=False)
        bound = qc.acts_bound(qc.acts_in_isolation(sd, i, x_in, lengths, g, emulate=True), want, lengths)
        if qc.acts_errors(run[0]["layer%d.acts" % i], want, lengths)[0] >= bound:
            seen.setdefault("acts in isolation", "layer%d.acts" % i)
            break
    return seen


def test_restatement_is_the_module_and_the_emulation_stays_inside_the_bounds():
    sd = _weights()
    loc_bound = qc.localisation_bound()[0]
    y, lengths, g, noise = qc.make_inputs("ragged")
    exact = qc.emulate_forward(sd, y, lengths, g, noise, emulate=False)
    for k, got, want in _pairs(exact, qc.case_reference("ragged", True, torch.float64)):
        assert np.abs(got - want).max() < 1e-11, k
    for name in FAULT_CASES:
        assert _first_seen(sd, name, None, loc_bound) == {}, name


def test_every_planted_fault_is_seen_and_the_acts_bound_is_derived():
    sd = _weights()
    loc_bound = qc.localisation_bound()[0]
    lines = ["host emulation of k_wn_layer's arithmetic (tests/qenc_cases.py emulate_forward), cases %s with g" % ", ".join(FAULT_CASES),
             "criteria: whole tensor < %.0e, every frame < %.0e, localisation < %.2f against the float32 reference; layerN.acts in "
             "isolation < acts_bound" % (TENSOR_BOUND, pm.FRAME_BOUND, loc_bound), ""]
    # the acts bound per layer, on the reference's own layer inputs (the GPU test derives it the same way from the engine's)
    for name in FAULT_CASES:
        y, lengths, g, noise = qc.make_inputs(name)
        lengths = [int(v) for v in lengths]
        ref = qc.case_reference(name, True, torch.float32)[0]
        for i in range(qc.CFG["n_layers"]):
            x_in = ref["pre" if i == 0 else "layer%d.x" % (i - 1)].numpy()
            want = qc.acts_in_isolation(sd, i, x_in, lengths, g, emulate=False)
            emu = qc.acts_in_isolation(sd, i, x_in, lengths, g, emulate=True)
            worst, share = qc.acts_errors(emu, want, lengths)
            bound = qc.acts_bound(emu, want, lengths)
            lines.append("%s layer%d.acts in isolation: emulation worst frame %.3e, WN_ACT_ERR share %.3e, bound %.3e" % (name, i, worst, share, bound))
            assert worst < bound < 1e-4, lines[-1]                  # far below the generic per-frame bound of 1e-3
    lines.append("")
    for fault in qc.FAULTS:
        caught = False
        for name in FAULT_CASES:
            seen = _first_seen(sd, name, fault, loc_bound)
            caught = caught or bool(seen)
            lines.append("%-24s %-8s %s" % (fault, name, "; ".join("%s first at %s" % (c, k) for c, k in seen.items()) or "not seen"))
        assert caught, lines[-2:]
    print("\n".join(lines))
    if os.environ.get("DVITS_PARITY_REPORT") == "1":
        with open(os.path.join(os.path.dirname(__file__), "..", "profiles", "qenc_reference.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
