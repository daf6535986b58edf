"""GPU: every sub-layer of the native text encoder (dv_tenc_*, csrc/tenc.hip) against the oracle's intermediates
(oracle.text_enc_ref on the CPU in fp32, tests/tenc_cases.py), frame by frame, on ragged batches, with and without the speaker
vector: the probes emb, layerN.attn, layerN.ln1, layerN.ffn1, layerN, proj and the outputs x, m, logs.

Criteria per tensor on the VALID frames (tests/parity_metrics.py): whole-tensor relative L2 < 2e-4, EVERY frame < FRAME_BOUND =
1e-3, localisation ratio < TENC_LOCALISATION_BOUND = 3 x 1.79 (three times the largest ratio the reference side shows against
itself in fp64 on these very cases: profiles/parity_localisation_tenc_ref.txt), at most 1 % of the valid frames on the norm
floor, every padding frame exactly zero.  DVITS_PARITY_REPORT=<file> appends every tensor's figures to that file (the way to
make profiles/parity_localisation_tenc_hip.txt).  Without a tolerance: two forwards are identical, utterances are independent,
a forward replayed from a captured graph equals the eager one."""
import os

import numpy as np
import pytest
import torch

import tenc_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sd():
    return tc.state_dict()


def _model(sd):
    from diff_vits_amd.model3 import TextEncoder
    m = TextEncoder(backend="hip", **tc.KW).eval()
    m.load_state_dict(sd)
    return m.cuda()


def _run(m, ids, ln, tone, lang, g):
    with torch.no_grad():
        x, mm, logs, mask = m(ids.cuda(), ln.cuda(), tone.cuda(), lang.cuda(), None if g is None else g.cuda())
    torch.cuda.synchronize()
    return [v.cpu() for v in (x, mm, logs, mask)]


@pytest.mark.parametrize("with_g", [True, False], ids=["g", "no-g"])
@pytest.mark.parametrize("name,B,T,lengths", tc.CASES, ids=tc.IDS)
def test_every_sublayer_per_frame(sd, name, B, T, lengths, with_g):
    ids, tone, lang, ln, g = tc.inputs(B, T, lengths)
    g = g if with_g else None
    with torch.no_grad():
        (x_ref, m_ref, logs_ref), ref = tc.oracle_probes(sd, ids, ln, tone, lang, g)
    names = tc.probe_names()
    got, outs = {}, []
    for keep in (True, False):
        if keep:
            os.environ["DVITS_KEEP_INTERMEDIATES"] = "1"
        try:
            m = _model(sd)
            out = _run(m, ids, ln, tone, lang, g)
            eng = m.hip_engine()
            assert eng.stats()[0] == 1 + 2 + 7 * tc.KW["n_layers"] + 2, eng.stats()
            if keep:
                for n in names:
                    got[n] = eng.probe(n)
            else:
                with pytest.raises(RuntimeError):
                    eng.probe("emb")
            out2 = _run(m, ids, ln, tone, lang, g)
            assert all(torch.equal(a, b) for a, b in zip(out, out2)), "two forwards of the same input differ"
            outs.append(out)
            del m, eng
        finally:
            os.environ.pop("DVITS_KEEP_INTERMEDIATES", None)
    report, failures = [], []
    for n in names:
        assert tuple(got[n].shape) == tuple(ref[n].shape), (n, tuple(got[n].shape), tuple(ref[n].shape))
        tc.check(n, got[n], ref[n], lengths, report, failures)
    for tag, out in (("probes", outs[0]), ("default", outs[1])):
        for k, v, w in (("x", out[0], x_ref), ("m", out[1], m_ref), ("logs", out[2], logs_ref)):
            tc.check("%s (%s)" % (k, tag), v.transpose(1, 2), w, lengths, report, failures)
        assert torch.equal(out[3][:, 0] > 0, torch.arange(T)[None, :] < ln[:, None])
    path = os.environ.get("DVITS_PARITY_REPORT")
    if path:
        with open(path, "a") as f:
            f.write("# %s B=%d T=%d lengths=%s %s\n%s\n" % (name, B, T, ",".join(str(v) for v in lengths),
                                                           "with g" if with_g else "without g", "\n".join(report)))
    print("\n".join(report))
    assert not failures, "%d of %d tensors fail; in schedule order:\n%s" % (len(failures), len(report), "\n".join(failures[:6]))


def test_utterances_are_independent_bitwise(sd):
    """B = 3 / T = 75 (75, 40, 9) on ONE prepared engine: utterance 1 gets other ids and another length; every valid frame of the
    other two must come out bit-identical and their padding stays zero.  The rows of all utterances are neighbours in the flat
    [B * T, C] row space: the k = 3 taps, the GEMM row tiles and the attention's key range must not reach across."""
    name, B, T, lengths = tc.case("3x75")
    ids, tone, lang, ln, g = tc.inputs(B, T, lengths)
    ids_o, tone_o, lang_o, _, g_o = tc.inputs(B, T, lengths, tag="te.other")
    m = _model(sd)
    y1 = _run(m, ids, ln, tone, lang, g)
    prepared = m.hip_engine()._prepared
    for new_len in (75, 41, 1):
        ids2, tone2, lang2, ln2, g2 = ids.clone(), tone.clone(), lang.clone(), ln.clone(), g.clone()
        ids2[1], tone2[1], lang2[1], g2[1], ln2[1] = ids_o[1], tone_o[1], lang_o[1], g_o[1], new_len
        y2 = _run(m, ids2, ln2, tone2, lang2, g2)
        assert m.hip_engine()._prepared == prepared and prepared is not None
        for a, b in zip(y1[:3], y2[:3]):
            assert not torch.equal(a[1], b[1])
            assert bool((b[1, :, new_len:] == 0).all())
            for u in (0, 2):
                n = lengths[u]
                assert bool((b[u, :, n:] == 0).all()), "padding of utterance %d is not zero" % u
                diff = np.flatnonzero((a[u, :, :n] != b[u, :, :n]).any(0).numpy())
                assert diff.size == 0, "utterance %d: %d of %d valid frames differ, first %d, last %d (utterance 1: %d -> %d tokens)" % (
                    u, diff.size, n, diff[0], diff[-1], lengths[1], new_len)


def test_graph_replay_equals_eager(sd):
    """dv_tenc_forward allocates nothing and never waits for the device: captured by torch.cuda.graph and replayed, it writes what
    the eager call writes."""
    name, B, T, lengths = tc.case("3x75")
    ids, tone, lang, ln, g = (v.cuda() for v in tc.inputs(B, T, lengths))
    m = _model(sd)
    eng = m.hip_engine()
    with torch.no_grad():
        eager = [v.clone() for v in eng.forward(ids, ln, tone, lang, g)]              # validates, syncs weights, prepares
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = eng.forward(ids, ln, tone, lang, g, validate=False)
        for v in captured:
            v.zero_()
        graph.replay()
        torch.cuda.synchronize()
    for a, b in zip(eager, captured):
        assert torch.equal(a, b)
