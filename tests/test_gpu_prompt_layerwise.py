"""GPU: every sub-layer of the native prompt encoder (dv_penc_*, Builder::build_penc) against the oracle's intermediates, frame
by frame, at the shapes it really runs at: the denoiser's conditioning (flavour D, B = 8 / 16 at L = 256) and the prior's o_proj
over frames (flavour P, T up to 2048) - tests/prompt_cases.py.  tests/test_gpu_prompt.py compares the encoder at M = 80 and
M = 225 rows with one whole-tensor number; the nine-tap feed-forward over two K-segments, the rowmask and relu split-plane
epilogues, k_prompt_pre, k_ln_affine and the converting k_attention with a per-call key bias run nowhere in the denoiser, so
tests/test_gpu_layerwise.py does not vouch for them.

Criteria per probe and for the output, on the VALID frames (tests/parity_metrics.py): whole-tensor relative L2 < 2e-4 (the bar of
tests/test_gpu_prompt.py), EVERY frame < FRAME_BOUND = 1e-3, localisation ratio < PENC_LOCALISATION_BOUND (3 x the largest ratio
the reference side shows against itself in fp64 on these very cases, profiles/parity_localisation_penc_ref.txt), at most 1 % of
the valid frames on the norm floor, and every padding frame exactly zero (layerN.ffn1 excepted: neither side masks it).
DVITS_PARITY_REPORT=<file> appends every probe's figures to that file (the way to make profiles/parity_localisation_penc_hip.txt)."""
import os

import numpy as np
import pytest
import torch

import prompt_cases as pc
from conftest import rel_l2
from parity_metrics import prompt_oracle_probes, prompt_probe_names

pytestmark = pytest.mark.gpu


def _model(flavour, sd):
    from diff_vits_amd.model3 import PromptEncoder
    m = PromptEncoder(p_dropout=0.2, backend="hip", **pc.FLAVOURS[flavour][0]).eval()
    m.load_state_dict(sd)
    return m.cuda()


def _run(m, prompt, lengths):
    with torch.no_grad():
        y = m.encode_channels_last(prompt.cuda(), lengths.cuda())
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize("name,flavour,B,L,lengths", pc.CASES, ids=pc.IDS)
def test_every_sublayer_per_frame(gold, name, flavour, B, L, lengths):
    """One forward with DVITS_KEEP_INTERMEDIATES=1: `pre`, every layer's `.attn` / `.ffn1` / output, `out_proj` (dv_penc_probe) and
    the output against oracle.prompt_ref in fp32 on the CPU, each under the criteria of the module docstring; a failure names the
    probe, the utterance, the frame and the worst 32 x C / 64 x 64 / 128 x 128 block.  The output of a second engine prepared
    without the probes (the arena then reuses its buffers) goes through the same criteria.  Without a tolerance: the launch
    count, and two forwards of one input are bit-identical.  The golden case (D, B = 2, L = 40) also compares the five probes the
    goldens carry, captured from the reference itself, through the same path."""
    n_layers = pc.FLAVOURS[flavour][0]["n_layers"]
    sd = pc.state_dict(flavour)
    prompt, ln = pc.inputs(flavour, B, L, lengths)
    with torch.no_grad():
        y_ref, ref = prompt_oracle_probes(sd, prompt, ln, n_layers)
    names = prompt_probe_names(n_layers)

    got, ys = {}, []
    for keep in (True, False):
        if keep:
            os.environ["DVITS_KEEP_INTERMEDIATES"] = "1"
        try:
            m = _model(flavour, sd)
            y = _run(m, prompt, ln)
            eng = m.hip_engine()
            assert eng.stats()[0] == 2 + 1 + 6 * n_layers + 2, eng.stats()
            if keep:
                for n in names:
                    try:
                        got[n] = eng.probe(n)
                    except RuntimeError as e:
                        raise AssertionError("the engine registers no probe %s: %s" % (n, e))
            else:
                with pytest.raises(RuntimeError):
                    eng.probe("pre")
            y2 = _run(m, prompt, ln)
            assert torch.equal(y, y2), "two forwards of the same input differ (%s)" % ("with probes" if keep else "default")
            ys.append(y)
            del m, eng
        finally:
            os.environ.pop("DVITS_KEEP_INTERMEDIATES", None)

    report, failures = [], []
    for n in names:
        assert tuple(got[n].shape) == tuple(ref[n].shape), (n, tuple(got[n].shape), tuple(ref[n].shape))
        pc.check(n, got[n], ref[n], lengths, report, failures, masked=not n.endswith(".ffn1"))
    pc.check("y (probes)", ys[0], y_ref, lengths, report, failures)
    pc.check("y (default)", ys[1], y_ref, lengths, report, failures)
    if name == "D-2x40":
        g = gold("prompt_cfg.npz")
        assert list(g["lengths"]) == lengths and int(g["L"]) == L
        for k in ["pre"] + ["layer%d" % i for i in range(n_layers)]:
            assert rel_l2(ref[k].numpy(), g["probe_" + k]) < 1e-6                    # (the oracle is the reference here)
            pc.check("golden " + k, got[k], torch.from_numpy(g["probe_" + k]), lengths, report, failures)
        pc.check("golden y", ys[0], torch.from_numpy(g["enc"]).permute(0, 2, 1), lengths, report, failures)
    path = os.environ.get("DVITS_PARITY_REPORT")
    if path:
        with open(path, "a") as f:
            f.write("# %s B=%d L=%d lengths=%s\n%s\n" % (name, B, L, ",".join(str(v) for v in lengths), "\n".join(report)))
    print("\n".join(report))
    assert not failures, "%d of %d tensors fail; in schedule order:\n%s" % (len(failures), len(report), "\n".join(failures[:6]))


def test_utterances_are_independent_bitwise():
    """B = 8 / L = 256 on ONE prepared engine: utterance 3 gets another prompt and another length; every valid frame of the other
    seven utterances must come out bit-identical (and their padding stays zero).  The rows of all utterances are neighbours in
    the flat [B * L, C] row space: the nine-tap halo of the feed-forward (taps at -3..+4 rows), the GEMM row tiles and the
    attention's key bias must not reach across.  The message lists the utterances that differ with their first and last differing
    frame, and says for every utterance boundary whether the frame just before it (the last valid one of the utterance in
    front) and just after it (frame 0) differ."""
    name, flavour, B, L, lengths = pc.case("D-8x256")
    sd = pc.state_dict(flavour)
    prompt, ln = pc.inputs(flavour, B, L, lengths)
    other, _ = pc.inputs(flavour, B, L, lengths, tag="pe.prompt.other")
    m = _model(flavour, sd)
    y1 = _run(m, prompt, ln)
    prepared = m.hip_engine()._prepared
    for new_len in (77, 256, 1):
        prompt2, ln2 = prompt.clone(), ln.clone()
        prompt2[3] = other[3]
        ln2[3] = new_len
        y2 = _run(m, prompt2, ln2)
        assert m.hip_engine()._prepared == prepared and prepared is not None     # the same prepared schedule
        assert not torch.equal(y1[3], y2[3])
        assert bool((y2[3, new_len:] == 0).all())
        bad = []
        for b in range(B):
            if b == 3:
                continue
            n = lengths[b]
            assert bool((y2[b, n:] == 0).all()), "padding of utterance %d is not zero" % b
            diff = np.flatnonzero((y1[b, :n] != y2[b, :n]).any(-1).numpy())
            if diff.size:
                bad.append("utterance %d: %d of %d valid frames differ, first %d, last %d" % (b, diff.size, n, diff[0], diff[-1]))
        if bad:
            for b in range(1, B):
                before, after = (y1[b - 1, lengths[b - 1] - 1] != y2[b - 1, lengths[b - 1] - 1]).any(), (y1[b, 0] != y2[b, 0]).any()
                bad.append("boundary %d|%d: frame %d of utterance %d %s, frame 0 of utterance %d %s" %
                           (b - 1, b, lengths[b - 1] - 1, b - 1, "DIFFERS" if before else "same", b, "DIFFERS" if after else "same"))
        assert not bad, "utterance 3 replaced (length %d -> %d):\n%s" % (lengths[3], new_len, "\n".join(bad))
