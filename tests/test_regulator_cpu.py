"""CPU: the length regulator's fp64 gather-form restatement (tests/regulator_cases.py) against the mirror's torch branch
(generate_path + matmul, float32) on every case and against the reference's own frame counts; planted faults in the restatement
under the comparison the GPU test applies to the kernels; and the Python surface of `prior_backend`."""
import numpy as np
import pytest
import torch

import regulator_cases as R
from diff_vits_amd.model3 import VITS, generate_path, sequence_mask


def torch_branch(logw, x_mask, m_p, logs_p, noise, length_scale, noise_scale):
    """Today's expression of VITS.infer_from_encoder between `dp` and `o_proj`, copied: (y_len, m_p', logs_p', z_p)."""
    w = torch.exp(logw) * x_mask * length_scale
    w_ceil = torch.ceil(w)
    y_len = torch.clamp_min(torch.sum(w_ceil, [1, 2]), 1).long()
    y_mask = torch.unsqueeze(sequence_mask(y_len, None), 1).to(x_mask.dtype)
    attn = generate_path(w_ceil, torch.unsqueeze(x_mask, 2) * torch.unsqueeze(y_mask, -1))
    m_p = torch.matmul(attn.squeeze(1), m_p.transpose(1, 2)).transpose(1, 2)
    logs_p = torch.matmul(attn.squeeze(1), logs_p.transpose(1, 2)).transpose(1, 2)
    eps = noise.to(m_p)
    z_p = m_p + eps * torch.exp(logs_p) * noise_scale
    return y_len, m_p, logs_p, z_p, w_ceil


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_restatement_equals_torch_branch(name):
    c, ref = R.make_case(name), R.reference(name)
    R.assert_margin(c)
    t = lambda a: torch.from_numpy(np.array(a))       # noqa: E731
    x_mask = torch.unsqueeze(sequence_mask(t(c["x_len"]), c["Tx"]), 1).float()
    with torch.no_grad():
        y_len, m, logs, z, w_ceil = torch_branch(t(c["logw"]).unsqueeze(1), x_mask, t(c["m_p"]), t(c["logs_p"]), t(c["noise"]),
                                                 c["length_scale"], c["noise_scale"])
    cum = torch.cumsum(w_ceil[:, 0].long(), 1)
    R.compare(ref, cum=cum.numpy(), y_len=y_len.numpy(), z=z.numpy(), m_exp=m.numpy(), logs_exp=logs.numpy(), label=name)
    # regulate_ref is the same thing in one call
    cum2, y_len2, z2 = R.regulate_ref(c["logw"], c["x_len"], c["m_p"], c["logs_p"], c["noise"], c["length_scale"], c["noise_scale"])
    assert np.array_equal(cum2, ref["cum"]) and np.array_equal(y_len2, ref["y_len"]) and np.array_equal(z2, ref["z"])


def test_cases_cover_what_they_claim():
    tp = {n: R.make_case(n)["Tp"] for n in R.CASES}
    assert (tp["one"], tp["tp255"], tp["tp256"], tp["tp257"], tp["tp2048c128"], tp["longtoken"]) == (1, 255, 256, 257, 2048, 309)
    assert tp["tx1025"] > 2048 and tp["ls0"] == 1
    assert R.reference("allzero")["y_len"][1] == 1 and (R.reference("allzero")["tok"][1] == -1).all()
    assert (R.reference("ls0")["tok"] == -1).all()
    z = R.reference("zeros")
    assert z["tok"][0, 0] == 2 and 7 not in z["tok"][0] and 19 not in z["tok"][0] and z["y_len"][0] == z["cum"][0, 18]
    assert (R.reference("ragged")["tok"][2] <= 0).all() and (R.reference("ragged")["tok"][2] == -1).any()


def test_restatement_reproduces_reference_frame_counts(gold):
    g = gold("prior_infer.npz")
    logw = g["logw"].reshape(g["logw"].shape[0], -1)
    assert not R.margin_violations(logw, g["x_lengths"], 1.0).any()
    _, y_len = R.durations_ref(logw, g["x_lengths"], 1.0)
    assert np.array_equal(y_len, g["y_len_out"])


# ---- planted faults: each is a wrong token map or a wrong sample put through the restatement's own arithmetic -------------------
def _tok_exclusive_boundary(cum, x_len, Tp):
    """first j with cum[j] >= t: frame t = cum[j] stays with token j instead of moving on."""
    tok = np.full((cum.shape[0], Tp), -1, dtype=np.int64)
    for b, n in enumerate(x_len):
        j = np.searchsorted(cum[b, :n], np.arange(Tp), side="left")
        tok[b] = np.where(j < n, j, -1)
    return tok


def _tok_zero_duration_kept(cum, x_len, Tp):
    """the FIRST token whose start is the largest start <= t: of tokens that start together, the zero-duration one wins."""
    tok = np.full((cum.shape[0], Tp), -1, dtype=np.int64)
    for b, n in enumerate(x_len):
        start = np.concatenate([[0], cum[b, :n - 1]]) if n > 0 else np.zeros(0, dtype=np.int64)
        for t in range(min(Tp, int(cum[b, n - 1]) if n > 0 else 0)):
            tok[b, t] = int(np.argmax(start == start[start <= t].max()))
    return tok


@pytest.mark.parametrize("fault,name", [("exclusive", "tx65"), ("exclusive", "longtoken"), ("exclusive", "tp257"), ("zero_kept", "zeros"),
                                        ("tokenless_zero", "ragged"), ("tokenless_zero", "allzero"), ("tokenless_zero", "ls0")])
def test_planted_faults_are_detected(fault, name):
    c, ref = R.make_case(name), R.reference(name)
    R.assert_margin(c)
    tok = {"exclusive": _tok_exclusive_boundary, "zero_kept": _tok_zero_duration_kept}.get(fault, R.tokens_ref)(ref["cum"], c["x_len"], c["Tp"])
    z, _ = R.sample_ref(tok, c["m_p"], c["logs_p"], c["noise"], c["noise_scale"])
    if fault == "tokenless_zero":
        z = np.where((tok >= 0)[:, None, :], z, 0.0)
    else:
        assert not np.array_equal(tok, ref["tok"])
    with pytest.raises(AssertionError):
        R.compare(ref, z=z, label="planted " + fault)
    if fault != "tokenless_zero":
        with pytest.raises(AssertionError):
            R.compare(ref, m_exp=R.gather(c["m_p"], tok), label="planted " + fault)
    R.compare(ref, z=ref["z"].astype(np.float32), label="the reference rounded to float32")       # ... which passes


# ---- the Python surface ---------------------------------------------------------------------------------------------------------
def test_unknown_prior_backend_is_refused():
    with pytest.raises(ValueError, match="prior_backend"):
        VITS(backend="torch", prior_backend="bogus")
    from diff_vits_amd import tts_infer
    import inspect
    assert inspect.signature(tts_infer.build_model).parameters["prior_backend"].default is None
    assert inspect.signature(VITS.__init__).parameters["prior_backend"].default is None


def test_hip_prior_refuses_cpu_tensors(gold):
    g = gold("prior_infer.npz")
    m = VITS(backend="torch", prior_backend="hip").eval()
    assert m.prior_backend == "hip" and m.native_regulator_calls == 0
    t = lambda k: torch.from_numpy(g[k])       # noqa: E731
    y = torch.zeros(2, 100, int(g["L"]))
    with pytest.raises(RuntimeError, match="GPU tensors"):
        m.infer_from_encoder(t("enc_x"), t("enc_m_p"), t("enc_logs_p"), t("enc_x_mask"), t("x_lengths"), y, t("y_lengths"))
    assert m.native_regulator_calls == 0


def test_default_is_todays_expression_bit_for_bit(gold):
    from test_prompt_cpu import prior_case, vits_mirror
    from diff_vits_amd import synth
    g, sd, y = prior_case(gold)
    m = vits_mirror(g, sd, "torch")
    assert m.prior_backend is None
    t = lambda k: torch.from_numpy(g[k])       # noqa: E731
    noise = torch.from_numpy(synth.normal(1234, "prior.noise", tuple(g["z"].shape)))
    yt = torch.from_numpy(y)
    with torch.no_grad():
        z, _, y_len = m.infer_from_encoder(t("enc_x"), t("enc_m_p"), t("enc_logs_p"), t("enc_x_mask"), t("x_lengths"), yt, t("y_lengths"),
                                           noise=noise, noise_scale=0.5)
        gg = m.ref_enc(yt.transpose(1, 2)).unsqueeze(-1)
        logw = m.dp(t("enc_x"), t("x_lengths"), yt, t("y_lengths"))
        y_len2, _, _, z_p, _ = torch_branch(logw, t("enc_x_mask"), t("enc_m_p"), t("enc_logs_p"), noise, 1, 0.5)
        z2 = m.o_proj(z_p, y_len2, gg)
    assert torch.equal(y_len, y_len2) and torch.equal(z, z2)
    assert m.native_regulator_calls == 0
