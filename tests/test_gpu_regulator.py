"""GPU: the native length regulator (dv_op_regulate_lengths / dv_op_regulate_sample, csrc/kernels_regulate.hip) alone against the
fp64 gather-form restatement of tests/regulator_cases.py - cum and y_len identical, the gathered statistics bit-equal, z within
4 * 2^-23 * (|m| + |noise * exp(logs) * noise_scale|) per element - on cases that each cross one boundary of the kernels (wave, chunk
carry, LDS / global search, workgroup of 256 frames, ragged lengths, zero durations, an utterance of zero durations, length_scale 0,
noise_scale 0); an invalid utterance as a VALUE (y_len = -1, ValueError from VITS), run-to-run and row-to-row independence, graph
capture, and VITS(prior_backend='hip') on the reference's prior fixture."""
import numpy as np
import pytest
import torch

import regulator_cases as R
from conftest import rel_l2

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda().contiguous()


def run_lengths(logw, x_len, length_scale):
    """-> (cum int32 [B, Tx], y_len int64 [B]) device tensors"""
    from diff_vits_amd import _lib
    B, Tx = logw.shape
    cum = torch.full((B, Tx), -7, dtype=torch.int32, device="cuda")
    y_len = torch.full((B,), -7, dtype=torch.int64, device="cuda")
    _lib.check(_lib.lib().dv_op_regulate_lengths(_lib.ptr(logw), _lib.ptr(x_len), B, Tx, float(length_scale), _lib.ptr(cum),
                                                 _lib.ptr(y_len), _lib.stream_ptr()), "dv_op_regulate_lengths")
    return cum, y_len


def run_sample(m_p, logs_p, cum, x_len, noise, noise_scale, expanded=True):
    """-> (z, m_exp, logs_exp) device tensors [B, C, Tp], NaN where the kernel wrote nothing"""
    from diff_vits_amd import _lib
    B, C, Tx = m_p.shape
    Tp = noise.shape[2]
    z, me, le = (torch.full((B, C, Tp), float("nan"), device="cuda") for _ in range(3))
    _lib.check(_lib.lib().dv_op_regulate_sample(_lib.ptr(m_p), _lib.ptr(logs_p), _lib.ptr(cum), _lib.ptr(x_len), _lib.ptr(noise),
                                                float(noise_scale), B, C, Tx, Tp, _lib.ptr(z), _lib.ptr(me) if expanded else None,
                                                _lib.ptr(le) if expanded else None, _lib.stream_ptr()), "dv_op_regulate_sample")
    return z, me, le


def run_case(c):
    logw, x_len, m_p, logs_p, noise = (_dev(c[k]) for k in ("logw", "x_len", "m_p", "logs_p", "noise"))
    cum, y_len = run_lengths(logw, x_len, c["length_scale"])
    z, me, le = run_sample(m_p, logs_p, cum, x_len, noise, c["noise_scale"])
    torch.cuda.synchronize()
    return cum, y_len, z, me, le


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_operator_against_restatement(name):
    c, ref = R.make_case(name), R.reference(name)
    R.assert_margin(c)
    cum, y_len, z, me, le = (a.cpu().numpy() for a in run_case(c))
    R.compare(ref, cum=cum, y_len=y_len, z=z, m_exp=me, logs_exp=le, label=name)


def test_two_runs_are_bitwise_equal_and_optional_outputs_are_optional():
    c = R.make_case("ragged")
    a, b = run_case(c), run_case(c)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    logw, x_len, m_p, logs_p, noise = (_dev(c[k]) for k in ("logw", "x_len", "m_p", "logs_p", "noise"))
    z, me, le = run_sample(m_p, logs_p, a[0], x_len, noise, c["noise_scale"], expanded=False)
    torch.cuda.synchronize()
    assert torch.equal(z, a[2]) and bool(torch.isnan(me).all()) and bool(torch.isnan(le).all())


def test_invalid_utterance_is_a_value_and_leaves_the_other_rows_alone():
    """logw = 40 (exp = 2.4e17 > 2^24) on utterance 1 of 3: y_len[1] = -1, rows 0 and 2 as without it; +inf, NaN and a token behind
    the utterance's length likewise / not at all."""
    c, ref = R.make_case("ragged"), R.reference("ragged")
    x_len = _dev(c["x_len"])
    for value, j, hit in ((40.0, 5, True), (float("inf"), 0, True), (float("nan"), 61, True), (40.0, 63, False)):
        logw = np.array(c["logw"])
        logw[1, j] = value                                   # x_len[1] = 62: token 63 is padding, its duration is masked
        cum, y_len = run_lengths(_dev(logw), x_len, c["length_scale"])
        torch.cuda.synchronize()
        cum, y_len = cum.cpu().numpy(), y_len.cpu().numpy()
        want = ref["y_len"].copy()
        if hit:
            want[1] = -1
        assert np.array_equal(y_len, want), (value, j, y_len)
        rows = [0, 2] if hit else [0, 1, 2]
        assert np.array_equal(cum[rows], ref["cum"][rows])
    # the sample kernel on such a row stays inside the row: the others are what they were
    logw = np.array(c["logw"])
    logw[1, 5] = 40.0
    cum, _ = run_lengths(_dev(logw), x_len, c["length_scale"])
    z, _, _ = run_sample(_dev(c["m_p"]), _dev(c["logs_p"]), cum, x_len, _dev(c["noise"]), c["noise_scale"])
    torch.cuda.synchronize()
    z = z.cpu().numpy()
    assert np.isfinite(z).all() and (np.abs(z[[0, 2]] - ref["z"][[0, 2]]) <= ref["bound"][[0, 2]]).all()


def test_replacing_one_utterance_leaves_the_others_bitwise_unchanged():
    c = R.make_case("ragged")
    cum0, y0, z0, _, _ = run_case(c)
    logw = np.array(c["logw"])
    logw[1] = logw[1, ::-1] - 0.4                          # other, shorter durations for utterance 1: Tp stays the old maximum
    m_p, logs_p = np.array(c["m_p"]), np.array(c["logs_p"])
    m_p[1], logs_p[1] = m_p[1, ::-1], logs_p[1, ::-1]
    x_len = _dev(c["x_len"])
    cum1, y1 = run_lengths(_dev(logw), x_len, c["length_scale"])
    z1, _, _ = run_sample(_dev(m_p), _dev(logs_p), cum1, x_len, _dev(c["noise"]), c["noise_scale"])
    torch.cuda.synchronize()
    assert not torch.equal(cum1[1], cum0[1]) and int(y1.max()) <= c["Tp"]
    for r in (0, 2):
        assert torch.equal(cum1[r], cum0[r]) and torch.equal(y1[r], y0[r]) and torch.equal(z1[r], z0[r])
    assert not torch.equal(z1[1], z0[1])


def test_both_ops_in_one_graph_replayed_with_new_durations():
    from diff_vits_amd import _lib
    c = R.make_case("ragged")
    B, C, Tx, Tp = c["B"], c["C"], c["Tx"], c["Tp"]
    logws = [np.array(c["logw"]), np.array(c["logw"])[:, ::-1] - 0.3, np.array(c["logw"]) - 0.7]      # none longer than Tp frames
    x_len, m_p, logs_p, noise = (_dev(c[k]) for k in ("x_len", "m_p", "logs_p", "noise"))
    eager = []
    for lw in logws:
        cum, y_len = run_lengths(_dev(lw), x_len, c["length_scale"])
        z, _, _ = run_sample(m_p, logs_p, cum, x_len, noise, c["noise_scale"], expanded=False)
        torch.cuda.synchronize()
        assert int(y_len.max()) <= Tp
        eager.append((cum.clone(), y_len.clone(), z.clone()))
    L = _lib.lib()
    logw = _dev(logws[0])
    cum = torch.zeros((B, Tx), dtype=torch.int32, device="cuda")
    y_len = torch.zeros((B,), dtype=torch.int64, device="cuda")
    z = torch.zeros((B, C, Tp), device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.check(L.dv_op_regulate_lengths(_lib.ptr(logw), _lib.ptr(x_len), B, Tx, float(c["length_scale"]), _lib.ptr(cum), _lib.ptr(y_len),
                                            _lib.stream_ptr()), "dv_op_regulate_lengths")
        _lib.check(L.dv_op_regulate_sample(_lib.ptr(m_p), _lib.ptr(logs_p), _lib.ptr(cum), _lib.ptr(x_len), _lib.ptr(noise),
                                           float(c["noise_scale"]), B, C, Tx, Tp, _lib.ptr(z), None, None, _lib.stream_ptr()),
                   "dv_op_regulate_sample")
    for lw, want in zip(logws[1:], eager[1:]):
        logw.copy_(_dev(lw))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cum, want[0]) and torch.equal(y_len, want[1]) and torch.equal(z, want[2])
    assert not torch.equal(eager[1][2], eager[2][2])


def test_bad_arguments_are_refused_before_a_launch():
    from diff_vits_amd import _lib
    L = _lib.lib()
    f = torch.zeros(16, device="cuda")
    i32 = torch.zeros(16, dtype=torch.int32, device="cuda")
    i64 = torch.ones(1, dtype=torch.int64, device="cuda")
    p, s = _lib.ptr, _lib.stream_ptr()
    assert L.dv_op_regulate_lengths(None, p(i64), 1, 4, 1.0, p(i32), p(i64), s) == -1 and b"null" in L.dv_last_error()
    assert L.dv_op_regulate_lengths(p(f), p(i64), 0, 4, 1.0, p(i32), p(i64), s) == -1
    assert L.dv_op_regulate_lengths(p(f), p(i64), 1, 0, 1.0, p(i32), p(i64), s) == -1 and b"Tx = 0" in L.dv_last_error()
    assert L.dv_op_regulate_lengths(p(f), p(i64), 1, 4, -1.0, p(i32), p(i64), s) == -1 and b"length_scale" in L.dv_last_error()
    assert L.dv_op_regulate_sample(p(f), p(f), p(i32), p(i64), p(f), 1.0, 1, 1, 4, 4, None, None, None, s) == -1
    for dims in ((0, 1, 4, 4), (1, 0, 4, 4), (1, 1, 0, 4), (1, 1, 4, 0)):
        assert L.dv_op_regulate_sample(p(f), p(f), p(i32), p(i64), p(f), 1.0, *dims, p(f), None, None, s) == -1
    torch.cuda.synchronize()


class _FixedDurations(torch.nn.Module):
    def __init__(self, logw):
        super().__init__()
        self.logw = logw

    def forward(self, x, x_lengths, y, y_lengths):
        return self.logw


@pytest.fixture(scope="module")
def prior(gold):
    """VITS(backend='hip', text_encoder_backend='hip', prior_backend='hip') with the fixture's weights, on the GPU."""
    import ast
    from test_prompt_cpu import prior_case
    from diff_vits_amd.model3 import VITS
    g, sd, y = prior_case(gold)
    kw = ast.literal_eval(str(g["vits_kwargs"]))
    m = VITS(int(g["n_vocab"]), 513, n_tones=int(g["n_tones"]), n_languages=int(g["n_languages"]), backend="hip",
             text_encoder_backend="hip", prior_backend="hip", **kw).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return g, y, m.cuda()


def test_product_on_the_prior_fixture(prior):
    """Frame counts equal the reference's, z within 2e-4 of its z (the bound tests/test_gpu_tenc.py applies to the same tensor), the
    native regulator ran once; the torch branch of the same model on the same inputs: identical y_len, z within that bound."""
    from diff_vits_amd import synth
    g, y, m = prior
    noise = torch.from_numpy(synth.normal(1234, "prior.noise", tuple(g["z"].shape))).cuda()
    args = [_dev(a) for a in (g["text"], g["x_lengths"], y, g["y_lengths"], g["tone"], g["language"])]
    assert m.prior_backend == "hip"
    before = m.native_regulator_calls
    z, _ = m.infer(*args, noise=noise)
    assert m.native_regulator_calls == before + 1
    assert z.shape == g["z"].shape
    frames = (z.abs().sum(1) != 0).sum(1).cpu().numpy()
    assert np.array_equal(frames, g["y_len_out"]), (frames, g["y_len_out"])
    r = rel_l2(z.cpu().numpy(), g["z"])
    print("z native regulator vs reference: rel_l2 %.3e" % r)
    assert r < 2e-4, r
    # the two branches of infer_from_encoder on the same encoder outputs
    with torch.no_grad():
        gg = m.ref_enc(args[2].transpose(1, 2)).unsqueeze(-1)
        x, m_p, logs_p, x_mask = m.enc_p(args[0], args[1], args[4], args[5], gg)
        zh, _, yh = m.infer_from_encoder(x, m_p, logs_p, x_mask, args[1], args[2], args[3], gg, noise=noise)
        m.prior_backend = None
        try:
            zt, _, yt = m.infer_from_encoder(x, m_p, logs_p, x_mask, args[1], args[2], args[3], gg, noise=noise)
        finally:
            m.prior_backend = "hip"
    assert m.native_regulator_calls == before + 2
    assert torch.equal(yh, yt) and np.array_equal(yh.cpu().numpy(), g["y_len_out"])
    r = rel_l2(zh.cpu().numpy(), zt.cpu().numpy())
    print("z native regulator vs torch branch: rel_l2 %.3e" % r)
    assert r < 2e-4, r


def test_vits_turns_an_invalid_utterance_and_a_wrong_noise_shape_into_value_errors(prior):
    g, y, m = prior
    t = lambda k: _dev(g[k])       # noqa: E731
    logw = torch.zeros((2, 1, g["enc_x"].shape[2]), device="cuda")
    logw[1, 0, 3] = 40.0
    dp, calls = m.dp, m.native_regulator_calls
    try:
        m.dp = _FixedDurations(logw)
        with pytest.raises(ValueError, match="utterance 1"):
            m.infer_from_encoder(t("enc_x"), t("enc_m_p"), t("enc_logs_p"), t("enc_x_mask"), t("x_lengths"), _dev(y), t("y_lengths"))
        m.dp = _FixedDurations(torch.zeros_like(logw))
        with pytest.raises(ValueError, match="noise must be"):
            m.infer_from_encoder(t("enc_x"), t("enc_m_p"), t("enc_logs_p"), t("enc_x_mask"), t("x_lengths"), _dev(y), t("y_lengths"),
                                 noise=torch.zeros(2, 128, 3, device="cuda"))
    finally:
        m.dp = dp
    torch.cuda.synchronize()
    assert m.native_regulator_calls == calls
