"""GPU: forced alignment on the device (dv_op_mas_scores / dv_op_mas_path, csrc/kernels_align.hip; VITS.align(align_backend='hip'))
and duration-pinned synthesis on the native regulator, against the restatements of tests/align_cases.py: the search's integers
IDENTICAL on cases that each cross one boundary of the kernel, the scores within the bound that follows from the kernel's documented
rounding order, the product route exact against the restated search on the kernel's own scores, graph capture, and the edit recipe
(align -> splice -> infer(durations=) -> edit_known_frames -> sample_from_prior(known_mel=)) end to end."""
import numpy as np
import pytest
import torch

import align_cases as A
from conftest import rel_l2

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda().contiguous()


def run_path(V, y_len, x_len):
    """-> (durations int32 [B, Tx], frame_token int32 [B, Ty]) device tensors; the input must come back untouched"""
    from diff_vits_amd import _lib
    L = _lib.lib()
    B, Ty, Tx = V.shape
    dur = torch.full((B, Tx), -7, dtype=torch.int32, device="cuda")
    tok = torch.full((B, Ty), -7, dtype=torch.int32, device="cuda")
    need = L.dv_op_mas_scratch_bytes(B, Ty, Tx)
    assert need >= 0
    scratch = torch.zeros((need,), dtype=torch.uint8, device="cuda") if need else None
    _lib.check(L.dv_op_mas_path(_lib.ptr(V), _lib.ptr(y_len), _lib.ptr(x_len), B, Ty, Tx, _lib.ptr(dur), _lib.ptr(tok), _lib.ptr(scratch),
                                need, _lib.stream_ptr()), "dv_op_mas_path")
    return dur, tok


def run_scores(z, m_p, logs_p, y_len, x_len):
    from diff_vits_amd import _lib
    B, C, Ty = z.shape
    Tx = m_p.shape[2]
    out = torch.full((B, Ty, Tx), float("nan"), device="cuda")
    _lib.check(_lib.lib().dv_op_mas_scores(_lib.ptr(z), _lib.ptr(m_p), _lib.ptr(logs_p), _lib.ptr(y_len), _lib.ptr(x_len), B, C, Ty, Tx,
                                           _lib.ptr(out), _lib.stream_ptr()), "dv_op_mas_scores")
    return out


@pytest.mark.parametrize("name", sorted(A.SEARCH_CASES))
def test_search_is_identical_to_the_restatement(name):
    from diff_vits_amd import _lib
    c = A.make_search_case(name)
    want_dur, want_tok, _ = A.search_reference(name)
    V, y_len, x_len = _dev(c["V"]), _dev(c["y_len"]), _dev(c["x_len"])
    before = V.clone()
    B, Ty, Tx = V.shape
    in_lds = _lib.lib().dv_op_mas_scratch_bytes(B, Ty, Tx) == 0
    assert in_lds == (name != "bits_in_scratch")
    dur, tok = run_path(V, y_len, x_len)
    torch.cuda.synchronize()
    assert torch.equal(V, before)                                          # read only: the reference accumulates in place
    dur, tok = dur.cpu().numpy(), tok.cpu().numpy()
    A.check_path(dur, tok, c["y_len"], c["x_len"])
    assert np.array_equal(tok, want_tok), (name, np.argwhere(tok != want_tok)[:4])
    assert np.array_equal(dur, want_dur), (name, dur, want_dur)
    if name == "all_zero":
        assert dur[0].tolist() == [1] * 4 + [8]                            # ties stay on the token (derived in align_cases.py)
    if name == "refused_between":
        assert (dur[1] == -1).all() and (dur[[0, 2]] >= 0).all()


def test_more_than_512_tokens_and_bad_arguments_are_refused_before_a_launch():
    from diff_vits_amd import _lib
    L = _lib.lib()
    f = torch.zeros(513 * 4, device="cuda")
    i32 = torch.zeros(600, dtype=torch.int32, device="cuda")
    i64 = torch.ones(1, dtype=torch.int64, device="cuda")
    p, s = _lib.ptr, _lib.stream_ptr()
    assert L.dv_op_mas_scratch_bytes(1, 4, 513) == -1 and L.dv_op_mas_scratch_bytes(1, 1024, 512) == 0
    assert L.dv_op_mas_scratch_bytes(2, 1025, 512) == 2 * 1025 * 64 and L.dv_op_mas_scratch_bytes(16, 1047, 150) == 0
    assert L.dv_op_mas_path(p(f), p(i64), p(i64), 1, 4, 513, p(i32), p(i32), None, 0, s) == -1 and b"Tx = 513" in L.dv_last_error()
    assert L.dv_op_mas_path(None, p(i64), p(i64), 1, 4, 4, p(i32), p(i32), None, 0, s) == -1 and b"null" in L.dv_last_error()
    assert L.dv_op_mas_path(p(f), p(i64), p(i64), 0, 4, 4, p(i32), p(i32), None, 0, s) == -1
    assert L.dv_op_mas_path(p(f), p(i64), p(i64), 1, 1025, 512, p(i32), p(i32), None, 0, s) == -1 and b"scratch" in L.dv_last_error()
    assert L.dv_op_mas_scores(p(f), p(f), None, p(i64), p(i64), 1, 2, 4, 4, p(f), s) == -1
    for dims in ((0, 2, 4, 4), (1, 0, 4, 4), (1, 2, 0, 4), (1, 2, 4, 0)):
        assert L.dv_op_mas_scores(p(f), p(f), p(f), p(i64), p(i64), *dims, p(f), s) == -1
    torch.cuda.synchronize()
    assert float(f.abs().sum()) == 0 and int(i32.abs().sum()) == 0


@pytest.mark.parametrize("name", sorted(A.SCORE_CASES))
def test_scores_within_the_bound_of_the_documented_rounding_order(name):
    C, Ty, Tx, y_len, x_len = A.SCORE_CASES[name]
    z, m_p, logs_p = A.score_inputs(name, len(y_len), C, Ty, Tx)
    ref, bound = A.scores_ref(z, m_p, logs_p, y_len, x_len)
    out = run_scores(_dev(z), _dev(m_p), _dev(logs_p), _dev(np.array(y_len, np.int64)), _dev(np.array(x_len, np.int64)))
    torch.cuda.synchronize()
    out = out.cpu().numpy().astype(np.float64)
    inside = bound > 0
    worst = float((np.abs(out - ref)[inside] / bound[inside]).max())
    print("scores %-9s worst error / bound %.3f   (bound up to %.3g on scores down to %.4g)" % (name, worst, bound.max(), ref.min()))
    assert np.isfinite(out).all() and (out[~inside] == 0).all()                 # padding cells are exactly zero
    assert worst <= 1.0


@pytest.fixture(scope="module")
def aligner(gold):
    from test_align_cpu import align_case, align_mirror
    g, sd, y, noise = align_case(gold)
    m = align_mirror(g, sd).cuda()
    args = [_dev(a) for a in (g["text"], g["x_lengths"], y, g["y_lengths"], g["tone"], g["language"])]
    return g, m, args, _dev(noise)


def test_align_on_the_golden_is_the_restated_search_on_the_kernels_own_scores(aligner):
    from test_align_cpu import golden_path
    g, m, args, noise = aligner
    before = m.native_align_calls
    dur, tok, scores = m.align(*args, noise=noise, align_backend="hip", return_scores=True)
    torch.cuda.synchronize()
    assert m.native_align_calls == before + 1 and dur.dtype == torch.int64 and tok.dtype == torch.int64 and dur.is_cuda
    want_dur, want_tok, margin = A.search_ref(scores.cpu().numpy(), g["y_lengths"], g["x_lengths"])
    assert np.array_equal(dur.cpu().numpy(), want_dur) and np.array_equal(tok.cpu().numpy(), want_tok)      # exact by construction
    gd, gt = golden_path(g)
    r = max(rel_l2(scores[b, :ty, :tx].cpu().numpy(), g["neg_cent"][b, :ty, :tx])          # (the reference leaves its padding unmasked)
            for b, (ty, tx) in enumerate(zip(g["y_lengths"], g["x_lengths"])))
    print("golden: kernel scores vs reference rel_l2 %.3e, smallest decision margin %.3g" % (r, margin))
    assert r < 1e-5
    assert np.array_equal(dur.cpu().numpy(), gd) and np.array_equal(tok.cpu().numpy(), gt)                # and the reference's path
    # the torch route on the same GPU tensors agrees; an utterance with fewer frames than tokens is named
    d2, t2 = m.align(*args, noise=noise)
    assert torch.equal(d2, dur) and torch.equal(t2, tok) and m.native_align_calls == before + 1
    short = args[3].clone()
    short[1] = int(g["x_lengths"][1]) - 1
    with pytest.raises(ValueError, match="utterance 1"):
        m.align(args[0], args[1], args[2], short, args[4], args[5], noise=noise, align_backend="hip")


def test_both_operators_in_one_graph_replayed_with_other_inputs():
    from diff_vits_amd import _lib
    C, Ty, Tx, y_len, x_len = A.SCORE_CASES["tile_edge"]
    B = len(y_len)
    sets = [A.score_inputs("graph%d" % i, B, C, Ty, Tx) for i in range(3)]
    yl, xl = _dev(np.array(y_len, np.int64)), _dev(np.array(x_len, np.int64))
    eager = []
    for z, m_p, logs_p in sets:
        sc = run_scores(_dev(z), _dev(m_p), _dev(logs_p), yl, xl)
        dur, tok = run_path(sc, yl, xl)
        torch.cuda.synchronize()
        eager.append((sc.clone(), dur.clone(), tok.clone()))
    L = _lib.lib()
    z, m_p, logs_p = (_dev(a) for a in sets[0])
    sc = torch.zeros((B, Ty, Tx), device="cuda")
    dur = torch.zeros((B, Tx), dtype=torch.int32, device="cuda")
    tok = torch.zeros((B, Ty), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.check(L.dv_op_mas_scores(_lib.ptr(z), _lib.ptr(m_p), _lib.ptr(logs_p), _lib.ptr(yl), _lib.ptr(xl), B, C, Ty, Tx, _lib.ptr(sc),
                                      _lib.stream_ptr()), "dv_op_mas_scores")
        _lib.check(L.dv_op_mas_path(_lib.ptr(sc), _lib.ptr(yl), _lib.ptr(xl), B, Ty, Tx, _lib.ptr(dur), _lib.ptr(tok), None, 0,
                                    _lib.stream_ptr()), "dv_op_mas_path")
    for (a, b, c), want in zip(sets[1:], eager[1:]):
        z.copy_(_dev(a)), m_p.copy_(_dev(b)), logs_p.copy_(_dev(c))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(sc, want[0]) and torch.equal(dur, want[1]) and torch.equal(tok, want[2])
    assert not torch.equal(eager[1][2], eager[2][2])


def test_pinned_durations_native_regulator_vs_torch_branch(gold):
    """durations= on prior_backend='hip' against the torch branch of the same model on the same encoder outputs: y_len and the
    resolved durations identical, z within the regulator's existing bound (tests/test_gpu_regulator.py: 2e-4)."""
    import ast
    from test_prompt_cpu import prior_case
    from diff_vits_amd import synth
    from diff_vits_amd.model3 import VITS
    g, sd, y = prior_case(gold)
    kw = ast.literal_eval(str(g["vits_kwargs"]))
    m = VITS(int(g["n_vocab"]), 513, n_tones=int(g["n_tones"]), n_languages=int(g["n_languages"]), backend="hip",
             text_encoder_backend="hip", prior_backend="hip", **kw).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.cuda()
    enc = [_dev(g[k]) for k in ("enc_x", "enc_m_p", "enc_logs_p", "enc_x_mask", "x_lengths")] + [_dev(y), _dev(g["y_lengths"])]
    B, C, Tx = g["enc_m_p"].shape
    given = torch.full((B, Tx), -1, dtype=torch.int64)
    given[0, 1], given[0, 4], given[1, 0], given[1, 5] = 7, 0, 3, 12
    outs = {}
    for backend in ("hip", None):
        m.prior_backend = backend
        try:
            calls = m.native_regulator_calls
            _, _, y_plain = m.infer_from_encoder(*enc)
            noise = torch.from_numpy(synth.normal(5, "pinned.noise", (B, C, 200))).cuda()
            # the noise's length is the run's frame count: resolve the durations first, then run with a noise of that length
            d = m.infer_from_encoder(*enc, durations=given.cuda(), return_durations=True)[3]
            T = int(d.sum(1).max())
            z, _, y_len, d2 = m.infer_from_encoder(*enc, durations=given.cuda(), return_durations=True, noise=noise[:, :, :T].contiguous())
            assert m.native_regulator_calls == calls + (3 if backend == "hip" else 0)
        finally:
            m.prior_backend = "hip"
        assert torch.equal(d, d2) and torch.equal(y_len, d.sum(1))
        outs[backend] = (z, y_len, d, y_plain)
    torch.cuda.synchronize()
    (zh, yh, dh, ph), (zt, yt, dt, pt) = outs["hip"], outs[None]
    assert torch.equal(yh, yt) and torch.equal(dh, dt) and torch.equal(ph, pt) and not torch.equal(yh, ph)
    assert dh[0, 1] == 7 and dh[0, 4] == 0 and dh[1, 0] == 3 and dh[1, 5] == 12
    r = rel_l2(zh.cpu().numpy(), zt.cpu().numpy())
    print("pinned durations: z native regulator vs torch branch rel_l2 %.3e" % r)
    assert r < 2e-4, r


def test_edit_recipe_end_to_end(gold, aligner, monkeypatch):
    """Align a recording, replace one token by two whose durations are predicted, synthesise on the pinned durations, build the
    known frames, infill: the kept frames of the returned mel are the recording's, and the run is one graph replay."""
    from test_prompt_cpu import diffusion_state_dict, sample_case
    from diff_vits_amd.model3 import edit_known_frames
    from diff_vits_amd.sampler import _plan
    from diff_vits_amd.sampler.uni_pc import UniPC
    g, vits, args, noise = aligner
    text, x_len, y, y_len, tone, lang = args
    _, cfg, NaturalSpeech2, *_ = sample_case(gold)
    ns2 = NaturalSpeech2(cfg, backend="hip").eval()
    ns2.diff_model.load_state_dict({k: torch.from_numpy(v) for k, v in diffusion_state_dict(cfg["diffusion_encoder"]).items()})
    ns2 = ns2.cuda()
    dur, _ = vits.align(*args, noise=noise, align_backend="hip")                              # 1. align
    ins = lambda t, v: torch.cat([t[:, :3], torch.full_like(t[:, :2], v), t[:, 4:]], 1)       # noqa: E731  token 3 -> two tokens
    new_text, new_tone, new_lang = ins(text, 5), ins(tone, 1), ins(lang, 0)
    new_d = torch.cat([dur[:, :3], torch.full_like(dur[:, :2], -1), dur[:, 4:]], 1)           # 2. splice
    new_d[:, 3] = 14                                                                           # (one pinned by hand, one predicted)
    z, _, d_res = vits.infer(new_text, x_len + 1, y, y_len, new_tone, new_lang, durations=new_d, return_durations=True)   # 3.
    assert torch.equal(d_res[:, :3], dur[:, :3]) and (d_res[:, 3] == 14).all() and (d_res[:, 4] >= 0).all()
    known, mask = edit_known_frames(y, dur, d_res, [(3, 4)] * 2, [(3, 5)] * 2)               # 4. (the recording is the mel here)
    assert known.shape == (2, 100, z.shape[2]) and mask.shape == (2, z.shape[2]) and 48 <= z.shape[2] <= 96
    x_T = torch.randn(known.shape, generator=torch.Generator().manual_seed(1)).cuda()
    real_sample = UniPC.sample
    monkeypatch.setattr(UniPC, "sample", lambda self, x, steps=20, **k: real_sample(self, x, steps=3, **k))     # a 3-step solver

    def stepped(*a, **k):
        raise AssertionError("the recipe's run left the native graph path")
    monkeypatch.setattr(_plan.Plan, "run_python", stepped)
    mel = ns2.sample_from_prior(z, y, x_len + 1, y_len, None, "unipc", noise=x_T, known_mel=known, known_mask=mask)[1]     # 5.
    mel2 = ns2.sample_from_prior(z, y, x_len + 1, y_len, None, "unipc", noise=x_T, known_mel=known, known_mask=mask)[1]
    torch.cuda.synchronize()
    keep = mask[:, None, :].expand_as(mel)
    assert torch.isfinite(mel).all() and torch.equal(mel[keep], known[keep]) and torch.equal(mel2, mel)
    assert not torch.equal(mel[~keep], known[~keep])
    plans = [p for p in ns2._native_samplers["unipc"]["solver"]._plans.values() if p.known_frames]
    assert len(plans) == 1 and len([q.graph_nodes() for q in plans[0]._per_shape.values()]) == 1      # one graph, replayed
