"""CPU: forced alignment and duration-pinned synthesis (VITS.align, durations=, edit_known_frames; diff_vits_amd/model3.py) against
the reference's own run (tests/golden/align_forward.npz, tools/make_golden_align.py) and the restatements of tests/align_cases.py;
and the planted faults that the bounds of the GPU tests (tests/test_gpu_align.py) must be able to catch."""
import ast

import numpy as np
import pytest
import torch

import align_cases as A
from conftest import rel_l2
from diff_vits_amd import synth, tts_infer
from diff_vits_amd.model3 import VITS, PosteriorEncoder, edit_known_frames, mas_scores, mas_search
from test_prompt_cpu import prior_case, vits_mirror


def align_case(gold):
    g = gold("align_forward.npz")
    names = [str(n) for n in g["names"]]
    shapes = {n: ast.literal_eval(str(s)) for n, s in zip(names, g["shapes"])}
    sd = synth.make_state_dict(shapes, seed=1234)
    for k in ("enc_p.proj.weight", "enc_p.proj.bias"):                  # the fixture's gain (tools/make_golden_align.py)
        sd[k] = (sd[k] * np.float32(g["proj_gain"])).astype(np.float32)
    y = synth.normal(1234, "align.mel", (2, 100, int(g["Ty"])))
    noise = synth.normal(1234, "align.noise", tuple(g["z"].shape))
    return g, sd, y, noise


def align_mirror(g, sd, **kw):
    """VITS(aligner=True) with the fixture's ref_enc / enc_p / enc_q weights (dp and o_proj, which align never runs, keep
    their initial values)."""
    vkw = ast.literal_eval(str(g["vits_kwargs"]))
    m = VITS(int(g["n_vocab"]), 513, n_tones=int(g["n_tones"]), n_languages=int(g["n_languages"]), aligner=True, **dict(vkw, **kw)).eval()
    res = m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not res.unexpected_keys and all(k.split(".")[0] in ("dp", "o_proj") for k in res.missing_keys)
    return m


def golden_path(g):
    """(durations [B, Tx], frame_token [B, Ty]) of the reference's 0/1 path tensor [B, Ty, Tx]."""
    path = g["path"].astype(np.int64)
    tok = np.where(path.sum(2) > 0, path.argmax(2), -1)
    assert (path.sum(2) <= 1).all()
    return path.sum(1), tok


def test_search_restatement_equals_the_reference_path(gold):
    g = gold("align_forward.npz")
    dur, tok, margin = A.search_ref(g["neg_cent"], g["y_lengths"], g["x_lengths"])
    gd, gt = golden_path(g)
    assert np.array_equal(dur, gd) and np.array_equal(dur, g["w"]) and np.array_equal(tok, gt)
    A.check_path(dur, tok, g["y_lengths"], g["x_lengths"])
    # the package's own host search says the same, and leaves its input alone
    nc = torch.from_numpy(g["neg_cent"].copy())
    d2, t2 = mas_search(nc, torch.from_numpy(g["y_lengths"]), torch.from_numpy(g["x_lengths"]))
    assert np.array_equal(d2.numpy(), gd) and np.array_equal(t2.numpy(), gt) and np.array_equal(nc.numpy(), g["neg_cent"])


def test_score_restatement_equals_the_reference_scores_and_the_margin_is_wide(gold):
    g = gold("align_forward.npz")
    ref, bound = A.scores_ref(g["z"], g["m_p"], g["logs_p"], g["y_lengths"], g["x_lengths"])
    inside = bound > 0
    # the reference's tensor is float32 torch.matmul on the CPU: inside the kernel's own bound of the float64 value
    assert (np.abs(g["neg_cent"] - ref)[inside] <= bound[inside]).all()
    ours = mas_scores(torch.from_numpy(g["z"]), torch.from_numpy(g["m_p"]), torch.from_numpy(g["logs_p"])).numpy()
    assert (np.abs(ours - ref)[inside] <= bound[inside]).all()
    # no decision of the golden path is near a tie (align_cases.py): the smallest margin is far above the score bound, and far
    # above what float32 scores as far from the exact ones as the reference's own can move a Q (2 t_y times that distance)
    _, _, margin = A.search_ref(g["neg_cent"], g["y_lengths"], g["x_lengths"])
    seen = float(np.abs(g["neg_cent"] - ref)[inside].max())
    print("golden: smallest decision margin %.3g, largest score bound %.3g, reference's scores within %.3g of float64"
          % (margin, bound.max(), seen))
    assert margin > 20 * float(bound.max()) and margin > 20 * 2 * int(g["y_lengths"].max()) * seen


def test_posterior_encoder_mirror(gold):
    g, sd, y, noise = align_case(gold)
    m = align_mirror(g, sd)
    own = {k for k in m.state_dict() if k.startswith("enc_q.")}
    assert own == {k for k in sd if k.startswith("enc_q.")} and any(k.endswith("weight_g") for k in own)
    assert isinstance(m.enc_q, PosteriorEncoder)
    with torch.no_grad():
        gg = m.ref_enc(torch.from_numpy(y).transpose(1, 2)).unsqueeze(-1)
        z, mq, logs, mask = m.enc_q(torch.from_numpy(y), torch.from_numpy(g["y_lengths"]), gg, noise=torch.from_numpy(noise))
    for a, k in ((z, "z"), (mq, "m_q"), (logs, "logs_q")):
        assert rel_l2(a.numpy(), g[k]) < 1e-5, k
    assert mask.shape == (2, 1, int(g["Ty"])) and mask.sum().item() == g["y_lengths"].sum()
    torch.manual_seed(3)
    with torch.no_grad():
        z2 = m.enc_q(torch.from_numpy(y), torch.from_numpy(g["y_lengths"]), gg)[0]          # noise=None draws
    assert not torch.equal(z2, z)
    assert not hasattr(VITS(11, 513), "enc_q")                                      # the default builds none


def test_align_torch_route_matches_the_reference(gold):
    g, sd, y, noise = align_case(gold)
    m = align_mirror(g, sd)
    t = lambda k: torch.from_numpy(g[k])       # noqa: E731
    args = (t("text"), t("x_lengths"), torch.from_numpy(y), t("y_lengths"), t("tone"), t("language"))
    dur, tok, scores = m.align(*args, noise=torch.from_numpy(noise), return_scores=True)
    gd, gt = golden_path(g)
    assert dur.dtype == torch.int64 and tok.dtype == torch.int64
    assert np.array_equal(dur.numpy(), gd) and np.array_equal(tok.numpy(), gt)
    assert rel_l2(scores.numpy(), g["neg_cent"]) < 1e-5 and m.native_align_calls == 0
    assert len(m.align(*args, noise=torch.from_numpy(noise))) == 2
    with pytest.raises(RuntimeError, match="GPU tensors"):
        m.align(*args, align_backend="hip")                                          # never a fall-back
    with pytest.raises(ValueError, match="align_backend"):
        m.align(*args, align_backend="torch")
    short = t("y_lengths").clone()
    short[1] = int(g["x_lengths"][1]) - 1                                           # fewer frames than tokens
    with pytest.raises(ValueError, match="utterance 1"):
        m.align(args[0], args[1], args[2], short, args[4], args[5], noise=torch.from_numpy(noise))
    with pytest.raises(RuntimeError, match="aligner=True"):
        VITS(int(g["n_vocab"]), 513).align(*args)


def _prior(gold):
    g, sd, y = prior_case(gold)
    m = vits_mirror(g, sd, "torch")
    t = lambda k: torch.from_numpy(g[k])       # noqa: E731
    enc = (t("enc_x"), t("enc_m_p"), t("enc_logs_p"), t("enc_x_mask"), t("x_lengths"), torch.from_numpy(y), t("y_lengths"))
    return g, m, enc


def test_pinned_durations(gold):
    g, m, enc = _prior(gold)
    B, C, Tx = g["enc_m_p"].shape
    noise = torch.from_numpy(synth.normal(1234, "prior.noise", tuple(g["z"].shape)))
    z0, _, y0 = m.infer_from_encoder(*enc, noise=noise)
    keep = torch.full((B, Tx), -1, dtype=torch.int64)
    z1, _, y1, d1 = m.infer_from_encoder(*enc, noise=noise, durations=keep, return_durations=True)
    assert torch.equal(z1, z0) and torch.equal(y1, y0)                              # all -1 is durations=None, exactly
    x_len = g["x_lengths"]
    assert d1.dtype == torch.int64 and np.array_equal(d1.sum(1).numpy(), g["y_len_out"])
    assert all((d1[b, x_len[b]:] == 0).all() for b in range(B))
    # every token pinned: the frame counts are the sums, and each frame's statistics are its token's
    given = torch.from_numpy(((synth.uniform(5, "pinned", (B, Tx)) * 0.5 + 0.5) * 4).astype(np.int64))       # 0 .. 3 frames
    given[0, 0] = 2
    inside = torch.arange(Tx)[None] < torch.from_numpy(x_len)[:, None]
    want_len = (given * inside).sum(1)
    seen = {}

    class Capture(torch.nn.Module):
        def forward(self, z_p, y_len, gg):
            return seen.setdefault("z_p", z_p)
    o_proj = m.o_proj
    m.o_proj = Capture()
    try:
        zero = torch.zeros((B, C, int(want_len.max())))
        _, _, y2, d2 = m.infer_from_encoder(*enc, noise=zero, durations=given, return_durations=True)      # zero noise: z_p = m_p
    finally:
        m.o_proj = o_proj
    assert torch.equal(y2, want_len) and torch.equal(d2, given * inside)
    for b in range(B):
        tok = torch.repeat_interleave(torch.arange(Tx), d2[b])
        assert torch.equal(seen["z_p"][b, :, :len(tok)], enc[1][b][:, tok])
        assert (seen["z_p"][b, :, len(tok):] == 0).all()
    # a mixed tensor changes only the pinned token's count; infer() hands both keywords through
    mixed = keep.clone()
    mixed[0, 2] = int(d1[0, 2]) + 5
    _, _, y3, d3 = m.infer_from_encoder(*enc, durations=mixed, return_durations=True)
    assert int(y3[0]) == int(y0[0]) + 5 and int(y3[1]) == int(y0[1]) and torch.equal(d3[1], d1[1])
    t = lambda k: torch.from_numpy(g[k])       # noqa: E731
    out = m.infer(t("text"), t("x_lengths"), enc[5], t("y_lengths"), t("tone"), t("language"), durations=given, return_durations=True)
    assert len(out) == 3 and torch.equal(out[2], given * inside) and out[0].shape[2] == int(want_len.max())
    for bad in (given.float(), given[:, :-1], torch.full_like(given, -2)):
        with pytest.raises(ValueError, match="durations"):
            m.infer_from_encoder(*enc, durations=bad)


def test_edit_known_frames():
    old = torch.tensor([[2, 3, 1, 4, 0], [1, 1, 5, 2, 2]])                           # 10 and 11 frames
    mel = torch.arange(2 * 3 * 11, dtype=torch.float32).reshape(2, 3, 11) + 1       # no zero among the frames
    # utterance 0: token 1 (3 frames) -> two tokens of 2 + 4 frames (longer); utterance 1: tokens 2..3 (7 frames) -> one of 3 (shorter)
    new = torch.tensor([[2, 2, 4, 1, 4, 0], [1, 1, 3, 2, 0, 0]])
    km, mask = edit_known_frames(mel, old, new, [(1, 2), (2, 4)], [(1, 3), (2, 3)])
    assert km.shape == (2, 3, 13) and mask.shape == (2, 13) and mask.dtype == torch.bool
    assert mask[0].tolist() == [True] * 2 + [False] * 6 + [True] * 5
    assert torch.equal(km[0, :, :2], mel[0, :, :2]) and torch.equal(km[0, :, 8:13], mel[0, :, 5:10]) and (km[0, :, 2:8] == 0).all()
    assert mask[1].tolist() == [True] * 2 + [False] * 3 + [True] * 2 + [False] * 6
    assert torch.equal(km[1, :, 5:7], mel[1, :, 9:11]) and (km[1, :, 7:] == 0).all() and (km[1, :, 2:5] == 0).all()
    # a span at the start (an insertion before token 0) and one at the end (the last tokens replaced)
    km, mask = edit_known_frames(mel[:1], old[:1], torch.tensor([[3, 2, 3, 1, 4, 0]]), [(0, 0)], [(0, 1)])
    assert mask[0].tolist() == [False] * 3 + [True] * 10 and torch.equal(km[0, :, 3:], mel[0, :, :10])
    km, mask = edit_known_frames(mel[:1], old[:1], torch.tensor([[2, 3, 6]]), [(2, 5)], [(2, 3)])
    assert mask[0].tolist() == [True] * 5 + [False] * 6 and torch.equal(km[0, :, :5], mel[0, :, :5])
    # refusals: an unchanged token with another duration (before and behind the span), unresolved durations, spans that do not line up
    with pytest.raises(ValueError, match="unchanged token 0"):
        edit_known_frames(mel[:1], old[:1], torch.tensor([[3, 2, 4, 1, 4]]), [(1, 2)], [(1, 3)])
    with pytest.raises(ValueError, match="unchanged token 3"):
        edit_known_frames(mel[:1], old[:1], torch.tensor([[2, 2, 4, 1, 5]]), [(1, 2)], [(1, 3)])
    with pytest.raises(ValueError, match="resolved"):
        edit_known_frames(mel[:1], old[:1], torch.tensor([[2, -1, 4, 1, 4]]), [(1, 2)], [(1, 3)])
    with pytest.raises(ValueError, match="same token"):
        edit_known_frames(mel[:1], old[:1], new[:1], [(1, 2)], [(2, 3)])


def test_build_model_loads_the_posterior_encoder_on_request(gold):
    from test_tts_infer import chain_cfg
    g, sd, _ = prior_case(gold)
    cfg = chain_cfg(g, gold("sample_full.npz"))
    plain = tts_infer.build_model(cfg, int(g["n_vocab"]), backend="torch")
    with_q = tts_infer.build_model(cfg, int(g["n_vocab"]), backend="torch", aligner=True)
    q_keys = [k for k in with_q.state_dict() if k.startswith("vits.enc_q.")]
    assert q_keys and not any(k.startswith("vits.enc_q.") for k in plain.state_dict())
    ckpt = {k: v.clone() for k, v in with_q.state_dict().items()}
    for k in q_keys:
        ckpt[k] = torch.full_like(ckpt[k], 0.25)
    assert tts_infer.load_state(with_q, ckpt) == [] and all(bool((with_q.state_dict()[k] == 0.25).all()) for k in q_keys)
    assert sorted(tts_infer.load_state(plain, ckpt)) == sorted(q_keys)             # the default still skips them ...
    with pytest.raises(RuntimeError, match="unknown"):                               # ... and nothing else
        tts_infer.load_state(plain, dict(ckpt, **{"vits.flow.x": torch.zeros(1)}))
    with pytest.raises(RuntimeError, match="lacks"):
        tts_infer.load_state(with_q, {k: v for k, v in ckpt.items() if k != q_keys[0]})


def test_all_zero_scores_stay_on_the_token():
    c = A.make_search_case("all_zero")
    dur, tok, _ = A.search_reference("all_zero")
    ty, tx = int(c["y_len"][0]), int(c["x_len"][0])
    assert dur[0].tolist() == [1] * (tx - 1) + [ty - tx + 1]                         # derived in align_cases.py
    d2, _ = mas_search(torch.from_numpy(c["V"]), torch.from_numpy(c["y_len"]), torch.from_numpy(c["x_len"]))
    assert d2[0].tolist() == dur[0].tolist()


@pytest.mark.parametrize("name", sorted(A.SEARCH_CASES))
def test_host_search_equals_the_restatement_on_every_case(name):
    c = A.make_search_case(name)
    if c["V"].shape[1] > 700:
        c = dict(c, V=c["V"][:, :, :64].copy(), x_len=np.minimum(c["x_len"], 60))   # (the torch route is slow on 1025 x 512)
        dur, tok, _ = A.search_ref(c["V"], c["y_len"], c["x_len"])
    else:
        dur, tok, _ = A.search_reference(name)
    A.check_path(dur, tok, c["y_len"], c["x_len"])
    d2, t2 = mas_search(torch.from_numpy(c["V"]), torch.from_numpy(c["y_len"]), torch.from_numpy(c["x_len"]))
    assert np.array_equal(d2.numpy(), dur) and np.array_equal(t2.numpy(), tok)


def test_planted_faults_are_visible():
    """Each wrong variant of the restatements changes the integers (search) or leaves the score bound (scores) on at least one
    case: the GPU tests' exact comparison and bound would catch a kernel with that fault."""
    names = [n for n in sorted(A.SEARCH_CASES) if A.SEARCH_CASES[n]().get("V").shape[1] <= 100]
    for fault in ("tie", "sentinel", "band"):
        hit = []
        for n in names:
            c = A.make_search_case(n)
            dur, tok, _ = A.search_reference(n)
            fd, ft, _ = A.search_ref(c["V"], c["y_len"], c["x_len"], fault=fault)
            if not (np.array_equal(fd, dur) and np.array_equal(ft, tok)):
                hit.append(n)
        print("search fault %-8s changes: %s" % (fault, hit))
        assert hit, fault
    C, Ty, Tx, y_len, x_len = A.SCORE_CASES["small"]
    z, m_p, logs_p = A.score_inputs("small", len(y_len), C, Ty, Tx)
    ref, bound = A.scores_ref(z, m_p, logs_p, y_len, x_len)
    for fault in ("term", "shift"):
        bad, _ = A.scores_ref(z, m_p, logs_p, y_len, x_len, fault=fault)
        worst = float((np.abs(bad - ref) / np.where(bound > 0, bound, np.inf)).max())
        print("score fault %-6s: worst error / bound %.3g" % (fault, worst))
        assert worst > 1, fault
