"""GPU: the native text encoder against the REFERENCE's own tensors (tests/golden/prior_infer.npz: enc_x, enc_m_p, enc_logs_p,
enc_x_mask, made by the reference's TextEncoder) and inside the product chains: VITS.infer on the prior fixture, and
configuration 5 from phoneme ids to mel with text_encoder_backend='hip'."""
import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu


def _vits(gold, text_encoder_backend):
    from test_prompt_cpu import prior_case
    from diff_vits_amd.model3 import VITS
    import ast
    g, sd, y = prior_case(gold)
    kw = ast.literal_eval(str(g["vits_kwargs"]))
    m = VITS(int(g["n_vocab"]), 513, n_tones=int(g["n_tones"]), n_languages=int(g["n_languages"]), backend="hip",
             text_encoder_backend=text_encoder_backend, **kw).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return g, sd, y, m.cuda()


def test_text_encoder_hip_matches_reference_golden(gold):
    """dv_tenc_forward on the fixture's ids / tones / languages / lengths with g from the reference encoder: x, m_p, logs_p within
    2e-4 of the reference's (the bar of tests/test_gpu_prompt.py), padding exactly zero, the mask reproduced."""
    g, sd, y, m = _vits(gold, "hip")
    dev = lambda a: torch.from_numpy(a).cuda()       # noqa: E731
    assert m.enc_p.backend == "hip"
    with torch.no_grad():
        gg = m.ref_enc(dev(y).transpose(1, 2)).unsqueeze(-1)
        x, m_p, logs_p, x_mask = m.enc_p(dev(g["text"]), dev(g["x_lengths"]), dev(g["tone"]), dev(g["language"]), gg)
    for a, k in ((x, "enc_x"), (m_p, "enc_m_p"), (logs_p, "enc_logs_p")):
        r = rel_l2(a.cpu().numpy(), g[k])
        print("%s: rel_l2 %.3e" % (k, r))
        assert a.shape == g[k].shape and r < 2e-4, (k, r)
        pad = np.broadcast_to(g["enc_x_mask"] == 0, g[k].shape)
        assert bool((a.cpu().numpy()[pad] == 0).all()), "%s: a padding frame is not zero" % k
    assert np.array_equal(x_mask.cpu().numpy(), g["enc_x_mask"])
    assert m.enc_p.hip_engine().stats()[0] == 1 + 2 + 7 * 6 + 2


def test_prior_chain_with_native_text_encoder(gold):
    """VITS(..., backend='hip', text_encoder_backend='hip').infer on the fixture: integer frame counts identical to the reference's,
    z within 2e-4 (the fixture's durations are >= 1e-3 from a rounding boundary: tests/test_prompt_cpu.py)."""
    from diff_vits_amd import synth
    g, sd, y, m = _vits(gold, "hip")
    dev = lambda a: torch.from_numpy(a).cuda()       # noqa: E731
    noise = torch.from_numpy(synth.normal(1234, "prior.noise", tuple(g["z"].shape))).cuda()
    z, _ = m.infer(dev(g["text"]), dev(g["x_lengths"]), dev(y), dev(g["y_lengths"]), dev(g["tone"]), dev(g["language"]), noise=noise)
    assert z.shape == g["z"].shape                                   # T' = max of the integer frame counts
    frames = (z.abs().sum(1) != 0).sum(1).cpu().numpy()
    assert np.array_equal(frames, g["y_len_out"]), (frames, g["y_len_out"])
    assert rel_l2(z.cpu().numpy(), g["z"]) < 2e-4, rel_l2(z.cpu().numpy(), g["z"])


def test_config5_chain_ids_to_mel_with_native_text_encoder(gold):
    """BASELINE configuration 5 (B = 16, 36 tokens) from phoneme ids to mel as tests/test_gpu_prompt.py runs it, with the text
    encoder on the native engine too: frame counts identical, mel within 5e-4 of the reference's."""
    from test_prompt_cpu import config5_case, diffusion_state_dict
    from diff_vits_amd.model3 import NaturalSpeech2
    from diff_vits_amd.sampler import dpm_solver
    g5, dcfg, y, x_T, pn, x_lengths, y_lengths = config5_case(gold)
    g, sd, _, vits = _vits(gold, "hip")
    ns2 = NaturalSpeech2({"diffusion_encoder": dcfg, "train": {"timesteps": int(g5["timesteps"])}}, vits=vits, backend="hip").eval()
    ns2.diff_model.load_state_dict({k: torch.from_numpy(v) for k, v in diffusion_state_dict(dcfg).items()})
    ns2 = ns2.cuda()
    dev = lambda a: torch.from_numpy(a).cuda()       # noqa: E731
    with torch.no_grad():
        content, refer = ns2.vits.infer(dev(g5["text"]), dev(x_lengths), dev(y), dev(y_lengths), dev(g5["tone"]), dev(g5["language"]),
                                        noise=dev(pn))
        assert content.shape == (16, 128, int(g5["T"]))
        frames = (content.abs().sum(1) != 0).sum(1).cpu().numpy()
        assert np.array_equal(frames, g5["frames"]), (frames, g5["frames"])
        data = (content, refer, dev(x_lengths), dev(y_lengths))
        ns = dpm_solver.NoiseScheduleVP("discrete", betas=ns2.betas)
        fn = dpm_solver.model_wrapper(ns2.diff_model.native_model(data), ns, model_type="x_start")
        mel = dpm_solver.DPM_Solver(fn, ns, algorithm_type="dpmsolver++").sample(dev(x_T), steps=int(g5["steps"]), order=2,
                                                                                skip_type="time_uniform", method="multistep")
    assert ns2.diff_model.unet.hip_engine().wait()
    assert ns2.vits.enc_p.hip_engine().stats()[0] == 1 + 2 + 7 * 6 + 2
    r = rel_l2(mel.cpu().numpy(), g5["mel"])
    print("config 5 mel: rel_l2 %.3e" % r)
    assert mel.shape == g5["mel"].shape and r < 5e-4, r
