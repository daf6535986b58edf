"""CPU: enrolled voices on the torch backend (NaturalSpeech2.enroll_voice, sample_from_prior(voices=), a Voice in
tts_infer.synthesize's refer slot) - the same arithmetic on stored encoder states, so every comparison is exact - and the
host-side validation.  The native records (dv_voice_*) are the business of tests/test_gpu_voices.py."""
import numpy as np
import pytest
import torch

from diff_vits_amd import synth, tts_infer
from diff_vits_amd.engine import Voice
from test_prompt_cpu import PassThroughVocoder, diffusion_state_dict, sample_case
from test_tts_infer import reference_checkpoint


@pytest.fixture(scope="module")
def ns2(gold):
    g, cfg, NaturalSpeech2, content, refer, noise = sample_case(gold)
    m = NaturalSpeech2(cfg, backend="torch").eval()
    m.diff_model.load_state_dict({k: torch.from_numpy(v) for k, v in diffusion_state_dict(cfg["diffusion_encoder"]).items()})
    return g, m, torch.from_numpy(content), torch.from_numpy(refer), torch.from_numpy(noise)


def test_voices_equal_refer_path_on_torch_backend(ns2):
    g, m, content, refer, noise = ns2
    lengths = torch.from_numpy(g["spec_lengths"])
    _, mel_ref = m.sample_from_prior(content, refer, None, lengths, None, "dpmsolver", noise=noise)
    voices = m.enroll_voice(refer, lengths)
    assert len(voices) == refer.shape[0] and all(isinstance(v, Voice) for v in voices)
    v = voices[0]
    assert v.L == refer.shape[2] and v.rebuilds == 0 and v.nbytes == 0 and v.enc.shape == (1, refer.shape[2], 128)
    assert torch.equal(v.refer, refer[:1]) and torch.equal(v.refer_length, lengths[:1])
    _, mel = m.sample_from_prior(content, voices=voices, sample_method="dpmsolver", noise=noise)      # refer may be None
    assert torch.equal(mel, mel_ref)


def test_voice_validation_errors(ns2):
    g, m, content, refer, noise = ns2
    lengths = torch.from_numpy(g["spec_lengths"])
    voices = m.enroll_voice(refer, lengths)
    with pytest.raises(ValueError, match="guidance"):
        m.sample_from_prior(content, voices=voices, noise=noise, guidance_scale=2.0)
    with pytest.raises(ValueError, match="one Voice per batch row"):
        m.sample_from_prior(content, voices=voices + voices, noise=noise)
    with pytest.raises(ValueError, match="refer"):
        m.sample_from_prior(content, noise=noise)
    short = Voice(voices[0].enc[:, :-1].clone())
    short.mask = voices[0].mask[:, :-1].clone()
    with pytest.raises(ValueError, match="key length"):
        m.sample_from_prior(torch.cat([content, content]), voices=[voices[0], short], noise=torch.cat([noise, noise]))
    with pytest.raises(ValueError, match="mel prompt"):
        tts_infer.synthesize(m, None, None, [(torch.zeros(1, 4, dtype=torch.long),) * 3 + (short, [4])], None, "cpu")


def test_voice_in_synthesize_refer_slot(gold, tmp_path):
    path, cfg, g, gf, y = reference_checkpoint(gold, tmp_path)
    model = tts_infer.load_model(path, "cpu", cfg, backend="torch")
    T = gf["mel"].shape[2]
    x_T = torch.from_numpy(synth.normal(1234, "full.x_T", (1, cfg["diffusion_encoder"]["in_channels"], T)))
    pn = torch.from_numpy(synth.normal(1234, "full.prior_noise", (1, 128, T)))
    spec = torch.from_numpy(y[:1])
    head = (torch.from_numpy(g["text"][:1]), torch.from_numpy(g["tone"][:1]), torch.from_numpy(g["language"][:1]))
    kw = dict(sample_method="unipc", noise=x_T, prior_noise=pn)
    audio_ref, mel_ref = tts_infer.synthesize(model, cfg, PassThroughVocoder(), [head + (spec, g["x_lengths"][:1].tolist())], None,
                                              "cpu", prompt_length="frames", **kw)
    voice, = model.enroll_voice(spec, torch.tensor([spec.shape[2]]))
    calls = []
    enc_fn = model.diff_model.prompt_encoder.encode_channels_last
    model.diff_model.prompt_encoder.encode_channels_last = lambda *a, **k: (calls.append(1), enc_fn(*a, **k))[1]
    try:
        audio, mel = tts_infer.synthesize(model, cfg, PassThroughVocoder(), [head + (voice, g["x_lengths"][:1].tolist())], None, "cpu", **kw)
    finally:
        del model.diff_model.prompt_encoder.encode_channels_last
    assert not calls                                       # the diffusion side did not encode the prompt again
    assert torch.equal(mel, mel_ref) and torch.equal(audio, audio_ref)
    assert np.isfinite(mel.numpy()).all()
