"""Host mirror of the reference's inference script glue (tts_infer.py:46-81): build the
model from a `{'step', 'model'}` checkpoint (model3.py:1326-1345), turn the reference audio into the log-mel prompt and
call `model.sample(phoneme, refer, phoneme_length, refer_length, tone, language, vocos)`.

What stays the reference's own: the text front-end (`text/`: G2P, cleaners, the symbol table) and the vocoder (Vocos) -
both are outside the diffusion hot path and their third-party dependencies are absent from this image.  So:
  * the size of the symbol table is taken from the checkpoint (`vits.enc_p.emb.weight`) unless `n_vocab` is passed;
  * `synthesize` takes batches whose reference audio is either a waveform tensor at 24 kHz (mel front-end of mel.py,
    pinned there to the fp64 restatement of its documented definition) or a ready log-mel prompt `[1, 100, L]`; a PATH needs torchaudio for decoding / resampling,
    exactly as in the reference, and raises ImportError when it is missing - unless `audio_backend="native"` asks for the package's
    own WAV reader and sample-rate converter (audio.py; `save_wav` is the way out).
Training-only checkpoint entries (the posterior encoder `vits.enc_q.*`) are not
part of the inference model and are skipped when loading; every key the inference model owns must be present.
`aligner=True` builds the posterior encoder for `VITS.align` (forced alignment): its entries are then the model's own and load.
"""
import torch

from .engine import Voice
from .mel import reference_mel_prompt
from .model3 import VITS, NaturalSpeech2

# reference state-dict entries that only training uses: the posterior encoder (model3.py:704-712; infer never calls it).  A model
# built with aligner=True owns them, so they are loaded like any other entry
TRAINING_ONLY_PREFIXES = ("vits.enc_q.",)


def build_model(cfg, n_vocab, backend=None, text_encoder_backend=None, prior_backend=None, aligner=False, posterior_backend=None):
    """NaturalSpeech2(cfg) as model3.py:955-975 builds it: VITS(len(symbols), window_size // 2 + 1, **cfg['vits']).
    aligner=True: with the posterior encoder `vits.enc_q` (VITS.align), whose checkpoint entries load_state then loads;
    posterior_backend='hip' (opt-in) runs it on the native posterior-encoder engine."""
    vits = VITS(n_vocab, cfg["data"]["window_size"] // 2 + 1, backend=backend, text_encoder_backend=text_encoder_backend,
                prior_backend=prior_backend, aligner=aligner, posterior_backend=posterior_backend, **cfg["vits"])
    return NaturalSpeech2(cfg, vits=vits, backend=backend)


def load_state(model, state_dict):
    """load_state_dict that tolerates the training-only entries and nothing else.  Returns the skipped keys."""
    own = model.state_dict()
    skipped = [k for k in state_dict if k not in own]
    bad = [k for k in skipped if not k.startswith(TRAINING_ONLY_PREFIXES)]
    if bad:
        raise RuntimeError("checkpoint entries unknown to the inference model: %s" % ", ".join(sorted(bad)[:8]))
    missing = [k for k in own if k not in state_dict]
    if missing:
        raise RuntimeError("checkpoint lacks %d entries of the inference model, e.g. %s" % (len(missing), ", ".join(missing[:8])))
    model.load_state_dict({k: v for k, v in state_dict.items() if k in own})
    return skipped


def load_model(model_path, device, cfg, n_vocab=None, backend=None, aligner=False, posterior_backend=None):
    """tts_infer.py:76-81: torch.load -> NaturalSpeech2(cfg) -> load_state_dict(data['model']) -> .to(device).eval()."""
    data = torch.load(model_path, map_location="cpu", weights_only=True)
    if not isinstance(data, dict) or "model" not in data:
        raise ValueError("%s is not a {'step', 'model'} checkpoint (model3.py:1326-1333)" % (model_path,))
    sd = data["model"]
    if n_vocab is None:
        if "vits.enc_p.emb.weight" not in sd:
            raise ValueError("checkpoint has no vits.enc_p.emb.weight; pass n_vocab")
        n_vocab = sd["vits.enc_p.emb.weight"].shape[0]
    model = build_model(cfg, n_vocab, backend=backend, aligner=aligner, posterior_backend=posterior_backend)
    load_state(model, sd)
    return model.to(device).eval()


def load_vocoder(path, backend=None, precision="bf16x3"):
    """A torch-saved Vocos state dict (the published names: vocoder.state_dict_names) -> `vocoder.Vocoder`, the object `sample`,
    `sample_from_prior` and `synthesize` take as `vocos`.  A missing or unknown key is refused (feature_extractor.* is accepted
    and ignored).  There is no from_pretrained and no network."""
    from .vocoder import Vocoder
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(sd, dict) and "state_dict" in sd and "head.out.weight" not in sd:
        sd = sd["state_dict"]
    if not isinstance(sd, dict):
        raise ValueError("%s is not a state dict" % (path,))
    return Vocoder.from_state_dict(sd, backend=backend, precision=precision)


def save_checkpoint(model, step, path):
    """The reference trainer's format (model3.py:1326-1333): {'step': int, 'model': state_dict}."""
    torch.save({"step": int(step), "model": model.state_dict()}, str(path))


def refer_prompt(refer, device, mel_backend=None, audio_backend=None, sample_rate=None, resample_backend=None):
    """Reference audio -> log-mel prompt [1, 100, L] (tts_infer.py:54-67).  `refer`: path, waveform [1, n] at 24 kHz,
    or an already computed log-mel [1, 100, L].  mel_backend='hip' (opt-in): the native front-end (mel.py), one launch.
    audio_backend='native' (opt-in): a path is decoded by audio.read_wav and converted from the file's rate to 24 kHz by
    audio.Resample; the default needs torchaudio, as the reference does.  sample_rate: the rate of a waveform tensor (None: 24 kHz).
    resample_backend='hip' (opt-in): the conversion on the native kernel (audio.py) - with mel_backend='hip' the route is upload,
    k_resample, k_log_mel."""
    if audio_backend not in (None, "native"):
        raise ValueError("audio_backend must be None or 'native'")
    if isinstance(refer, (str, bytes)) or hasattr(refer, "__fspath__"):
        if audio_backend == "native":
            from .audio import read_wav
            refer, sample_rate = read_wav(refer)
        else:
            try:
                import torchaudio
                import torchaudio.transforms as T
            except ImportError as e:
                raise ImportError("decoding a reference audio file needs torchaudio (as tts_infer.py:54-55); pass a 24 kHz "
                                  "waveform tensor or a log-mel prompt instead") from e
            audio, sr = torchaudio.load(refer)
            refer = T.Resample(sr, 24000)(audio)
            sample_rate = None
    refer = torch.as_tensor(refer)
    if refer.dim() == 3:
        return refer.to(device=device, dtype=torch.float32)
    if refer.dim() != 2:
        raise ValueError("reference audio must be [channels, samples] or a log-mel [1, 100, L], got %s" % (tuple(refer.shape),))
    refer = refer.to(device=device, dtype=torch.float32)
    if sample_rate is not None and int(sample_rate) != 24000:
        from .audio import Resample
        refer = Resample(int(sample_rate), 24000, backend=resample_backend)(refer)
    return reference_mel_prompt(refer, backend=mel_backend)


def recording_mels(waves, n_samples, device, mel_backend=None, sample_rates=None, resample_backend=None):
    """A batch of recordings -> (y, y_lengths) for `VITS.align(..., y, y_lengths, ...)` and `NaturalSpeech2.enroll_voice`:
    waves [B, n_max] at 24 kHz (zero padded, or any content behind each row's samples), n_samples [B] -> the log-mel
    y [B, 100, 1 + n_max // 256] with zeros behind every row's own frames, and y_lengths int64 [B] = 1 + n_samples // 256.
    Every row is the mel of its own recording alone (reflect padding about its own end), on either backend;
    mel_backend='hip' computes the batch in one launch.
    sample_rates (opt-in): the recordings' rate, one for the batch or one per row; every row is first converted to 24 kHz from its own
    samples alone (audio.Resample), and n_max / n_samples above then read as the converted widths.  resample_backend='hip': that
    conversion in one launch, its lengths handed to the mel kernel on the device."""
    waves = torch.as_tensor(waves).to(device=device, dtype=torch.float32)
    n_samples = torch.as_tensor(n_samples).to(device=device, dtype=torch.int64)
    if sample_rates is not None:
        from .audio import Resample
        waves, n_samples = Resample(sample_rates, 24000, backend=resample_backend)(waves, n_samples)
    return reference_mel_prompt(waves, lengths=n_samples, backend=mel_backend)


def save_wav(path, samples, out_rate=None, resample_backend=None, bits=16):
    """Write what `sample` / `synthesize` return (24 kHz audio [B, n] - every row a channel of the file - or [n]) as a WAVE file
    (audio.write_wav: PCM 16, or float32 with bits=32).  out_rate: convert from 24 kHz first (audio.Resample);
    resample_backend='hip': on the native kernel (the samples go to the GPU and back)."""
    from .audio import Resample, write_wav
    x = torch.as_tensor(samples).detach().to(torch.float32)
    if x.dim() == 1:
        x = x[None, :]
    rate = 24000
    if out_rate is not None and int(out_rate) != 24000:
        if resample_backend == "hip":
            x = x.cuda()
        x = Resample(24000, int(out_rate), backend=resample_backend)(x)
        rate = int(out_rate)
    write_wav(path, x.cpu(), rate, bits=bits)


def synthesize(model, cfg, vocos, batchs, control_values=None, device="cuda", prompt_length="reference", mel_backend=None,
               **sample_kw):
    """tts_infer.py:46-75 with the same batch tuples `(phoneme, tone, language, refer, phoneme_length)`; returns the last
    batch's samples like the reference (and its mel as a second value).  `control_values` is accepted and, as in the
    reference, unused.  Extra keywords (`sample_method`, `noise`, `prior_noise`, `known_mel` / `known_mask` / `known_noise` /
    `paste_known` for infilling, ...) go to `model.sample`; `mel_backend` goes to `refer_prompt`.

    prompt_length: tts_infer.py:68 passes `refer.size(1)` - the mel CHANNEL count, 100 - as the prompt length, so the
    prompt masks cover the first 100 frames whatever the audio's length.  "reference" keeps that; "frames" passes the
    real frame count `refer.size(2)`.

    A batch tuple's `refer` may also be an enrolled `Voice` (`model.enroll_voice`): the diffusion side then binds the voice
    instead of encoding the prompt again; the prior still reads the mel prompt and the length the voice was enrolled with
    (`voice.refer`, `voice.refer_length`)."""
    if prompt_length not in ("reference", "frames"):
        raise ValueError("prompt_length must be 'reference' or 'frames'")
    samples = mel = None
    for phoneme, tone, language, refer, phoneme_length in batchs:
        phoneme, tone, language = phoneme.to(device), tone.to(device), language.to(device)
        phoneme_length = torch.as_tensor(phoneme_length, dtype=torch.long).to(device)
        if isinstance(refer, Voice):
            if refer.refer is None:
                raise ValueError("a Voice in a batch tuple must carry its mel prompt (enrol it with model.enroll_voice): the prior reads it")
            spec, refer_length = refer.refer.to(device), refer.refer_length.to(device)
            kw = dict(sample_kw, voices=[refer])
        else:
            spec = refer_prompt(refer, device, mel_backend=mel_backend)
            refer_length = torch.tensor([spec.size(1) if prompt_length == "reference" else spec.size(2)]).to(device)
            kw = sample_kw
        with torch.no_grad():
            samples, mel = model.sample(phoneme, spec, phoneme_length, refer_length, tone, language, vocos, **kw)
        samples = samples.detach().cpu()
    return samples, mel
