"""Mel front-end of the reference's inference script: `tts_infer.py:57-66` builds
`torchaudio.transforms.MelSpectrogram(sample_rate=24000, n_fft=1024, hop_length=256, n_mels=100, center=True, power=1)`
and feeds `log(clip(spec, 1e-7))` as the reference mel prompt `[B, 100, L]`.

PARITY: torchaudio is not installed in the build container or on the GPU box, so this restatement of its documented
defaults (Hann window, periodic; reflect padding; one-sided magnitude spectrum; HTK mel scale, no filter normalisation,
f_min 0, f_max sr/2) is still not compared with torchaudio OUTPUT.  It is pinned to the fp64 restatement of that
documented definition (tests/mel_cases.py: explicit reflect index map, explicit cos / sin DFT matrix;
profiles/mel_reference.txt, profiles/mel_parity.txt); tests/test_mel.py checks known-answer properties.

Two backends.  None: torch ops (torch.stft does the transform).  "hip" (opt-in): the native front-end
(csrc/kernels_mel.hip, dv_mel_*), a ragged batch of recordings in one launch; GPU float32 tensors only, never a
fall-back.  With `lengths` both backends return (mel, frames) and treat every row as the recording of its own length:
reflect padding about the row's own end, frames[b] = 1 + lengths[b] // hop, zeros at and behind frame frames[b].
`torch.stft` on a zero-padded batch reflects about the end of the BUFFER instead, which makes the last frames of every
row but the longest wrong; without `lengths` that (today's) behaviour is kept bit for bit.
"""
import math

import torch


def _hz_to_mel(f):
    return 2595.0 * math.log10(1.0 + f / 700.0)


def melscale_fbanks(n_freqs, f_min, f_max, n_mels, sample_rate):
    """Triangular HTK-scale filterbank [n_freqs, n_mels] (torchaudio.functional.melscale_fbanks, norm=None)."""
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs, dtype=torch.float64)
    m_pts = torch.linspace(_hz_to_mel(f_min), _hz_to_mel(f_max), n_mels + 2, dtype=torch.float64)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.clamp(torch.min(down, up), min=0.0).to(torch.float32)


class MelSpectrogram(torch.nn.Module):
    """`spec_process` of tts_infer.py:57-64 (torchaudio defaults otherwise): waveform [..., n] -> [..., n_mels, frames]."""

    def __init__(self, sample_rate=24000, n_fft=1024, hop_length=256, n_mels=100, center=True, power=1.0, f_min=0.0, f_max=None,
                 backend=None, log_clip=1e-7):
        super().__init__()
        if backend not in (None, "hip"):
            raise ValueError("backend must be None or 'hip'")
        self.n_fft, self.hop_length, self.center, self.power = n_fft, hop_length, center, power
        self.n_mels, self.backend, self.log_clip = n_mels, backend, float(log_clip)
        self._hip = None
        self.register_buffer("window", torch.hann_window(n_fft, periodic=True), persistent=False)
        self.register_buffer("fb", melscale_fbanks(n_fft // 2 + 1, f_min, f_max if f_max is not None else sample_rate / 2.0,
                                                  n_mels, sample_rate), persistent=False)

    def forward(self, waveform, lengths=None, validate=True, log=False):
        """lengths=None (and backend=None): the batch as one buffer, returns mel.  With `lengths` [B] (samples per row of a
        [B, n_max] batch): returns (mel [B, n_mels, 1 + n_max // hop], frames int64 [B]), each row computed from its own
        samples alone.  log=True (with lengths): log(clip(mel, log_clip)) on the valid frames, zeros behind them."""
        if self.backend == "hip":
            return self._forward_hip(waveform, lengths, validate, log)
        if lengths is not None:
            return self._forward_rows(waveform, lengths, validate, log)
        if log:
            raise ValueError("log=True needs lengths (reference_mel_prompt is the log form of a plain batch)")
        return self._forward_torch(waveform)

    def _forward_torch(self, waveform):
        shape = waveform.shape
        x = waveform.reshape(-1, shape[-1])
        spec = torch.stft(x, self.n_fft, hop_length=self.hop_length, win_length=self.n_fft, window=self.window.to(x),
                          center=self.center, pad_mode="reflect", normalized=False, onesided=True, return_complex=True).abs()
        if self.power != 1.0:
            spec = spec.pow(self.power)
        mel = torch.matmul(spec.transpose(-1, -2), self.fb.to(spec)).transpose(-1, -2)
        return mel.reshape(shape[:-1] + mel.shape[-2:])

    def check_lengths(self, waveform, lengths):
        """One host read: every n_b in [n_fft / 2 + 1, n_max] (reflect padding needs n_fft / 2 + 1 samples)."""
        n = [int(v) for v in lengths.tolist()]
        lo, hi = self.n_fft // 2 + 1, waveform.shape[-1]
        bad = [(b, v) for b, v in enumerate(n) if v < lo or v > hi]
        if bad:
            raise ValueError("lengths must be in [%d, %d] (n_fft / 2 + 1 .. the buffer's width); row %d has %d" % (lo, hi, bad[0][0], bad[0][1]))
        return n

    def _ragged_args(self, waveform, lengths):
        if waveform.dim() != 2:
            raise ValueError("with lengths the waveform must be [B, n_max], got %s" % (tuple(waveform.shape),))
        lengths = torch.as_tensor(lengths)
        if lengths.dtype not in (torch.int64, torch.int32) or lengths.shape != (waveform.shape[0],):
            raise ValueError("lengths must be an integer tensor [B]")
        return lengths

    def _forward_rows(self, waveform, lengths, validate, log):
        """The definition the native kernel is held to: every row on its own truncated waveform, zero filled."""
        lengths = self._ragged_args(waveform, lengths)
        n = self.check_lengths(waveform, lengths)          # the torch route needs the integers anyway
        B, n_max = waveform.shape
        out = waveform.new_zeros(B, self.n_mels, 1 + n_max // self.hop_length)
        for b in range(B):
            m = self._forward_torch(waveform[b:b + 1, :n[b]])[0]
            out[b, :, :m.shape[-1]] = torch.log(torch.clip(m, min=self.log_clip)) if log else m
        frames = torch.tensor([1 + v // self.hop_length for v in n], dtype=torch.int64, device=waveform.device)
        return out, frames

    def _forward_hip(self, waveform, lengths, validate, log):
        import ctypes as C

        from . import _lib
        if not (isinstance(waveform, torch.Tensor) and waveform.is_cuda and waveform.dtype == torch.float32):
            raise ValueError("backend='hip' needs a float32 GPU waveform (there is no fall-back)")
        if float(self.power) not in (1.0, 2.0):
            raise ValueError("backend='hip' computes power 1 or 2, not %r" % (self.power,))
        ragged = lengths is not None
        shape = waveform.shape
        x = (waveform if ragged else waveform.reshape(-1, shape[-1])).contiguous()
        if ragged:
            lengths = self._ragged_args(x, lengths)
            if not lengths.is_cuda or lengths.dtype != torch.int64:
                raise ValueError("backend='hip' needs int64 GPU lengths")
            if validate:
                self.check_lengths(x, lengths)
            lengths = lengths.contiguous()
        else:
            if shape[-1] < self.n_fft // 2 + 1:
                raise ValueError("reflect padding needs at least n_fft / 2 + 1 samples")
            lengths = torch.full((x.shape[0],), shape[-1], dtype=torch.int64, device=x.device)
        L = _lib.lib()
        if self._hip is None:
            cfg = _lib.MelCfg(self.n_fft, self.hop_length, self.n_mels, 1 if self.center else 0, self.log_clip)
            win = self.window.detach().to("cpu", torch.float32).contiguous()
            fb = self.fb.detach().to("cpu", torch.float32).contiguous()
            h = C.c_void_p()
            _lib.check(L.dv_mel_create(C.byref(cfg), _lib.ptr(win), _lib.ptr(fb), C.byref(h)), "dv_mel_create")
            self._hip = _MelHandle(h)
        B, n_max = x.shape
        L_max = 1 + n_max // self.hop_length
        out = torch.empty(B, self.n_mels, L_max, dtype=torch.float32, device=x.device)
        frames = torch.empty(B, dtype=torch.int64, device=x.device)
        flags = (_lib.MEL_LOG if log else 0) | (_lib.MEL_POWER2 if float(self.power) == 2.0 else 0)
        with torch.cuda.device(x.device):
            _lib.check(L.dv_mel_forward(self._hip.h, _lib.ptr(x), _lib.ptr(lengths), B, n_max, _lib.ptr(out), _lib.ptr(frames), L_max, flags,
                                        _lib.stream_ptr()), "dv_mel_forward")
        if ragged:
            return out, frames
        return out.reshape(shape[:-1] + out.shape[-2:])


class _MelHandle:
    """Owner of a dv_mel handle (the device tables of the native front-end)."""

    def __init__(self, h):
        self.h = h

    def __del__(self):
        try:
            from . import _lib
            _lib.lib().dv_mel_destroy(self.h)
        except Exception:
            pass


def reference_mel_prompt(waveform_24k, lengths=None, backend=None, **kw):
    """tts_infer.py:57-67: log(clip(MelSpectrogram(...)(refer_audio24k), min=1e-7)) -> the `refer` tensor [B, 100, L].
    With `lengths`: (log-mel [B, 100, L_max], frames [B]) of a ragged batch, zeros behind each row's frames.  backend='hip': the
    native front-end, the logarithm inside its launch."""
    if lengths is None and backend is None:
        m = MelSpectrogram(**kw).to(waveform_24k.device)
        return torch.log(torch.clip(m(waveform_24k), min=1e-7))
    m = MelSpectrogram(backend=backend, **kw).to(waveform_24k.device)
    if lengths is not None:
        return m(waveform_24k, lengths, log=True)
    shape = waveform_24k.shape
    x = waveform_24k.reshape(-1, shape[-1])
    n = torch.full((x.shape[0],), shape[-1], dtype=torch.int64, device=x.device)
    y, _ = m(x, n, log=True)
    return y.reshape(shape[:-1] + y.shape[-2:])
