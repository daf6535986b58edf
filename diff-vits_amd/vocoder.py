"""Native vocoder: the Vocos ConvNeXt-1D backbone and ISTFT head (the published `charactr/vocos-mel-24khz` model), the stage
behind `NaturalSpeech2.sample`'s mel - the object `sample`, `sample_from_prior` and `tts_infer.synthesize` take as `vocos`.

PARITY: neither the `vocos` package nor a checkpoint is installed in the build container or on the GPU box.  The architecture
and the state-dict names below are written from the published source and are NOT checked against it; the kernels are pinned to
the fp64 restatement of that definition (tests/vocoder_cases.py).  The name table lives in ONE place (`state_dict_names`): a
wrong key costs a one-line fix.

The model: mel [B, n_mels, T] -> embed Conv1d(k 7, pad 3) -> LayerNorm(eps 1e-6) -> n_layers x [dwconv(k 7, groups C) ->
LayerNorm -> Linear(C, I) -> exact-erf GELU -> Linear(I, C) -> x gamma -> + residual] -> LayerNorm -> Linear(C, n_fft + 2) ->
S = min(exp(m), 1e2) (cos p + i sin p) -> torch.istft(n_fft 1024, hop 256, periodic Hann, center) -> (T - 1) * 256 samples.

Ragged batches: with `lengths` [B] every row is its own utterance of L_b frames - a filter tap reads zeros at t < 0 and
t >= L_b, the overlap-add and its envelope use L_b frames, row b holds n_b = (L_b - 1) * hop samples followed by exact zeros and
samples[b] = n_b; a row with L_b < 2 or L_b > T is all zeros with samples[b] = 0.  So row b equals decode(mel[b:b+1, :, :L_b]).
lengths=None: every row has T frames (what the reference's `vocos.decode` computes).

Two backends.  "torch": the eager restatement in the tensor's dtype.  "hip": the native engine (csrc/voc.hip, dv_voc_*); GPU
tensors only, never a fall-back.
"""
import ctypes as C

import torch
import torch.nn.functional as F

DEFAULT_CFG = dict(n_mels=100, dim=512, intermediate=1536, n_layers=8, n_fft=1024, hop=256)
IGNORED_PREFIXES = ("feature_extractor.",)


def state_dict_names(cfg):
    """name -> shape of every entry of the published state dict that the vocoder reads.  THE name table."""
    C_, I, M, N = cfg["dim"], cfg["intermediate"], cfg["n_mels"], cfg["n_fft"]
    names = {"backbone.embed.weight": (C_, M, 7), "backbone.embed.bias": (C_,),
             "backbone.norm.weight": (C_,), "backbone.norm.bias": (C_,),
             "backbone.final_layer_norm.weight": (C_,), "backbone.final_layer_norm.bias": (C_,),
             "head.out.weight": (N + 2, C_), "head.out.bias": (N + 2,), "head.istft.window": (N,)}
    for i in range(cfg["n_layers"]):
        p = "backbone.convnext.%d." % i
        names.update({p + "dwconv.weight": (C_, 1, 7), p + "dwconv.bias": (C_,), p + "norm.weight": (C_,), p + "norm.bias": (C_,),
                      p + "pwconv1.weight": (I, C_), p + "pwconv1.bias": (I,), p + "pwconv2.weight": (C_, I), p + "pwconv2.bias": (C_,),
                      p + "gamma": (C_,)})
    return names


def cfg_from_state_dict(sd):
    """The configuration a published state dict implies (its shapes; n_fft from the head, hop = n_fft / 4)."""
    try:
        C_, M, _ = sd["backbone.embed.weight"].shape
        I = sd["backbone.convnext.0.pwconv1.weight"].shape[0]
        n_fft = sd["head.out.weight"].shape[0] - 2
    except KeyError as e:
        raise RuntimeError("vocoder state dict lacks %s" % (e,)) from None
    L = 0
    while ("backbone.convnext.%d.gamma" % L) in sd:
        L += 1
    return dict(n_mels=int(M), dim=int(C_), intermediate=int(I), n_layers=L, n_fft=int(n_fft), hop=int(n_fft) // 4)


def check_state_dict(sd, cfg):
    """Refuses a missing or unknown key and a wrong shape, as tts_infer.load_state does; feature_extractor.* is accepted and
    ignored.  Returns the entries the vocoder reads."""
    names = state_dict_names(cfg)
    bad = sorted(k for k in sd if k not in names and not k.startswith(IGNORED_PREFIXES))
    if bad:
        raise RuntimeError("vocoder state dict entries unknown to the model: %s" % ", ".join(bad[:8]))
    missing = [k for k in names if k not in sd]
    if missing:
        raise RuntimeError("vocoder state dict lacks %d entries, e.g. %s" % (len(missing), ", ".join(missing[:8])))
    for k, shape in names.items():
        if tuple(sd[k].shape) != tuple(shape):
            raise RuntimeError("vocoder state dict entry %s has shape %s, expected %s" % (k, tuple(sd[k].shape), tuple(shape)))
    return {k: sd[k] for k in names}


def fold_gamma(W, b, gamma):
    """The layer scale folded into pwconv2: W'[n, :] = gamma[n] W[n, :], b' = gamma b."""
    return gamma[:, None] * W, gamma * b


def istft_rows(S, window, n_fft=1024, hop=256):
    """The hand-written form of torch.istft(center=True) for ONE utterance: S complex [n_fft / 2 + 1, L] -> [(L - 1) * hop]:
    inverse real FFT per frame, times the window, overlap-add, trim n_fft / 2 at both ends, divide by the overlap-added squared
    window of the same L frames."""
    L = S.shape[-1]
    frames = torch.fft.irfft(S.transpose(0, 1), n=n_fft, dim=-1) * window             # [L, n_fft]
    total = n_fft + (L - 1) * hop
    y = frames.new_zeros(total)
    env = frames.new_zeros(total)
    w2 = window * window
    for f in range(L):
        y[f * hop:f * hop + n_fft] += frames[f]
        env[f * hop:f * hop + n_fft] += w2
    lo, hi = n_fft // 2, n_fft // 2 + (L - 1) * hop
    return y[lo:hi] / env[lo:hi]


def decode_rows(sd, cfg, mel, lengths=None):
    """The eager restatement in mel's dtype: (wave [B, (T - 1) * hop], samples int64 [B]) with the per-utterance rule."""
    B, _, T = mel.shape
    hop, n_fft, L = cfg["hop"], cfg["n_fft"], cfg["n_layers"]
    W = {k: v.to(device=mel.device, dtype=mel.dtype) for k, v in sd.items()}
    n = [T] * B if lengths is None else [int(v) for v in torch.as_tensor(lengths).tolist()]
    wave = mel.new_zeros(B, max(T - 1, 0) * hop)
    samples = torch.zeros(B, dtype=torch.int64, device=mel.device)
    C_ = cfg["dim"]
    for nb in sorted({v for v in n if 2 <= v <= T}):          # rows of one length are one batch: each still sees its own frames only
        rows = [b for b in range(B) if n[b] == nb]
        x = F.conv1d(mel[rows, :, :nb], W["backbone.embed.weight"], W["backbone.embed.bias"], padding=3)
        x = F.layer_norm(x.transpose(1, 2), (C_,), W["backbone.norm.weight"], W["backbone.norm.bias"], 1e-6).transpose(1, 2)
        for i in range(L):
            p = "backbone.convnext.%d." % i
            r = x
            x = F.conv1d(x, W[p + "dwconv.weight"], W[p + "dwconv.bias"], padding=3, groups=C_).transpose(1, 2)
            x = F.layer_norm(x, (C_,), W[p + "norm.weight"], W[p + "norm.bias"], 1e-6)
            x = F.linear(F.gelu(F.linear(x, W[p + "pwconv1.weight"], W[p + "pwconv1.bias"])), W[p + "pwconv2.weight"], W[p + "pwconv2.bias"])
            x = r + (W[p + "gamma"] * x).transpose(1, 2)
        x = F.layer_norm(x.transpose(1, 2), (C_,), W["backbone.final_layer_norm.weight"], W["backbone.final_layer_norm.bias"], 1e-6)
        o = F.linear(x, W["head.out.weight"], W["head.out.bias"]).transpose(1, 2)                # [rows, n_fft + 2, L_b]
        m, ph = o[:, :n_fft // 2 + 1], o[:, n_fft // 2 + 1:]
        mag = torch.clip(torch.exp(m), max=1e2)
        S = torch.complex(mag * torch.cos(ph), mag * torch.sin(ph))
        y = torch.istft(S, n_fft, hop_length=hop, win_length=n_fft, window=W["head.istft.window"], center=True)
        wave[rows, :y.shape[1]] = y
        samples[rows] = y.shape[1]
    return wave, samples


class _VocHandle:
    """Owner of a dv_voc handle."""

    def __init__(self, h):
        self.h = h
        self.prepared = None

    def __del__(self):
        try:
            from . import _lib
            _lib.lib().dv_voc_destroy(self.h)
        except Exception:
            pass


class Vocoder:
    """Vocoder(cfg=None, backend=None): cfg defaults to the published model's; backend "hip" (the default on a build with the
    library) or "torch".  Weights come from `from_state_dict` / `load_state_dict`."""

    def __init__(self, cfg=None, backend=None, precision="bf16x3"):
        if backend not in (None, "hip", "torch"):
            raise ValueError("backend must be None, 'hip' or 'torch'")
        if precision not in ("bf16x3", "bf16"):
            raise ValueError("precision must be 'bf16x3' or 'bf16'")
        self.cfg = dict(DEFAULT_CFG, **(cfg or {}))
        unknown = sorted(set(self.cfg) - set(DEFAULT_CFG))
        if unknown:
            raise ValueError("unknown vocoder cfg entries: %s" % ", ".join(unknown))
        if (self.cfg["n_fft"], self.cfg["hop"]) != (1024, 256):
            raise ValueError("n_fft = %d, hop = %d: only 1024 / 256 are supported" % (self.cfg["n_fft"], self.cfg["hop"]))
        self.backend = backend or "hip"
        self.precision = precision
        self.sd = None
        self._hip = None
        self._dev_sd = None

    @classmethod
    def from_state_dict(cls, sd, backend=None, cfg=None, precision="bf16x3"):
        v = cls(cfg if cfg is not None else cfg_from_state_dict(sd), backend=backend, precision=precision)
        v.load_state_dict(sd)
        return v

    def load_state_dict(self, sd):
        own = check_state_dict(sd, self.cfg)
        self.sd = {k: t.detach().to(torch.float32).contiguous() for k, t in own.items()}
        self._hip = None
        self._dev_sd = None
        return self

    def state_dict(self):
        return dict(self.sd)

    def to(self, device):
        if self.sd is None:
            raise RuntimeError("the vocoder has no weights (from_state_dict / load_state_dict)")
        device = torch.device(device)
        if next(iter(self.sd.values())).device != device:
            self.sd = {k: t.to(device) for k, t in self.sd.items()}
            self._hip = None
            self._dev_sd = None
        return self

    def eval(self):
        return self

    # ---- decode ----
    @torch.no_grad()
    def decode(self, mel, lengths=None):
        """mel [B, n_mels, T] -> wave [B, (T - 1) * hop]."""
        return self.decode_with_lengths(mel, lengths)[0]

    @torch.no_grad()
    def decode_with_lengths(self, mel, lengths=None):
        """-> (wave [B, (T - 1) * hop], samples int64 [B])."""
        if self.sd is None:
            raise RuntimeError("the vocoder has no weights (from_state_dict / load_state_dict)")
        if mel.dim() != 3 or mel.shape[1] != self.cfg["n_mels"]:
            raise ValueError("mel must be [B, %d, T], got %s" % (self.cfg["n_mels"], tuple(mel.shape)))
        if lengths is not None:
            lengths = torch.as_tensor(lengths)
            if lengths.dtype not in (torch.int64, torch.int32) or tuple(lengths.shape) != (mel.shape[0],):
                raise ValueError("lengths must be an integer tensor [B]")
        if self.backend == "torch":
            return decode_rows(self.sd, self.cfg, mel, lengths)
        return self._decode_hip(mel, lengths)

    def hip_engine(self, device):
        """The dv_voc handle with this object's weights on `device` (built once)."""
        from . import _lib
        if self._hip is None:
            L = _lib.lib()
            c = _lib.VocCfg(*(self.cfg[k] for k in ("n_mels", "dim", "intermediate", "n_layers", "n_fft", "hop")))
            h = C.c_void_p()
            _lib.check(L.dv_voc_create(C.byref(c), C.byref(h)), "dv_voc_create")
            self._hip = _VocHandle(h)
            self._dev_sd = {k: t.to(device=device, dtype=torch.float32).contiguous() for k, t in self.sd.items()}
            for k, t in self._dev_sd.items():
                shape = (C.c_int64 * t.dim())(*t.shape)
                _lib.check(L.dv_voc_set_weight(h, k.encode(), _lib.ptr(t), shape, t.dim()), "dv_voc_set_weight(%s)" % k)
            torch.cuda.synchronize(device)
        return self._hip

    def prepare(self, B, T, device):
        from . import _lib
        eng = self.hip_engine(device)
        prec = _lib.PREC_BF16X3 if self.precision == "bf16x3" else _lib.PREC_BF16
        if eng.prepared != (B, T, prec):
            _lib.check(_lib.lib().dv_voc_prepare(eng.h, B, T, prec), "dv_voc_prepare")
            eng.prepared = (B, T, prec)
        return eng

    def _decode_hip(self, mel, lengths):
        from . import _lib
        if not mel.is_cuda:
            raise RuntimeError("vocoder backend='hip' needs GPU tensors; got mel on %s (there is no fall-back)" % mel.device)
        if lengths is not None:
            if not lengths.is_cuda:
                raise RuntimeError("vocoder backend='hip' needs GPU tensors; got lengths on %s" % lengths.device)
            lengths = lengths.to(torch.int64).contiguous()
        B, _, T = mel.shape
        mel32 = mel.detach().to(torch.float32).contiguous()
        with torch.cuda.device(mel.device):
            eng = self.prepare(B, T, mel.device)
            wave = torch.empty((B, (T - 1) * self.cfg["hop"]), device=mel.device, dtype=torch.float32)
            samples = torch.empty((B,), device=mel.device, dtype=torch.int64)
            _lib.check(_lib.lib().dv_voc_forward(eng.h, _lib.ptr(mel32), _lib.ptr(lengths), _lib.ptr(wave), _lib.ptr(samples),
                                                 _lib.stream_ptr()), "dv_voc_forward")
        return wave.to(mel.dtype), samples

    def stats(self):
        """(launches per forward, FLOPs) of the prepared schedule."""
        from . import _lib
        n, fl = C.c_int64(), C.c_double()
        _lib.check(_lib.lib().dv_voc_stats(self._hip.h, C.byref(n), C.byref(fl)), "dv_voc_stats")
        return n.value, fl.value

    def probe(self, name):
        """A kept intermediate [B, T, C] of the last forward (prepared with DVITS_KEEP_INTERMEDIATES=1), as a CPU tensor."""
        from . import _lib
        L = _lib.lib()
        dims = (C.c_int64 * 3)()
        _lib.check(L.dv_voc_probe(self._hip.h, name.encode(), None, 0, dims), "dv_voc_probe")
        out = torch.empty(tuple(dims), dtype=torch.float32)
        _lib.check(L.dv_voc_probe(self._hip.h, name.encode(), _lib.ptr(out), out.numel(), dims), "dv_voc_probe")
        return out


def probe_names(n_layers):
    names = ["embed", "norm"]
    for i in range(n_layers):
        names += ["l%d.dwln" % i, "l%d.act" % i, "l%d.out" % i]
    return names + ["final", "head"]
