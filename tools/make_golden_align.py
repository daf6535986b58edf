#!/usr/bin/env python3
"""Generate tests/golden/align_forward.npz by stub-IMPORTING the reference's model3.VITS and monotonic_align (build container
only): the posterior encoder, the alignment scores and the monotonic alignment search of the reference's training forward
(model3.py:755-798) on a small ragged case, with the seeded synthetic weights of synth.py in ref_enc / enc_p / enc_q and a fixed
posterior noise.

The absent third-party packages are stubbed as in make_golden_prompt.py.  numba is absent too: numba.jit passes through as the
identity decorator - the body of the search routine is plain Python over numpy arrays, and the float32 element it accumulates into
rounds every sum exactly as the compiled routine's add-in-double-store-float32 does.  Only inputs, shapes, names and outputs are
stored, never reference text.
Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_align.py [--ref /root/reference]
"""
import argparse
import os
import sys
from unittest.mock import MagicMock

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import diff_vits_amd  # noqa: E402,F401
from diff_vits_amd import synth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
B, TX, TY = 2, 12, 40
X_LENGTHS, Y_LENGTHS = [12, 9], [40, 31]
PROJ_GAIN = 16.0


def import_reference(ref):
    import accelerate  # noqa: F401  (real, must be imported before the stubs)
    for m in ("vocos", "torchaudio", "torchaudio.transforms", "ema_pytorch", "numba", "librosa",
              "torch.utils.tensorboard", "matplotlib", "matplotlib.pyplot"):
        if m not in sys.modules:
            try:
                __import__(m)
            except Exception:
                sys.modules[m] = MagicMock()
    if isinstance(sys.modules["numba"], MagicMock):
        sys.modules["numba"].jit = lambda *a, **k: (lambda f: f)
    sys.path.insert(0, ref)
    import monotonic_align          # the reference's own package, now importable
    import model3
    return model3, monotonic_align


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    import json
    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    model3, monotonic_align = import_reference(args.ref)
    cfg = json.load(open(os.path.join(args.ref, "config.json")))
    v = model3.NaturalSpeech2(cfg).eval().vits
    # the trainer's exploration noise on the scores (model3.py:781-787, switched on by the config) is no part of an alignment:
    # the fixture holds the scores of model3.py:767-780 and the search on exactly those
    v.use_noise_scaled_mas = False
    shapes = {k: tuple(t.shape) for k, t in v.state_dict().items() if k.split(".")[0] in ("ref_enc", "enc_p", "enc_q")}
    sd = synth.make_state_dict(shapes, seed=1234)
    # seeded weights give every token nearly the same statistics (|m_p| ~ 0.04, logs_p ~ 0): an alignment of near-ties.  A trained
    # prior separates its tokens; the gain on the text encoder's output projection does that here, so that no decision of the
    # fixture's path is within rounding of a tie (checked in tests/test_align_cpu.py).  The tests apply the same gain.
    for k in ("enc_p.proj.weight", "enc_p.proj.bias"):
        sd[k] = (sd[k] * np.float32(PROJ_GAIN)).astype(np.float32)
    missing = v.load_state_dict({k: torch.from_numpy(t) for k, t in sd.items()}, strict=False)
    assert not missing.unexpected_keys
    n_sym = v.enc_p.emb.weight.shape[0]
    n_tones, n_lang = v.enc_p.tone_emb.weight.shape[0], v.enc_p.language_emb.weight.shape[0]
    text = torch.from_numpy((synth.uniform(1234, "align.text", (B, TX)) * 0.5 + 0.5) * (n_sym - 1)).long()
    tone = torch.from_numpy((synth.uniform(1234, "align.tone", (B, TX)) * 0.5 + 0.5) * (n_tones - 1)).long()
    lang = torch.from_numpy((synth.uniform(1234, "align.lang", (B, TX)) * 0.5 + 0.5) * (n_lang - 1)).long()
    y = torch.from_numpy(synth.normal(1234, "align.mel", (B, 100, TY)))
    x_lengths, y_lengths = torch.tensor(X_LENGTHS), torch.tensor(Y_LENGTHS)

    captured = {}
    enc_q_forward, enc_p_forward, real_path = v.enc_q.forward, v.enc_p.forward, model3.monotonic_align.maximum_path

    def enc_q_hook(*a, **k):
        out = enc_q_forward(*a, **k)
        captured["q"] = [t.clone() for t in out]
        return out

    def enc_p_hook(*a, **k):
        out = enc_p_forward(*a, **k)
        captured["p"] = [t.clone() for t in out]
        return out

    def path_hook(neg_cent, mask):
        captured["neg_cent"] = neg_cent.clone()
        captured["path"] = real_path(neg_cent, mask)
        return captured["path"]

    real_like = torch.randn_like
    torch.randn_like = lambda t, **k: torch.from_numpy(synth.normal(1234, "align.noise", tuple(t.shape))).to(t.dtype)
    v.enc_q.forward, v.enc_p.forward, model3.monotonic_align.maximum_path = enc_q_hook, enc_p_hook, path_hook
    try:
        v.forward(text, x_lengths, y, y_lengths, tone, lang)
    finally:
        torch.randn_like = real_like
        v.enc_q.forward, v.enc_p.forward, model3.monotonic_align.maximum_path = enc_q_forward, enc_p_forward, real_path
    z, m_q, logs_q, _ = captured["q"]
    _, m_p, logs_p, _ = captured["p"]
    path = captured["path"]                                   # [B, Ty, Tx]
    w = path.sum(1)                                           # frames per token (reference: attn.sum(2) on [b, 1, t_y, t_x])
    print("align  frames per token:", w.long().tolist())
    names = sorted(shapes)
    np.savez_compressed(
        os.path.join(GOLD, "align_forward.npz"), text=text.numpy(), tone=tone.numpy(), language=lang.numpy(),
        x_lengths=x_lengths.numpy(), y_lengths=y_lengths.numpy(), Ty=TY, proj_gain=PROJ_GAIN, n_vocab=n_sym, n_tones=n_tones, n_languages=n_lang,
        vits_kwargs=np.array(repr(cfg["vits"])), names=np.array(names), shapes=np.array([repr(shapes[k]) for k in names]),
        z=z.numpy(), m_q=m_q.numpy(), logs_q=logs_q.numpy(), m_p=m_p.numpy(), logs_p=logs_p.numpy(),
        neg_cent=captured["neg_cent"].numpy(), path=path.numpy().astype(np.int8), w=w.numpy().astype(np.int64))


if __name__ == "__main__":
    main()
