#!/usr/bin/env python3
"""What binding enrolled voices saves in front of the sampler graph: the per-utterance conditioning of the diffusion side,

  encode + set_cond:  Diffusion_Encoder._conditioning (the 4-layer prompt encoder, dv_penc_*) + UNetEngine.set_cond (the whole
                      cond schedule: pooled-text embedding, the K / V projections and fragments of 16 blocks, the key bias)
  bind_voices:        UNetEngine.bind_voices - one k_voice_scatter launch

both on this build, in one process, at the production denoiser (synthetic weights), T = 1024, L = 256:
B = 1; B = 8 with all rows rebound; B = 8 with one row rebound (against the full B = 8 conditioning pass it would need today).
Each figure: --calls calls between one HIP event pair after --warmup untimed calls (device time of the stream, gaps between
launches included - the calls are back to back, so this is what an utterance pays), and the host's wall-clock time per call
to enqueue them.  Also the bytes of a voice record and the bind's achieved GB/s (record bytes x rows, read + written).
The process ends itself after --time-limit seconds.  One JSON line per case and a summary line.

Usage: python tools/voice_bench.py [--calls 50] [--warmup 10] [--time-limit 240]"""
import argparse
import json
import os
import signal
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--time-limit", type=int, default=240)
    args = ap.parse_args()
    signal.alarm(args.time_limit)
    import torch
    import diff_vits_amd  # noqa: F401
    from diff_vits_amd import _lib, synth
    from diff_vits_amd.model3 import Diffusion_Encoder

    kw = dict(in_channels=80, out_channels=80, hidden_channels=128, n_heads=8)
    with torch.device("meta"):
        shapes = {k: tuple(v.shape) for k, v in Diffusion_Encoder(backend="torch", **kw).state_dict().items()}
    dm = Diffusion_Encoder(backend="hip", **kw).eval()
    dm.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(shapes, seed=1234).items()})
    dm = dm.cuda()
    unet = dm.unet
    eng = unet.hip_engine("bf16x3")
    T, L = 1024, 256
    n = args.warmup + args.calls

    def timed(fn):
        """(device ms per call, host ms per call to enqueue) of fn(i), i = warmup .. warmup + calls - 1."""
        for i in range(args.warmup):
            fn(i)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for i in range(args.warmup, n):
            fn(i)
        e1.record()
        host = 1e3 * (time.perf_counter() - t0)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.calls, host / args.calls

    rows_out = []
    with torch.no_grad():
        for B, rebound in ((1, 1), (8, 8), (8, 1)):
            lengths = torch.tensor([L - 13 * b for b in range(B)], dtype=torch.long).cuda()
            base = torch.from_numpy(synth.normal(4321, "voice_bench.prompt", (B, 100, L))).cuda()
            prompts = [base.clone() for _ in range(n)]            # new tensor objects: _conditioning's one-entry cache never hits
            eng.prepare(B, T, L)

            def encode_set_cond(i):
                enc, mask = dm._conditioning(prompts[i], lengths, torch.float32)
                eng.set_cond(enc, unet._bias_from_mask(mask, torch.float32))

            dev_ref, host_ref = timed(encode_set_cond)
            enc, mask = dm._conditioning(base, lengths, torch.float32)
            voices = eng.enroll(enc, unet._bias_from_mask(mask, torch.float32))
            rows = list(range(rebound))
            dev_bind, host_bind = timed(lambda i: eng.bind_voices(rows, voices[:rebound]))
            assert all(v.rebuilds == 0 for v in voices)
            rec = voices[0].nbytes
            out = dict(B=B, T=T, L=L, rows_rebound=rebound, calls=args.calls, warmup=args.warmup,
                       encode_set_cond_ms=round(dev_ref, 4), encode_set_cond_host_ms=round(host_ref, 4),
                       bind_voices_ms=round(dev_bind, 4), bind_voices_host_ms=round(host_bind, 4),
                       record_bytes=rec, bind_GBps=round(2.0 * rec * rebound / (dev_bind * 1e-3) / 1e9, 1),
                       saved_ms=round(dev_ref - dev_bind, 4), bind_not_slower=bool(dev_bind <= dev_ref))
            rows_out.append(out)
            print(json.dumps(out), flush=True)
    print(json.dumps(dict(library=_lib.lib().dv_version().decode(), device=torch.cuda.get_device_name(0),
                          all_rows_bind_not_slower=all(r["bind_not_slower"] for r in rows_out if r["rows_rebound"] == r["B"]))), flush=True)


if __name__ == "__main__":
    main()
