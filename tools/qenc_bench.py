"""Posterior encoder: the native engine (dv_qenc_*, one k_wn_layer launch per WaveNet layer) against the torch ops of the same
build on the same GPU, at the aligner's own sizes.  One process, HIP events around 50 calls after 10 warm-up calls.  Writes
profiles/qenc_bench.txt:  python tools/qenc_bench.py"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import diff_vits_amd  # noqa: E402,F401  (registers the package under its import name)
from diff_vits_amd import _lib  # noqa: E402
from diff_vits_amd.model3 import VITS  # noqa: E402

SIZES = ((1, 100, 265), (16, 150, 1047))          # B, Tx, Ty: profiles/align_bench.txt
PEAK_BF16_DENSE = 2.5e15                           # MI355X bf16 MFMA peak, FLOP/s; the bf16x3 contraction spends three products per FLOP
N_VOCAB = 108


def timed(fn, warm=10, reps=50):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / reps


def main():
    torch.manual_seed(0)
    dev = "cuda"
    native = VITS(N_VOCAB, 513, aligner=True, posterior_backend="hip", text_encoder_backend="hip").to(dev).eval()
    plain = VITS(N_VOCAB, 513, aligner=True, text_encoder_backend="hip").to(dev).eval()
    plain.load_state_dict(native.state_dict())
    lines = ["posterior encoder, %s, build %s; HIP events around 50 calls after 10 warm-up calls, microseconds per call"
             % (torch.cuda.get_device_name(0), _lib.lib().dv_version().decode())]
    with torch.no_grad():
        for B, Tx, Ty in SIZES:
            y = torch.randn(B, 100, Ty, device=dev)
            yl = torch.full((B,), Ty, device=dev, dtype=torch.int64)
            x = torch.randint(0, N_VOCAB, (B, Tx), device=dev)
            xl = torch.full((B,), Tx, device=dev, dtype=torch.int64)
            tone, lang = torch.zeros_like(x), torch.zeros_like(x)
            g = torch.randn(B, 256, 1, device=dev)
            noise = torch.randn(B, 128, Ty, device=dev)
            t_nat = timed(lambda: native.enc_q(y, yl, g, noise=noise))
            t_tor = timed(lambda: plain.enc_q(y, yl, g, noise=noise))
            a_nat = timed(lambda: native.align(x, xl, y, yl, tone, lang, noise=noise, align_backend="hip"))
            a_tor = timed(lambda: plain.align(x, xl, y, yl, tone, lang, noise=noise, align_backend="hip"))
            native.enc_q(y, yl, g, noise=noise)
            eng = native.enc_q.hip_engine()
            eng.time_layers(10)
            t_layers = eng.time_layers(50)
            n_launch, flops = eng.stats()
            H, L, M = 256, 16, B * Ty
            layer_flops = 2.0 * M * (5 * H * 2 * H + H * 2 * H) * (L - 1) + 2.0 * M * (5 * H * 2 * H + H * H)
            lines += ["B = %d, Tx = %d, Ty = %d:" % (B, Tx, Ty),
                      "  posterior encoder, native         %9.1f   (%d launches, %.2f GFLOP)" % (t_nat, n_launch, flops / 1e9),
                      "  posterior encoder, torch ops      %9.1f   (x%.2f)" % (t_tor, t_tor / t_nat),
                      "  align, native posterior encoder   %9.1f" % a_nat,
                      "  align, torch posterior encoder    %9.1f   (x%.2f)" % (a_tor, a_tor / a_nat),
                      "  k_wn_layer alone, %d launches         %9.1f   (%.1f per layer; events around the layers of one forward, replayed 50 times)"
                      % (L, t_layers, t_layers / L),
                      "  k_wn_layer: %.1f %% of the bf16x3 MFMA peak (%.2f GFLOP x 3 products in that time, peak %.1f PFLOP/s bf16)"
                      % (100.0 * 3 * layer_flops / (t_layers * 1e-6) / PEAK_BF16_DENSE, layer_flops / 1e9, PEAK_BF16_DENSE / 1e15),
                      "  native %s the torch route" % ("is not slower than" if t_nat <= t_tor else "IS SLOWER than")]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(os.path.join(ROOT, "profiles", "qenc_bench.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
