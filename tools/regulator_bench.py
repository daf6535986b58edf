"""The length regulator of the prior alone - from logw, m_p, logs_p (and a given noise) to z_p - on the torch ops of
VITS.infer_from_encoder's default branch (the expression is copied here) against the native branch (VITS._regulate_hip:
dv_op_regulate_lengths, the read of the frame counts, dv_op_regulate_sample), same build, same process, same GPU: HIP events
around 50 calls after 10 warm-up calls, at B = 1 / Tx = 100 and at B = 16 / Tx = 150 / T' ~ 1024, C = 128; and the peak of
torch's allocator over one call of each branch, above what the inputs hold.  Both branches read the frame counts back once.
  python tools/regulator_bench.py > profiles/regulator_bench.txt"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import diff_vits_amd  # noqa: E402,F401
from diff_vits_amd import synth  # noqa: E402
from diff_vits_amd.model3 import VITS, generate_path, sequence_mask  # noqa: E402

WARMUP, CALLS = 10, 50
C = 128


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / CALLS          # us per call


def peak(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    p = torch.cuda.max_memory_allocated() - base
    del out
    return p / 2.0 ** 20                              # MiB


def torch_branch(logw, x_mask, m_p, logs_p, noise, length_scale, noise_scale):
    w = torch.exp(logw) * x_mask * length_scale
    w_ceil = torch.ceil(w)
    y_len = torch.clamp_min(torch.sum(w_ceil, [1, 2]), 1).long()
    y_mask = torch.unsqueeze(sequence_mask(y_len, None), 1).to(x_mask.dtype)
    attn = generate_path(w_ceil, torch.unsqueeze(x_mask, 2) * torch.unsqueeze(y_mask, -1))
    m_p = torch.matmul(attn.squeeze(1), m_p.transpose(1, 2)).transpose(1, 2)
    logs_p = torch.matmul(attn.squeeze(1), logs_p.transpose(1, 2)).transpose(1, 2)
    eps = noise.to(m_p)
    return m_p + eps * torch.exp(logs_p) * noise_scale, y_len


def main():
    vits = VITS(backend="torch", prior_backend="hip")
    print("# length regulator (logw, m_p, logs_p, noise -> z_p; C = %d), us per call: HIP events around %d calls after %d warm-up calls,\n"
          "# one process, %s; peak = torch allocator peak over one call above the inputs (tools/regulator_bench.py)"
          % (C, CALLS, WARMUP, torch.cuda.get_device_name(0)))
    for B, Tx, mu, std in ((1, 100, 0.5, 0.6), (16, 150, 1.75, 0.4)):
        tag = "regbench.%d.%d." % (B, Tx)
        x_len = torch.tensor([max(1, Tx - 2 * b) for b in range(B)]).cuda()
        x_mask = torch.unsqueeze(sequence_mask(x_len, Tx), 1).float()
        logw = (torch.from_numpy(synth.normal(1234, tag + "logw", (B, 1, Tx), std=std)).cuda() + mu) * x_mask
        m_p = torch.from_numpy(synth.normal(1234, tag + "m", (B, C, Tx))).cuda()
        logs_p = torch.from_numpy(synth.normal(1234, tag + "logs", (B, C, Tx), std=0.3)).cuda() - 0.5
        with torch.no_grad():
            Tp = int(torch.clamp_min(torch.ceil(torch.exp(logw) * x_mask).sum([1, 2]), 1).max())
            noise = torch.from_numpy(synth.normal(1234, tag + "noise", (B, C, Tp))).cuda()
            run_t = lambda: torch_branch(logw, x_mask, m_p, logs_p, noise, 1, 0.667)                       # noqa: E731
            run_h = lambda: vits._regulate_hip(logw, m_p, logs_p, x_len, 0.667, 1, noise)                   # noqa: E731
            (zt, yt), (zh, yh) = run_t(), run_h()
            assert torch.equal(yt, yh), (yt, yh)
            dz = float((zt - zh).abs().max())
            t_t, t_h = timed(run_t), timed(run_h)
            p_t, p_h = peak(run_t), peak(run_h)
        print("B=%d Tx=%d T'=%d: torch branch %.1f us, peak %.2f MiB | native branch %.1f us (x%.2f), peak %.2f MiB | frame counts identical, "
              "max |z_torch - z_native| %.2e" % (B, Tx, Tp, t_t, p_t, t_h, t_t / t_h, p_h, dz))


if __name__ == "__main__":
    main()
