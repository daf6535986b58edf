#!/usr/bin/env python3
"""Hash of the denoiser output at four shapes (GPU box): two builds whose change is meant to be bit-neutral must print the same
lines.  Usage: python tools/hash_fwd.py [bf16x3|bf16]   |   DVITS_LIB_FILE=diff-vits_amd/libdvits_hip_<other>.so python tools/hash_fwd.py
(2, 300, 77): padded row spaces on the fused schedule.  (1, 99, 33): a short utterance - under 128 rows at the deep levels, one
launch per GEMM, the small tiles, and last row blocks with fewer than 32 frames at every level."""
import sys, hashlib, torch
sys.path.insert(0, '.')
import bench
from diff_vits_amd import synth
precision = sys.argv[1] if len(sys.argv) > 1 else "bf16x3"
assert precision in ("bf16x3", "bf16"), precision
dev = torch.device("cuda", 0)
m, _ = bench.build_model(dev, precision)
for (B, T, L) in [(8, 1024, 256), (2, 300, 77), (1, 256, 128), (1, 99, 33)]:
    x, cond, enc, mask = (torch.from_numpy(a).to(dev) for a in synth.make_inputs(B, 80, T, L, seed=5))
    t = torch.linspace(900., 30., B, device=dev)
    with torch.no_grad():
        y = m(torch.cat([x, cond], 1), t, enc, encoder_attention_mask=mask).sample
    torch.cuda.synchronize()
    print(precision, B, T, L, hashlib.sha1(y.cpu().numpy().tobytes()).hexdigest()[:16], float(y.abs().mean()))
