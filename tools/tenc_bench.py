"""Text encoder enc_p, torch ops against the native engine (dv_tenc_forward), same process, same GPU: HIP events around 50
calls after 10 warm-up calls, at B = 1 / T = 100 and at B = 16 / T = 36 (configuration 5's token count), product configuration,
synthetic weights, with the speaker vector.
  python tools/tenc_bench.py > profiles/tenc_bench.txt"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import diff_vits_amd  # noqa: E402,F401
import tenc_cases as tc  # noqa: E402
from diff_vits_amd.model3 import TextEncoder  # noqa: E402

WARMUP, CALLS = 10, 50


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


def main():
    sd = tc.state_dict()
    models = {}
    for backend in (None, "hip"):
        m = TextEncoder(backend=backend, **tc.KW).eval()
        m.load_state_dict(sd)
        models[backend] = m.cuda()
    print("# enc_p (TextEncoder: H = 256, 2 heads, 6 layers, k = 3, window 4, speaker vector), us per call: HIP events around %d calls\n"
          "# after %d warm-up calls, one process, %s (tools/tenc_bench.py)" % (CALLS, WARMUP, torch.cuda.get_device_name(0)))
    for B, T in ((1, 100), (16, 36)):
        lengths = [max(1, T - 2 * b) for b in range(B)]
        ids, tone, lang, ln, g = (v.cuda() for v in tc.inputs(B, T, lengths))
        eng = models["hip"].hip_engine()
        with torch.no_grad():
            t_torch = timed(lambda: models[None](ids, ln, tone, lang, g))
            t_mod = timed(lambda: models["hip"](ids, ln, tone, lang, g))
            t_eng = timed(lambda: eng.forward(ids, ln, tone, lang, g, validate=False))
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                eng.forward(ids, ln, tone, lang, g, validate=False)
            t_graph = timed(graph.replay)
        n_launch, flops = eng.stats()
        print("B=%d T=%d: torch ops %.1f us | dv_tenc_forward %.1f us (x%.2f) | the same replayed from a captured graph %.1f us (x%.2f) | "
              "TextEncoder(backend='hip') with its host checks %.1f us | %d launches per forward, %.3f GFLOP"
              % (B, T, t_torch, t_eng, t_torch / t_eng, t_graph, t_torch / t_graph, t_mod, n_launch, flops * 1e-9))


if __name__ == "__main__":
    main()
