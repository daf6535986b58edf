#!/usr/bin/env python3
"""Hashes of what the single-operator entry points (csrc/ops.hip) write, one line per case (GPU box): two builds whose change is
meant to be bit-neutral must print the same lines.  Every output buffer of a call is hashed - fp32 outputs, hi and lo planes,
statistics - from zero-filled buffers, so rows a kernel leaves alone count too.
The shapes and the seeded inputs are this tool's own, small ones that take each listed path once - not those of tests/test_gpu_*.py.
Usage: python tools/hash_ops.py   |   DVITS_LIB_FILE=diff-vits_amd/libdvits_hip_<other>.so python tools/hash_ops.py"""
import sys, hashlib, torch
sys.path.insert(0, '.')
from diff_vits_amd import _lib as L

gen = torch.Generator().manual_seed(11)


def rnd(*shape, scale=1.0):
    return (scale * torch.randn(*shape, generator=gen)).cuda()


def f32(*shape):
    return torch.zeros(*shape, device="cuda")


def i16(*shape):
    return torch.zeros(*shape, dtype=torch.int16, device="cuda")


def report(name, rc, outs):
    L.check(rc, name)
    torch.cuda.synchronize()
    print("%-44s %s" % (name, " ".join(hashlib.sha1(o.cpu().numpy().tobytes()).hexdigest()[:12] for o in outs)), flush=True)


P = lambda t: None if t is None else L.ptr(t)
lib = L.lib()

# dv_op_conv1d: k = 3 with stride 2; k = 1 with up_T
B, Cin, T, Cout = 2, 40, 37, 72
x, w3, w1, b = rnd(B, Cin, T), rnd(Cout, Cin, 3, scale=0.1), rnd(Cout, Cin, 1, scale=0.1), rnd(Cout, scale=0.1)
y = f32(B, Cout, (T + 2 - 3) // 2 + 1)
report("conv1d k=3 stride=2", lib.dv_op_conv1d(P(x), P(w3), P(b), P(y), B, Cin, T, Cout, 3, 2, 0, L.PREC_BF16X3, None), [y])
y = f32(B, Cout, 90)
report("conv1d k=1 up_T=90", lib.dv_op_conv1d(P(x), P(w1), P(b), P(y), B, Cin, T, Cout, 1, 1, 90, L.PREC_BF16X3, None), [y])

# dv_op_linear, dv_op_linear_planes (plain and GEGLU)
M, K, N = 130, 96, 72
x, w, b = rnd(M, K), rnd(N, K, scale=K ** -0.5), rnd(N, scale=0.1)
y = f32(M, N)
report("linear", lib.dv_op_linear(P(x), P(w), P(b), P(y), M, K, N, L.PREC_BF16X3, None), [y])
y = f32(M, N)
report("linear bf16", lib.dv_op_linear(P(x), P(w), P(b), P(y), M, K, N, L.PREC_BF16, None), [y])
y, hi, lo = f32(M, 76), i16(M, 76), i16(M, 76)
report("linear_planes", lib.dv_op_linear_planes(P(x), P(w), P(b), P(y), P(hi), P(lo), M, K, N, 76, 0, L.PREC_BF16X3, None), [y, hi, lo])
No = 32
w, b = rnd(2 * No, K, scale=K ** -0.5), rnd(2 * No, scale=0.1)
hi, lo = i16(M, 36), i16(M, 36)
report("linear_planes geglu", lib.dv_op_linear_planes(P(x), P(w), P(b), None, P(hi), P(lo), M, K, 2 * No, 36, 1, L.PREC_BF16X3, None), [hi, lo])

# dv_op_gemm: two sources; residual + ReLU + row mask; fused split-K
M, K, N = 130, 160, 96
x, w, b, res = rnd(M, K), rnd(N, K, scale=K ** -0.5), rnd(N, scale=0.1), rnd(M, 100)
mask = (torch.arange(M) % 5 != 0).float().cuda()
y, hi, lo = f32(M, N), i16(M, N), i16(M, N)
report("gemm two sources K0=64", lib.dv_op_gemm(P(x), P(w), P(b), None, None, P(y), P(hi), P(lo), M, K, N, 64, N, 0, L.GEMM_STORE, 0, 0, 0,
                                                L.PREC_BF16X3, None), [y, hi, lo])
y = f32(M, N)
report("gemm residual relu rowmask", lib.dv_op_gemm(P(x), P(w), P(b), P(res), P(mask), P(y), None, None, M, K, N, 0, N, 100, L.GEMM_RESIDUAL, 1,
                                                    0, 0, L.PREC_BF16X3, None), [y])
M, K, N = 130, 256, 96
x, w, b = rnd(M, K), rnd(N, K, scale=K ** -0.5), rnd(N, scale=0.1)
y = f32(M, N)
report("gemm fused split-K", lib.dv_op_gemm(P(x), P(w), P(b), None, None, P(y), None, None, M, K, N, 0, N, 0, L.GEMM_STORE, 0, 0,
                                            2 | L.GEMM_SPLITK_FUSED, L.PREC_BF16X3, None), [y])
y = f32(M, N)
report("gemm split-K 3 slices bf16", lib.dv_op_gemm(P(x), P(w), P(b), None, None, P(y), None, None, M, K, N, 0, N, 0, L.GEMM_STORE, 0, 0, 3,
                                                    L.PREC_BF16, None), [y])


# dv_op_conv_rows: [a0 | a1] with stats16; a second k-segment; DV_UP_SIZE; stride 2 in bf16 mode
def conv_rows(name, B, T, Tp_in, c0, c1, c_sc, Cout, taps, stride, up_mode, up_T, Tp_out, stats, prec):
    x0, x1, xs = rnd(B, Tp_in, c0), (rnd(B, Tp_in, c1) if c1 else None), (rnd(B, Tp_in, c_sc) if c_sc else None)
    w, ws, b = rnd(Cout, c0 + c1, taps, scale=0.05), (rnd(Cout, c_sc, 1, scale=0.05) if c_sc else None), rnd(Cout, scale=0.1)
    y, hi, lo = f32(B, Tp_out, Cout), i16(B, Tp_out, Cout), i16(B, Tp_out, Cout)
    st = f32(B * Tp_out // 32, Cout // 16, 2) if stats else None
    rc = lib.dv_op_conv_rows(P(x0), P(x1), P(w), P(b), P(xs), P(ws), P(y), P(hi), P(lo), P(st), B, T, Tp_in, c0, c1, c_sc, Cout, taps, stride,
                             up_mode, up_T, Tp_out, 0, prec, None)
    report(name, rc, [y, hi, lo] + ([st] if stats else []))


conv_rows("conv_rows [a0|a1] stats16", 2, 33, 40, 64, 32, 0, 48, 3, 1, L.UP_NONE, 0, 64, True, L.PREC_BF16X3)
conv_rows("conv_rows second k-segment", 2, 33, 64, 64, 0, 64, 40, 3, 1, L.UP_NONE, 0, 64, False, L.PREC_BF16X3)
conv_rows("conv_rows UP_SIZE 20 -> 50", 2, 20, 32, 64, 0, 0, 40, 3, 1, L.UP_SIZE, 50, 64, False, L.PREC_BF16X3)
conv_rows("conv_rows stride 2 bf16", 2, 33, 64, 64, 0, 0, 40, 3, 2, L.UP_NONE, 0, 32, False, L.PREC_BF16)

# dv_op_conv3: with the shortcut segment; up2
B, Cin, T, Tp, Cout, Csc = 2, 256, 63, 64, 256, 128
x, w, b = rnd(B, Tp, Cin), rnd(Cout, Cin, 3, scale=(3 * Cin) ** -0.5), rnd(Cout, scale=0.1)
xs, ws = rnd(B, Tp, Csc), rnd(Cout, Csc, 1, scale=Csc ** -0.5)
y = f32(B, Tp, Cout)
report("conv3 shortcut", lib.dv_op_conv3(P(x), P(w), P(b), P(xs), P(ws), P(y), B, Cin, T, Tp, Cout, Csc, 0, None), [y])
y = f32(B, Tp, Cout)
report("conv3", lib.dv_op_conv3(P(x), P(w), P(b), None, None, P(y), B, Cin, T, Tp, Cout, 0, 0, None), [y])
T = 50
y = f32(B, (2 * T + 31) // 32 * 32, Cout)
report("conv3 up2", lib.dv_op_conv3(P(x), P(w), P(b), None, None, P(y), B, Cin, T, Tp, Cout, 0, 1, None), [y])
B, Cin, T, Cout = 1, 1024, 128, 512      # (long K, 128 frames: the fused split-K pair where the CU count asks for it)
x, w, b = rnd(B, T, Cin), rnd(Cout, Cin, 3, scale=(3 * Cin) ** -0.5), rnd(Cout, scale=0.1)
y = f32(B, T, Cout)
report("conv3 long K", lib.dv_op_conv3(P(x), P(w), P(b), None, None, P(y), B, Cin, T, T, Cout, 0, 0, None), [y])

# dv_op_linear_ln: fused and unfused
M, K, C, N = 33, 64, 128, 96
a = [rnd(M, K), rnd(C, K, scale=K ** -0.5), rnd(C, scale=0.1), rnd(M, C), 1 + rnd(C, scale=0.1), rnd(C, scale=0.1), rnd(N, C, scale=C ** -0.5),
     rnd(N, scale=0.1)]
for fused in (1, 0):
    y1, rs, y2 = f32(M, C), f32(M, C // 32, 2), f32(M, N)
    report("linear_ln fused=%d" % fused, lib.dv_op_linear_ln(*[P(t) for t in a], M, K, C, N, fused, P(y1), P(rs) if fused else None, P(y2), None),
           [y1, rs, y2])

# dv_op_linear_gn: the three routes
B, K, C, G = 2, 64, 128, 8
for name, route, T, Tp in (("stat16", L.GN_STAT16, 33, 64), ("slab", L.GN_SLAB, 64, 64), ("k_stat16", L.GN_KSTAT16, 64, 64)):
    a = [rnd(B, Tp, K), rnd(C, K, scale=K ** -0.5), rnd(C, scale=0.1), 1 + rnd(C, scale=0.1), rnd(C, scale=0.1)]
    y, hi, lo = f32(B, Tp, C), i16(B, Tp, C), i16(B, Tp, C)
    st = f32(B * Tp // 32, C, 2) if route == L.GN_SLAB else f32(B * Tp // 32, C // 16, 2)
    report("linear_gn " + name, lib.dv_op_linear_gn(*[P(t) for t in a], B, T, Tp, K, C, G, 1e-5, route, P(y), P(st), P(hi), P(lo), None), [y, st, hi, lo])
    y, hi, lo = f32(B, Tp, C), i16(B, Tp, C), i16(B, Tp, C)
    report("linear_gn " + name + ", own statistics", lib.dv_op_linear_gn(*[P(t) for t in a], B, T, Tp, K, C, G, 1e-5, route, P(y), None, P(hi), P(lo), None),
           [y, hi, lo])

# dv_op_attention_frag
B, H, Tq, Tk, d = 2, 8, 300, 65, 16
q, k, v = rnd(B, Tq, H * d), rnd(B, Tk, H * d), rnd(B, Tk, H * d)
bias = torch.zeros(B, Tk)
for i in range(B):
    bias[i, max(1, Tk - 7 * (i + 1)):] = -10000.0
bias, o = bias.cuda(), f32(B, Tq, H * d)
report("attention_frag", lib.dv_op_attention_frag(P(q), P(k), P(v), P(bias), P(o), B, H, Tq, Tk, d, None), [o])

# dv_op_group_stats
B, T, C, G = 2, 300, 128, 8
x, mean, rstd = rnd(B, T, C), f32(B, G), f32(B, G)
report("group_stats", lib.dv_op_group_stats(P(x), P(mean), P(rstd), B, T, C, G, 1e-5, None), [mean, rstd])
