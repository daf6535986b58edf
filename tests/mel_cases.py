"""The restatement the log-mel front-end is held to, its cases and criteria (mel.MelSpectrogram with `lengths`, both backends;
dv_mel_forward / k_log_mel, csrc/kernels_mel.hip).  Shared by tests/test_mel_reference.py (CPU), tests/test_gpu_mel.py and
tools/mel_reference.py; every input is generated from a seed, nothing is read from disk.

`restate64` is the definition in fp64, frame by frame: the explicit reflect index map about each ROW's own ends, an explicit cos / sin
DFT matrix, sqrt, the dense filterbank product.  It never goes through torch.stft's padding; test_mel_reference.py pins it to mel.py's
fp64 torch.stft path on full-length rows.

`emulate32` is a numpy float32 restatement of the KERNEL's arithmetic: the same even / odd packing, the same three radix-8 Stockham
passes with the same rounded twiddle table, the same untangle, the same ascending band sums.  It cannot hold fma contraction and the
device's sqrtf / logf equal.  Its `fault` argument plants the mistakes the criteria must catch (test_mel_reference.py).

MEL_FRAME_BOUND is measured, not chosen: tools/mel_reference.py runs (a) mel.py's fp32 path on the CPU and (b) emulate32 over this
case list against restate64; the bound is 2 x the larger worst figure (the factor covers what the emulation cannot hold equal).  Both
figures are in profiles/mel_reference.txt and sit at <= 0.5 of the bound by construction."""
import numpy as np
import torch

N_FFT, HOP, N_BINS, FPW = 1024, 256, 513, 4          # FPW: frames per workgroup of k_log_mel
CLIP = float(np.float32(1e-7))                       # what log(clip(x, 1e-7)) compares float32 values with
MEL_FRAME_BOUND = 8.0e-7                             # profiles/mel_reference.txt (tools/mel_reference.py): 2 x max(a, b)
LOGF_ULPS = 4 * 2.0 ** -24

RAGGED_N = [513, 2048, 1025, 4096, 769]
# single-row lengths: every frame reflecting (513), around 3 / 4 / 5 hops, and L one below / at / above FPW and 2 FPW
SINGLE_N = [513, 767, 768, 769, 1023, 1024, 1025, 1279, 1280, 1281, 1791, 1792, 2048]
SIGNALS = ("noise", "tone", "zeros", "imp0", "imp1", "impN1", "impN2", "impB", "dc", "quiet")


def signal(kind, n, seed):
    rs = np.random.RandomState(seed)
    t = np.arange(n, dtype=np.float64)
    if kind == "noise":
        x = 0.3 * rs.standard_normal(n)
    elif kind == "quiet":
        x = 0.3e-4 * rs.standard_normal(n)
    elif kind == "tone":     # bin 37's centre, and a tone 80 dB below it at bin 400
        x = 0.5 * np.sin(2 * np.pi * 37 * t / N_FFT) + 0.5e-4 * np.sin(2 * np.pi * 400 * t / N_FFT + 0.3)
    elif kind == "zeros":
        x = np.zeros(n)
    elif kind == "dc":
        x = np.ones(n)
    elif kind.startswith("imp"):
        x = np.zeros(n)
        x[{"imp0": 0, "imp1": 1, "impN1": n - 1, "impN2": n - 2, "impB": 512}[kind]] = 1.0
    else:
        raise KeyError(kind)
    return x.astype(np.float32)


def impulse_position(kind, n):
    return {"imp0": 0, "imp1": 1, "impN1": n - 1, "impN2": n - 2, "impB": 512}[kind]


def _case(name, ns, n_max, kinds, mel_kw=None):
    return dict(name=name, n=list(ns), n_max=n_max, kinds=list(kinds), mel_kw=dict(mel_kw or {}))


def cases():
    out = [_case("noise_n%d" % n, [n], n, ["noise"]) for n in SINGLE_N]
    for kind in SIGNALS[1:]:
        out += [_case("%s_n%d" % (kind, n), [n], n, [kind]) for n in (513, 1025, 2048)]
    kinds = ["noise", "tone", "noise", "quiet", "tone"]
    out.append(_case("ragged4096", RAGGED_N, 4096, kinds))
    out.append(_case("ragged5000", RAGGED_N, 5000, kinds))
    out.append(_case("b16_n24000", [24000] * 16, 24000, ["noise"] * 16))
    # a filterbank that reaches past the Nyquist bin: row 512 of fb is non-zero (with f_max = sr / 2 it is all zeros)
    out.append(_case("fmax12500_n1025", [1025], 1025, ["noise"], dict(f_max=12500.0)))
    return out


CASES = {c["name"]: c for c in cases()}
POWER2_CASES = ("ragged4096", "tone_n2048")


def make_wave(case, fill=0.0):
    """float32 [B, n_max]: each row's signal, `fill` behind its n_b samples."""
    w = np.full((len(case["n"]), case["n_max"]), fill, dtype=np.float32)
    for b, (n, kind) in enumerate(zip(case["n"], case["kinds"])):
        w[b, :n] = signal(kind, n, 1000 + 17 * b + n)
    return w


def tables(mel_kw=None):
    """(window float32 [1024], fb float32 [513, n_mels]) - the buffers mel.MelSpectrogram registers."""
    from diff_vits_amd.mel import MelSpectrogram
    m = MelSpectrogram(**(mel_kw or {}))
    return m.window.numpy().copy(), m.fb.numpy().copy()


def frame_index(n, n_ref=None, L=None, symmetric=False):
    """[L, 1024] sample index of every frame of an n-sample recording: f hop - 512 + j reflected about 0 and about n_ref - 1."""
    n_ref = n if n_ref is None else n_ref
    L = 1 + n // HOP if L is None else L
    i = np.arange(L)[:, None] * HOP - N_FFT // 2 + np.arange(N_FFT)[None, :]
    if symmetric:            # planted fault: the edge sample repeated
        i = np.where(i < 0, -i - 1, i)
        i = np.where(i >= n_ref, 2 * n_ref - 1 - i, i)
    else:
        i = np.where(i < 0, -i, i)
        i = np.where(i >= n_ref, 2 * (n_ref - 1) - i, i)
    return i


_DFT = {}


def dft_matrices():
    if not _DFT:
        ang = 2.0 * np.pi * ((np.arange(N_FFT)[:, None] * np.arange(N_BINS)[None, :]) % N_FFT) / N_FFT
        _DFT["c"], _DFT["s"] = np.cos(ang), -np.sin(ang)
    return _DFT["c"], _DFT["s"]


def restate64(wave, ns, window, fb, power=1):
    """fp64 linear mel [B, n_mels, 1 + n_max // hop] (zeros behind each row's frames) and frames [B]."""
    Cm, Sm = dft_matrices()
    w64, fb64 = window.astype(np.float64), fb.astype(np.float64)
    B, n_max = wave.shape
    out = np.zeros((B, fb.shape[1], 1 + n_max // HOP))
    for b, n in enumerate(ns):
        x = wave[b, :n].astype(np.float64)[frame_index(n)] * w64
        mag = np.sqrt((x @ Cm) ** 2 + (x @ Sm) ** 2)
        if power == 2:
            mag = mag * mag
        out[b, :, :1 + n // HOP] = (mag @ fb64).T
    return out, np.array([1 + n // HOP for n in ns], dtype=np.int64)


# ------------------------------------------------------------------------------------------ the kernel's arithmetic in numpy float32
def twiddles():
    t = np.arange(512)
    tw512 = (np.cos(2 * np.pi * t / 512.0).astype(np.float32), (-np.sin(2 * np.pi * t / 512.0)).astype(np.float32))
    tw1024 = (np.cos(2 * np.pi * t / 1024.0).astype(np.float32), (-np.sin(2 * np.pi * t / 1024.0)).astype(np.float32))
    return tw512, tw1024


def _dft8(r, i):
    h = np.float32(0.70710678118654752440)
    s = [(r[j] + r[j + 4], i[j] + i[j + 4]) for j in range(4)]
    d = [(r[j] - r[j + 4], i[j] - i[j + 4]) for j in range(4)]
    t0, t1 = (s[0][0] + s[2][0], s[0][1] + s[2][1]), (s[0][0] - s[2][0], s[0][1] - s[2][1])
    t2, t3 = (s[1][0] + s[3][0], s[1][1] + s[3][1]), (s[1][0] - s[3][0], s[1][1] - s[3][1])
    o = [None] * 8
    o[0] = (t0[0] + t2[0], t0[1] + t2[1])
    o[4] = (t0[0] - t2[0], t0[1] - t2[1])
    o[2] = (t1[0] + t3[1], t1[1] - t3[0])
    o[6] = (t1[0] - t3[1], t1[1] + t3[0])
    e1 = ((d[1][0] + d[1][1]) * h, (d[1][1] - d[1][0]) * h)
    e2 = (d[2][1], -d[2][0])
    e3 = ((d[3][1] - d[3][0]) * h, (-d[3][0] - d[3][1]) * h)
    u0, u1 = (d[0][0] + e2[0], d[0][1] + e2[1]), (d[0][0] - e2[0], d[0][1] - e2[1])
    u2, u3 = (e1[0] + e3[0], e1[1] + e3[1]), (e1[0] - e3[0], e1[1] - e3[1])
    o[1] = (u0[0] + u2[0], u0[1] + u2[1])
    o[5] = (u0[0] - u2[0], u0[1] - u2[1])
    o[3] = (u1[0] + u3[1], u1[1] - u3[0])
    o[7] = (u1[0] - u3[1], u1[1] + u3[0])
    return [x[0] for x in o], [x[1] for x in o]


def _twiddle(br, bi, tr, ti):
    return br * tr - bi * ti, br * ti + bi * tr


def fft512_f32(zr, zi):
    """[L, 512] float32 -> Z [L, 512]: three radix-8 Stockham passes, as k_log_mel runs them."""
    (t5r, t5i), _ = twiddles()
    L = zr.shape[0]
    k8 = np.arange(8)
    # pass 1: x[p + 64 j] -> y[8 p + k] W_512^(p k)
    xr, xi = zr.reshape(L, 8, 64), zi.reshape(L, 8, 64)
    br, bi = _dft8([xr[:, j] for j in range(8)], [xi[:, j] for j in range(8)])
    yr, yi = np.empty((L, 64, 8), np.float32), np.empty((L, 64, 8), np.float32)
    p = np.arange(64)
    for k in k8:
        yr[:, :, k], yi[:, :, k] = (br[k], bi[k]) if k == 0 else _twiddle(br[k], bi[k], t5r[p * k], t5i[p * k])
    # pass 2: x[q + 8 p + 64 j] -> y[q + 64 p + 8 k] W_64^(p k)
    xr, xi = yr.reshape(L, 8, 8, 8), yi.reshape(L, 8, 8, 8)
    br, bi = _dft8([xr[:, j] for j in range(8)], [xi[:, j] for j in range(8)])
    yr, yi = np.empty((L, 8, 8, 8), np.float32), np.empty((L, 8, 8, 8), np.float32)
    p = np.arange(8)[:, None]
    for k in k8:
        yr[:, :, k, :], yi[:, :, k, :] = (br[k], bi[k]) if k == 0 else _twiddle(br[k], bi[k], t5r[8 * p * k], t5i[8 * p * k])
    # pass 3: x[q + 64 j] -> Z[q + 64 k]
    xr, xi = yr.reshape(L, 8, 64), yi.reshape(L, 8, 64)
    br, bi = _dft8([xr[:, j] for j in range(8)], [xi[:, j] for j in range(8)])
    return np.stack(br, 1).reshape(L, 512), np.stack(bi, 1).reshape(L, 512)


def _bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).bfloat16().float().numpy()


def magnitudes_f32(xw, fault=None):
    """Windowed frames float32 [L, 1024] -> 513 magnitudes float32 [L, 513]."""
    L = xw.shape[0]
    if fault == "bf16x3":      # the rejected MFMA design: the DFT as a contraction of split bf16 planes, fp32 accumulation
        Cm, Sm = dft_matrices()
        xh = _bf16(xw)
        xl = _bf16(xw - xh)
        res = []
        for M in (Cm, Sm):
            mh = _bf16(M)
            ml = _bf16(M.astype(np.float32) - mh)
            res.append(xh @ mh + (xh @ ml + xl @ mh))
        return np.sqrt(res[0] * res[0] + res[1] * res[1])
    zr, zi = fft512_f32(np.ascontiguousarray(xw[:, 0::2]), np.ascontiguousarray(xw[:, 1::2]))
    _, (t1r, t1i) = twiddles()
    k = np.arange(512)
    k2 = (512 - k) & 511
    ar, ai, cr, ci = zr[:, k], zi[:, k], zr[:, k2], -zi[:, k2]
    half = np.float32(0.5)
    er, ei = half * (ar + cr), half * (ai + ci)
    orr, oi = half * (ai - ci), -half * (ar - cr)
    Xr = er + (orr * t1r - oi * t1i)
    Xi = ei + (orr * t1i + oi * t1r)
    mag = np.empty((L, N_BINS), np.float32)
    mag[:, :512] = np.sqrt(Xr * Xr + Xi * Xi)
    mag[:, 512] = 0.0 if fault == "no_nyquist" else np.abs(zr[:, 0] - zi[:, 0])
    return mag


def band_ranges(fb):
    out = []
    for m in range(fb.shape[1]):
        nz = np.nonzero(fb[:, m])[0]
        out.append((int(nz[0]), int(nz[-1])) if len(nz) else (0, -1))
    return out


def emulate32(wave, ns, window, fb, power=1, log=False, fault=None):
    """The kernel's result in numpy float32: out [B, n_mels, L_max], frames [B].  fault: None or one of FAULTS."""
    B, n_max = wave.shape
    if fault == "symmetric_hann":
        window = torch.hann_window(N_FFT, periodic=False).numpy()
    out = np.zeros((B, fb.shape[1], 1 + n_max // HOP), np.float32)
    frames = np.zeros(B, np.int64)
    bands = band_ranges(fb)
    for b, n in enumerate(ns):
        L = -(-n // HOP) if fault == "ceil_frames" else 1 + n // HOP
        idx = frame_index(n, n_ref=n_max if fault == "buffer_end" else n, L=L, symmetric=fault == "symmetric_pad")
        mag = magnitudes_f32(wave[b][np.clip(idx, 0, n_max - 1)] * window[None, :], fault)
        if power == 2:
            mag = mag * mag
        for m, (lo, hi) in enumerate(bands):
            acc = np.zeros(L, np.float32)
            for k in range(lo, hi + (0 if fault == "band_hi_short" else 1)):
                acc = acc + fb[k, m] * mag[:, k]
            out[b, m, :L] = np.log(np.maximum(acc, np.float32(CLIP))) if log else acc
        frames[b] = L
    return out, frames


FAULTS = ("symmetric_pad", "buffer_end", "ceil_frames", "symmetric_hann", "no_nyquist", "band_hi_short", "bf16x3")


# ------------------------------------------------------------------------------------------ criteria
def linear_error(v, v64, frames):
    """Worst frame's max_m |v - v64| / max(peak_f, clip), peak_f = max_m v64, over every row's valid frames."""
    worst = 0.0
    for b, L in enumerate(frames):
        L = int(L)
        if L > 0:
            peak = np.maximum(v64[b, :, :L].max(0), CLIP)
            worst = max(worst, float((np.abs(v[b, :, :L].astype(np.float64) - v64[b, :, :L]).max(0) / peak).max()))
    return worst


def log_error(y, v64, frames, bound=None):
    """Worst |y - log(max(v64, clip))| as a fraction of its tolerance
    bound * max(peak_f, clip) / max(v64, clip) + 4 * 2^-24 * |log| - the linear bound carried through the log plus logf's own error."""
    bound = MEL_FRAME_BOUND if bound is None else bound
    worst = 0.0
    for b, L in enumerate(frames):
        L = int(L)
        if L > 0:
            floor = np.maximum(v64[b, :, :L], CLIP)
            ref = np.log(floor)
            tol = bound * np.maximum(v64[b, :, :L].max(0), CLIP)[None, :] / floor + LOGF_ULPS * np.abs(ref)
            worst = max(worst, float((np.abs(y[b, :, :L].astype(np.float64) - ref) / tol).max()))
    return worst


def padding_is_zero(out, frames):
    return all(not np.any(out[b, :, int(L):]) for b, L in enumerate(frames))


def check(case, out, frames, v64, log, bound=None):
    """Every criterion on one result; returns the list of (criterion, figure) that fail (empty: the result passes)."""
    bound = MEL_FRAME_BOUND if bound is None else bound
    want = np.array([1 + n // HOP for n in case["n"]], dtype=np.int64)
    bad = []
    if out.shape != v64.shape or not np.array_equal(np.asarray(frames, dtype=np.int64), want):
        return [("frames", [int(f) for f in frames])]
    if not np.all(np.isfinite(out)):
        return [("finite", float("nan"))]
    if not padding_is_zero(out, want):
        bad.append(("padding", 1.0))
    if log:
        e = log_error(out, v64, want, bound)
        if e > 1.0:
            bad.append(("log", e))
    else:
        e = linear_error(out, v64, want)
        if e > bound:
            bad.append(("linear", e))
    return bad
