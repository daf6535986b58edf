"""The restatement the sample-rate converter is held to, its cases and criteria (audio.Resample, both backends; dv_resample_forward /
k_resample, csrc/kernels_resample.hip).  Shared by tests/test_resample_reference.py (CPU), tests/test_gpu_resample.py and
tools/resample_reference.py; every input is generated from a seed, nothing is read from disk.

The definition is torchaudio.transforms.Resample(orig, new) with its documented defaults (sinc_interp_hann, lowpass_filter_width 6,
rolloff 0.99), written from the published source.  torchaudio is not installed where this project builds and runs, so the
restatement is NOT checked against torchaudio output.  With o = orig / gcd, n = new / gcd: base = min(o, n) * 0.99,
width = ceil(6 o / base), K = 2 width + o,
    t = clamp((-p / n + (j - width) / o) * base, -6, 6),  h[p][j] = (t == 0 ? 1 : sin(pi t) / (pi t)) * cos(pi t / 12)^2 * base / o,
the taps in fp64 rounded ONCE to fp32 (audio.filter_table); an N-sample row gives N_out = ceil(n N / o) samples
    y[q n + p] = sum_j h[p][j] x[q o - width + j],   x = 0 outside [0, N);   orig == new: the input unchanged.

`restate64` is that definition in dense fp64: the explicit index map q o - width + j, a gather, a sum - no convolution routine; every
row from its own N samples alone.

`emulate32` is a numpy float32 restatement of the KERNEL's arithmetic: per phase the range from the first to the last non-zero tap,
the sum over it in ascending j starting from the first product, the tile's staged span.  It cannot hold fma contraction equal.  Its
`fault` argument plants the mistakes the criterion must catch (test_resample_reference.py).

The criterion is per block of 256 output samples: worst |v - v64| over the block's fp64 peak, floored at 0.1 x the row's rms.
RESAMPLE_BLOCK_BOUND is measured, not chosen: tools/resample_reference.py runs (a) audio.Resample's fp32 torch route on the CPU and
(b) emulate32 over this case list against restate64; the bound is 2 x the larger worst figure (the factor covers fma contraction,
which the emulation cannot hold equal).  Both figures are in profiles/resample_reference.txt and sit at <= 0.5 of the bound by
construction."""
import numpy as np

import mel_cases
from diff_vits_amd.audio import filter_table, output_length, reduce_pair

TILE = 512                                   # output samples per workgroup of k_resample
BLOCK = 256                                  # output samples per block of the criterion
RESAMPLE_BLOCK_BOUND = 6.6e-7                # profiles/resample_reference.txt (tools/resample_reference.py): 2 x max(a, b)

# (orig, new): 2:1, 2:3, 1:3, 147:80, 147:160 into 24 kHz; 3:2, 80:147, 1:2 out of it; 441:160
RATES = [(48000, 24000), (16000, 24000), (8000, 24000), (44100, 24000), (22050, 24000), (24000, 16000), (24000, 44100), (24000, 48000),
         (44100, 16000)]
SIGNALS = ("noise", "quiet", "tone", "dc", "imp0", "impN1")


def ratio_name(orig, new):
    return "%d:%d" % reduce_pair(orig, new)


def length_for(target, o, n):
    """The smallest N whose N_out = ceil(n N / o) reaches `target` (equal to it whenever o >= n; when upsampling N_out moves in steps)."""
    return ((target - 1) * o) // n + 1


def signal(kind, n, seed):
    return mel_cases.signal(kind, n, seed)


def _case(name, rates, new, ns, n_max, kinds):
    return dict(name=name, rates=list(rates), new=new, n=list(ns), n_max=n_max, kinds=list(kinds))


def ratio_cases(orig, new):
    """One ratio's single-row cases: N_out at TILE - 1, TILE, TILE + 1 and 2 TILE + 1, N = 1, N < width, and every signal kind."""
    o, n = reduce_pair(orig, new)
    _, width = filter_table(o, n)
    tag = "%dto%d" % (orig, new)
    out = []
    for target in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        N = length_for(target, o, n)
        out.append(_case("%s_noise_out%d" % (tag, target), [orig], new, [N], N, ["noise"]))
    out.append(_case("%s_noise_n1" % tag, [orig], new, [1], 1, ["noise"]))
    out.append(_case("%s_noise_n%d" % (tag, width - 2), [orig], new, [width - 2], width - 2, ["noise"]))
    N = length_for(TILE + 1, o, n)
    for kind in SIGNALS[1:]:
        out.append(_case("%s_%s" % (tag, kind), [orig], new, [N], N, [kind]))
    return out


RAGGED_RATES = [44100, 16000, 48000, 22050, 8000]
RAGGED_N = [2825, 700, 3000, 1500, 171]


def cases():
    out = []
    for orig, new in RATES:
        out += ratio_cases(orig, new)
    kinds = ["noise", "tone", "noise", "quiet", "tone"]
    out.append(_case("ragged3000", RAGGED_RATES, 24000, RAGGED_N, 3000, kinds))
    out.append(_case("ragged3333", RAGGED_RATES, 24000, RAGGED_N, 3333, kinds))       # a row pitch that is no multiple of four samples
    # an identity row among converted ones
    out.append(_case("with_identity", [24000, 44100, 24000], 24000, [1000, 1200, 1], 1200, ["noise", "noise", "dc"]))
    return out


CASES = {c["name"]: c for c in cases()}
# Outside the list the bound is measured on: a pair whose span does not fit the LDS beside its table, so that k_resample works its tile
# off in chunks (two of them here).  Its 12 121 taps per output are no audio filter; the result is held per element to the
# a-priori bound of a recursive float32 sum, (taps + 1) * 2^-24 * sum_j |h[p][j] x[.]| (`abs_sum64`), not to RESAMPLE_BLOCK_BOUND.
CHUNKED_CASE = _case("1000to1_chunked", [1000], 1, [20000], 20000, ["noise"])
RATIO_CASES = {ratio_name(o, n): [c["name"] for c in ratio_cases(o, n)] for o, n in RATES}


def make_wave(case, fill=0.0):
    """float32 [B, n_max]: each row's signal, `fill` behind its n_b samples."""
    w = np.full((len(case["n"]), case["n_max"]), fill, dtype=np.float32)
    for b, (n, kind) in enumerate(zip(case["n"], case["kinds"])):
        w[b, :n] = signal(kind, n, 2000 + 31 * b + n)
    return w


def case_pairs(case):
    return [reduce_pair(r, case["new"]) for r in case["rates"]]


def out_width(case):
    return max(output_length(case["n_max"], o, n) for o, n in case_pairs(case))


def expected_n_out(case):
    return np.array([output_length(N, o, n) for N, (o, n) in zip(case["n"], case_pairs(case))], dtype=np.int64)


_TABLES = {}


def table(o, n):
    """(h float32 [n, K], width, first [n], count [n]): the taps and, per phase, the range from the first to the last non-zero one."""
    if (o, n) not in _TABLES:
        h, width = filter_table(o, n)
        first, count = np.zeros(n, np.int64), np.zeros(n, np.int64)
        for p in range(n):
            nz = np.nonzero(h[p])[0]
            if len(nz):
                first[p], count[p] = nz[0], nz[-1] - nz[0] + 1
        for a in (h, first, count):
            a.setflags(write=False)
        _TABLES[(o, n)] = (h, width, first, count)
    return _TABLES[(o, n)]


def restate_row64(x, o, n, absolute=False):
    """One row of the definition in fp64: explicit index map, gather, sum.  absolute: sum_j |h[p][j] x[.]| instead."""
    h, width, _, _ = table(o, n)
    N = len(x)
    i = np.arange(output_length(N, o, n))
    q, p = i // n, i % n
    idx = q[:, None] * o - width + np.arange(h.shape[1])[None, :]
    inside = (idx >= 0) & (idx < N)
    xg = np.where(inside, x.astype(np.float64)[np.clip(idx, 0, max(N - 1, 0))], 0.0)
    prod = h.astype(np.float64)[p] * xg
    return np.abs(prod).sum(1) if absolute else prod.sum(1)


def abs_sum64(x, o, n):
    return restate_row64(x, o, n, absolute=True)


def restate64(wave, ns, pairs, width_out=None):
    """fp64 out [B, width_out] (zeros behind each row's samples) and n_out [B]; row b from wave[b, :ns[b]] alone."""
    rows = [restate_row64(wave[b, :N], o, n) for b, (N, (o, n)) in enumerate(zip(ns, pairs))]
    width_out = max(output_length(wave.shape[1], o, n) for o, n in pairs) if width_out is None else width_out
    out = np.zeros((len(rows), width_out))
    for b, y in enumerate(rows):
        out[b, :len(y)] = y
    return out, np.array([len(y) for y in rows], dtype=np.int64)


# ------------------------------------------------------------------------------------------ the kernel's arithmetic in numpy float32
FAULTS = ("phase_off", "pad_short", "read_behind", "floor_len", "last_tap", "seam_short")


def emulate_row32(buf, N, o, n, fault=None):
    """One row as k_resample computes it; buf is the row's whole buffer (content behind N must not matter)."""
    h, width, first, count = table(o, n)
    n_buf = len(buf)
    n_out = (n * N) // o if fault == "floor_len" else output_length(N, o, n)
    if n_out == 0:
        return np.zeros(0, np.float32)
    i = np.arange(n_out)
    q, p = i // n, i % n
    hp = (p + 1) % n if fault == "phase_off" else p
    pad = width - 1 if fault == "pad_short" else width
    nz = count > 0
    c = (np.arange(n) * o) // n
    dmax = int((first + count - 1 - c)[nz].max())
    # the last sample staged for the output's tile: what floor(i o / n) - width + dmax is at the tile's last live output
    tile_last_out = np.minimum((i // TILE + 1) * TILE, n_out) - 1
    staged_last = (tile_last_out * o) // n - width + dmax - (1 if fault == "seam_short" else 0)
    limit = n_buf if fault == "read_behind" else N
    acc = np.zeros(n_out, np.float32)
    for jj in range(int(count.max())):
        live = jj < (count[hp] - (1 if fault == "last_tap" else 0))
        s = q * o - pad + first[hp] + jj
        ok = live & (s >= 0) & (s < limit) & (s <= staged_last)
        x = np.where(ok, buf[np.clip(s, 0, n_buf - 1)], np.float32(0)).astype(np.float32)
        tap = h[hp, np.minimum(first[hp] + jj, h.shape[1] - 1)]
        prod = (tap * x).astype(np.float32)
        acc = np.where(live, prod if jj == 0 else (acc + prod).astype(np.float32), acc)
    return acc


def emulate32(wave, ns, pairs, width_out=None, fault=None):
    """The kernel's result in numpy float32: out [B, width_out], n_out [B].  fault: None or one of FAULTS."""
    rows = [emulate_row32(wave[b], N, o, n, fault) for b, (N, (o, n)) in enumerate(zip(ns, pairs))]
    width_out = max(output_length(wave.shape[1], o, n) for o, n in pairs) if width_out is None else width_out
    out = np.zeros((len(rows), width_out), np.float32)
    for b, y in enumerate(rows):
        out[b, :len(y)] = y
    return out, np.array([len(y) for y in rows], dtype=np.int64)


# ------------------------------------------------------------------------------------------ criteria
def block_error(v, v64, n_out):
    """Worst block's max |v - v64| / max(block peak of |v64|, 0.1 x the row's rms) over every row's own samples, blocks of 256."""
    worst = 0.0
    for b, L in enumerate(n_out):
        L = int(L)
        if L == 0:
            continue
        ref = v64[b, :L]
        floor = max(0.1 * float(np.sqrt(np.mean(ref * ref))), 1e-30)
        err = np.abs(v[b, :L].astype(np.float64) - ref)
        for s in range(0, L, BLOCK):
            worst = max(worst, float(err[s:s + BLOCK].max()) / max(float(np.abs(ref[s:s + BLOCK]).max()), floor))
    return worst


def padding_is_zero(out, n_out):
    return all(not np.any(out[b, int(L):]) for b, L in enumerate(n_out))


def check(case, out, n_out, v64, bound=None):
    """Every criterion on one result; returns the list of (criterion, figure) that fail (empty: the result passes)."""
    bound = RESAMPLE_BLOCK_BOUND if bound is None else bound
    want = expected_n_out(case)
    if out.shape != v64.shape or not np.array_equal(np.asarray(n_out, dtype=np.int64), want):
        return [("n_out", [int(f) for f in n_out])]
    if not np.all(np.isfinite(out)):
        return [("finite", float("nan"))]
    bad = []
    if not padding_is_zero(out, want):
        bad.append(("padding", 1.0))
    e = block_error(out, v64, want)
    if e > bound:
        bad.append(("block", e))
    return bad
