"""The restatements the alignment tests trust, and their cases (forced alignment: VITS.align, dv_op_mas_scores / dv_op_mas_path,
csrc/kernels_align.hip).  Shared by tests/test_align_cpu.py and tests/test_gpu_align.py.

THE SEARCH (search_ref), for one utterance with 1 <= t_x <= t_y, in float32 with ONE addition per cell:
  forward   rows y = 0 .. t_y - 1, columns x = max(0, t_x + y - t_y) .. min(t_x - 1, y):  Q[y][x] = V[y][x] + max(P, C),
            C = Q[y-1][x] (-1e9 when x == y), P = Q[y-1][x-1] (x == 0: 0 in row 0, -1e9 below);
  backward  idx = t_x - 1; from y = t_y - 1 down, frame y belongs to idx, then idx decreases by one iff
            idx != 0 and (idx == y or Q[y-1][idx] < Q[y-1][idx-1]) - strict, a tie stays on the token.
Python loops over the rows, numpy over the columns; the whole table is kept (cells outside the band keep V, as in the
reference, and are never compared).  The integers must be IDENTICAL to this, not close.

THE SCORES (scores_ref) in float64 on the float32 inputs, with the magnitude the bound scales with:
  bound = (C + 6) * 2^-23 * sum_c(|K| + |logs| + |z^2 s / 2| + |z m s| + |m^2 s / 2|),  K = -0.5 log 2 pi, s = exp(-2 logs):
a summand of the kernel passes through at most 2 roundings in s (expf: one ulp, counted twice), 1 in its product, C in its running
sum and 3 in the final additions (the order is in the kernel's header comment), each at most 2^-24 relative to a partial sum that
the sum of the magnitudes bounds; 2^-23 per rounding leaves the second-order terms a factor of two.

ALL-ZERO SCORES: every in-band Q is 0, so no comparison is ever strictly smaller and the walk leaves a token only where it is
forced to (idx == y).  Walking down from (t_y - 1, t_x - 1) it stays on the last token until y = t_x - 1 and then steps every row:
tokens 0 .. t_x - 2 take one frame each and the LAST token takes the remaining t_y - t_x + 1, durations [1, ..., 1, t_y - t_x + 1].

THE GOLDEN CASE (tests/golden/align_forward.npz): its smallest decision margin - the smallest |Q[y-1][idx] - Q[y-1][idx-1]| the walk
compares - is 1.16, against a largest score bound of 0.038 and float32 scores (the reference's own) that lie within 2.4e-4 of the
float64 ones.  A perturbation of every score by eps moves every Q by at most (y + 1) eps, so scores that far from exact move a
compared difference by at most 2 * 40 * 2.4e-4 = 0.02: test_align_cpu.py asserts the margin above 20 times the score bound and
above 20 times that figure.  No fp32-vs-fp64 or CPU-vs-GPU difference of the scores turns a decision there (the text encoder's
output projection carries a gain in this fixture for exactly that: seeded weights alone give near-ties).  The GPU's end-to-end
test is nevertheless exact by construction: the restated search on the kernel's own scores.
"""
import math

import numpy as np

from diff_vits_amd import synth

NEG = np.float32(-1e9)
LDS_LIMIT_TY = 1024          # at Tx = 512 (64 bytes of decision bits per row) the bits stay in LDS up to this many frames
MAX_TX = 512


def search_one(V, ty, tx, fault=None):
    """-> (frame_token int32 [ty], smallest margin of a compared decision).  fault: None | 'tie' | 'sentinel' | 'band'."""
    Q = np.array(V[:ty, :tx], dtype=np.float32, copy=True)
    cols = np.arange(tx)
    for y in range(ty):
        lo, hi = max(0, tx + y - ty), min(tx - 1, y)
        if fault == "band":
            lo = min(lo + 1, hi)                                     # the band's lower edge off by one
        x = cols[lo:hi + 1]
        if y == 0:
            C = np.full(len(x), NEG, np.float32)
            P = np.zeros(len(x), np.float32)
        else:
            C = Q[y - 1, x].copy()
            if fault != "sentinel":
                C[x == y] = NEG
            P = np.where(x == 0, NEG, Q[y - 1, np.maximum(x - 1, 0)]).astype(np.float32)
        Q[y, lo:hi + 1] = (V[y, lo:hi + 1].astype(np.float32) + np.maximum(P, C)).astype(np.float32)
    token = np.empty(ty, np.int32)
    idx, margin = tx - 1, math.inf
    for y in range(ty - 1, -1, -1):
        token[y] = idx
        if idx != 0:
            if idx == y:
                idx -= 1
            else:
                a, b = Q[y - 1, idx], Q[y - 1, idx - 1]
                margin = min(margin, abs(float(a) - float(b)))
                if (a <= b) if fault == "tie" else (a < b):
                    idx -= 1
    return token, margin


def search_ref(neg_cent, y_len, x_len, fault=None):
    """neg_cent float32 [B, Ty, Tx] -> (durations int32 [B, Tx], frame_token int32 [B, Ty], smallest decision margin).  An
    utterance with t_x < 1, t_y < 1, t_x > t_y or a length beyond the padded dimensions: both rows all -1."""
    B, Ty, Tx = neg_cent.shape
    dur = np.zeros((B, Tx), np.int32)
    tok = np.full((B, Ty), -1, np.int32)
    margin = math.inf
    for b in range(B):
        ty, tx = int(y_len[b]), int(x_len[b])
        if tx < 1 or ty < 1 or tx > ty or tx > Tx or ty > Ty:
            dur[b] = -1
            continue
        tok[b, :ty], m = search_one(neg_cent[b], ty, tx, fault)
        margin = min(margin, m)
        dur[b, :tx] = np.bincount(tok[b, :ty], minlength=tx)
    return dur, tok, margin


def scores_ref(z, m_p, logs_p, y_len, x_len, fault=None):
    """float64 scores [B, Ty, Tx] (zeros outside an utterance) and the per-cell bound.  fault: None | 'term' | 'shift'."""
    z, m, logs = (np.asarray(a, np.float64) for a in (z, m_p, logs_p))
    if fault == "shift":
        m, logs = np.roll(m, 1, axis=2), np.roll(logs, 1, axis=2)    # every token column shifted by one
    B, C, Ty = z.shape
    Tx = m.shape[2]
    K = -0.5 * math.log(2 * math.pi)
    s = np.exp(-2 * logs)
    t1 = (K - logs).sum(1)[:, None, :]
    t2 = np.einsum("bcy,bcx->byx", -0.5 * z * z, s)
    t3 = np.einsum("bcy,bcx->byx", z, m * s)
    t4 = (-0.5 * m * m * s).sum(1)[:, None, :]
    out = t1 + t2 + t3 + (0 if fault == "term" else t4)
    mag = ((abs(K) + np.abs(logs)).sum(1)[:, None, :] + np.einsum("bcy,bcx->byx", 0.5 * z * z, s)
           + np.einsum("bcy,bcx->byx", np.abs(z), np.abs(m) * s) + (0.5 * m * m * s).sum(1)[:, None, :])
    inside = (np.arange(Ty)[None, :, None] < np.asarray(y_len)[:, None, None]) & (np.arange(Tx)[None, None, :] < np.asarray(x_len)[:, None, None])
    return out * inside, (C + 6) * 2.0 ** -23 * mag * inside


def score_inputs(name, B, C, Ty, Tx):
    """z, m_p, logs_p in the ranges the prior produces (unit-scale means, log-deviations around -0.5)."""
    z = synth.normal(77, name + ".z", (B, C, Ty))
    m_p = synth.normal(77, name + ".m", (B, C, Tx))
    logs_p = (synth.normal(77, name + ".logs", (B, C, Tx), std=0.4) - np.float32(0.5)).astype(np.float32)
    return z, m_p, logs_p


# name: (C, Ty, Tx, y_len, x_len)
SCORE_CASES = {
    "small": (128, 40, 12, [40, 31], [12, 9]),
    "tile_edge": (128, 65, 64, [65, 64], [64, 63]),
    "ragged": (128, 130, 70, [130, 97, 64], [70, 65, 1]),
}


def _normal(name, shape, scale=3.0):
    return (synth.normal(99, "mas." + name, shape) * np.float32(scale)).astype(np.float32)


def _single(name, ty, tx, scale=3.0, Ty=None, Tx=None):
    Ty, Tx = Ty or ty, Tx or tx
    return dict(V=_normal(name, (1, Ty, Tx), scale), y_len=[ty], x_len=[tx])


# each is the smallest that crosses one boundary of the search kernel (lane = 8 columns, wave = 512 columns, LDS / scratch bits)
SEARCH_CASES = {
    "one_cell": lambda: _single("one_cell", 1, 1),
    "never_steps": lambda: _single("never_steps", 5, 1),
    "all_forced": lambda: _single("all_forced", 7, 7),
    "lane_last_column": lambda: _single("lane_last_column", 9, 8),
    "lane_first_column": lambda: _single("lane_first_column", 10, 9),
    "across_lanes_64": lambda: _single("across_lanes_64", 70, 64),
    "across_lanes_65": lambda: _single("across_lanes_65", 70, 65),
    "tx_511": lambda: _single("tx_511", 600, 511),
    "tx_512": lambda: _single("tx_512", 600, 512),
    "bits_in_lds_limit": lambda: _single("bits_in_lds_limit", LDS_LIMIT_TY, 500, Tx=MAX_TX),
    "bits_in_scratch": lambda: _single("bits_in_scratch", LDS_LIMIT_TY + 1, 500, Tx=MAX_TX),
    "ragged": lambda: dict(V=_normal("ragged", (3, 50, 20)), y_len=[41, 30, 47], x_len=[13, 17, 5]),
    "all_zero": lambda: dict(V=np.zeros((1, 12, 5), np.float32), y_len=[12], x_len=[5]),
    "huge_scores": lambda: _single("huge_scores", 40, 12, scale=1e6),
    "refused_between": lambda: dict(V=_normal("refused_between", (3, 30, 16)), y_len=[30, 9, 22], x_len=[11, 10, 16]),
}


def make_search_case(name):
    c = SEARCH_CASES[name]()
    c["V"] = np.ascontiguousarray(c["V"], np.float32)
    c["y_len"], c["x_len"] = np.array(c["y_len"], np.int64), np.array(c["x_len"], np.int64)
    return c


_REF = {}


def search_reference(name):
    """(durations, frame_token, margin) of a case, computed once and shared."""
    if name not in _REF:
        c = make_search_case(name)
        _REF[name] = search_ref(c["V"], c["y_len"], c["x_len"])
    return _REF[name]


def check_path(dur, tok, y_len, x_len):
    """What every alignment satisfies: valid utterances have durations >= 1 over their tokens that sum to t_y, zeros behind,
    a non-decreasing frame_token from 0 to t_x - 1 and -1 behind; a refused utterance is all -1."""
    B, Tx = dur.shape
    Ty = tok.shape[1]
    for b in range(B):
        ty, tx = int(y_len[b]), int(x_len[b])
        if tx < 1 or ty < 1 or tx > ty or tx > Tx or ty > Ty:
            assert (dur[b] == -1).all() and (tok[b] == -1).all(), b
            continue
        assert (dur[b, :tx] >= 1).all() and dur[b, :tx].sum() == ty and (dur[b, tx:] == 0).all(), (b, dur[b])
        assert tok[b, 0] == 0 and tok[b, ty - 1] == tx - 1 and (np.diff(tok[b, :ty]) >= 0).all() and (np.diff(tok[b, :ty]) <= 1).all()
        assert (tok[b, ty:] == -1).all()
