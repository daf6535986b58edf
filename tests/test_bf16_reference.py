"""CPU: the one-plane emulation of the bf16 fast mode (parity_metrics emulate="bf16") is pinned, and the bounds
tests/test_gpu_bf16_mode.py derives from it have teeth.

(1) emulate=True is untouched by the new mode, and the operand-rounding hook of the oracle probes changes nothing while it is off.
(2) For every stretch between two taps, at the three shapes of the GPU test (inputs: the fp64 oracle's own intermediates), the worst
frame of the emulation against fp64 is printed; the bound is 2 x that + 2^-9, and the whole-forward emulation stays under the
documented 3e-2.  (3) Faults planted in the restatements: each one either exceeds the bound the un-faulted emulation sets on the
stretches named in DETECTED, or is named in NOT_DETECTABLE (profiles/bf16_mode_parity.txt lists them).  (4) The attention cases
reach every k_attention<DP, NW, 1> instantiation.  DVITS_PARITY_REPORT=<file> appends the figures."""
import os

import pytest
import torch

import bf16_cases as bc
from parity_metrics import (BF16_FLOOR, attn_chain_fp64, frame_errors, isolated_bound, one_plane, oracle_probes, sdpa_fp64)

# fault -> the stretch kinds on which it must exceed the bf16 bound, on every block of every shape
DETECTED = {"beta_sign": ("attn1", "attn2", "ff"), "tscale": ("resnet", "resnet+skip"), "skip_stats": ("resnet+skip",), "mask_tail": ("attn2",)}
# faults one plane cannot show: the rounded-row mean moves a frame by about (|mean| / sigma) 2^-9 / sqrt(3 C) of a sigma, two
# orders below the plane's own 2^-9 per operand; fp16 P is MORE accurate than the documented bf16 P, and an upper bound against
# fp64 cannot see an error that is too small
NOT_DETECTABLE = ("mean_from_bf16", "p_fp16")


def _report(header, lines):
    print("# %s\n%s" % (header, "\n".join(lines)))
    path = os.environ.get("DVITS_PARITY_REPORT")
    if path:
        with open(path, "a") as f:
            f.write("# %s\n%s\n" % (header, "\n".join(lines)))


@pytest.fixture(scope="module", params=range(len(bc.SHAPES)), ids=["%dx%d-L%d" % s for s in bc.SHAPES])
def case(request):
    B, T, L = bc.SHAPES[request.param]
    sd = bc.state_dict()
    sample, t, enc, mask = bc.inputs(B, T, L)
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        y64, p64 = oracle_probes(bc.KW, sd64, sample.double(), t.double(), enc.double(), mask)
        y1, _ = oracle_probes(bc.KW, sd64, sample.double(), t.double(), enc.double(), mask, round_operand=one_plane)
    return {"shape": (B, T, L), "sd": sd, "sample": sample, "enc": enc, "mask": mask, "y64": y64, "y1": y1, "pr": p64,
            "stretches": bc.stretches(sd, p64, sample, enc, mask, y64, T)}


def test_attention_shapes_cover_every_plain_instantiation():
    want = {(dp, nw) for dp in (16, 32, 48, 64) for nw in (1, 2, 4, 8)}
    have = {bc.plain_instantiation(B, H, Tq, Tk, d) for B, H, Tq, Tk, d, _, _ in bc.ATTN_PLAIN_SHAPES}
    assert len(want) == 16 and have == want, sorted(want ^ have)
    assert {1, 31, 32, 33, 64, 65, 97, 161} <= {s[3] for s in bc.ATTN_PLAIN_SHAPES}
    assert {1, 31, 33, 300} <= {s[2] for s in bc.ATTN_PLAIN_SHAPES}
    assert {None, "ragged", "one", "all", "tile"} == {s[5] for s in bc.ATTN_PLAIN_SHAPES}
    assert sum(s[6] == 8 for s in bc.ATTN_PLAIN_SHAPES) >= 2 and {4, 8, 12} <= {s[4] for s in bc.ATTN_PLAIN_SHAPES}
    assert all(s[4] % 4 == 0 for s in bc.ATTN_PLAIN_SHAPES)


def test_the_switch_leaves_the_parity_mode_emulation_alone():
    """emulate=True computes what it computed (two planes, fp16 P: its figures stay at the 1e-5 class, two orders below one plane),
    and the hook's default leaves oracle_probes' outputs bit for bit."""
    from diff_vits_amd import synth
    sd = bc.state_dict()
    tb = "down_blocks.0.attentions.0.transformer_blocks.0."
    sample, t, enc, mask = bc.inputs(2, 40, 20)
    x = torch.from_numpy(synth.normal(5, "bf16.x", (2, 40, 128)))
    want = attn_chain_fp64(sd, tb, "attn2", x, 8, enc, mask)
    two, one = (frame_errors(attn_chain_fp64(sd, tb, "attn2", x, 8, enc, mask, emulate=e), want)["worst"] for e in (True, "bf16"))
    assert two < 1e-4 < 20 * two < one < 2e-2, (two, one)
    assert isolated_bound(want, want, "bf16") == BF16_FLOOR and isolated_bound(want, want) == 1e-4
    with torch.no_grad():
        a = oracle_probes(bc.KW, sd, sample, t, enc, mask)
        b = oracle_probes(bc.KW, sd, sample, t, enc, mask, round_operand=None)
    assert torch.equal(a[0], b[0]) and all(torch.equal(a[1][k], b[1][k]) for k in a[1])


def test_a_single_valid_key_makes_the_emulation_exact():
    """The floor's argument: q, k, v held exactly by one plane and one valid key -> P = 1 exactly, o = v."""
    q, k, v, bias = bc.attention_case(2, 8, 33, 65, 16, "one", 1)
    want = sdpa_fp64(q, k, v, 8, bias)
    assert frame_errors(sdpa_fp64(q, k, v, 8, bias, emulate="bf16"), want)["worst"] < 1e-12


def test_emulation_figures_per_stretch(case):
    """What sets every bound of the GPU test, printed per stretch; the restatements agree with the oracle in fp64 (the new
    conv_in / resampler / conv_out ones included), and the whole-forward emulation stays under the documented 3e-2."""
    lines = []
    for name, kind, want, fn in case["stretches"]:
        ref = fn(False)
        assert frame_errors(ref, want)["worst"] < 1e-11, name
        emu = frame_errors(fn("bf16"), ref)
        bound = isolated_bound(fn("bf16"), ref, "bf16")
        assert emu["floored_ok"] and emu["worst"] < bound < 0.1, (name, emu["worst"], bound)
        lines.append("%-52s %-11s emulation tensor %.2e worst frame %.2e at %s; bound %.2e" % (name, kind, emu["rel_l2"], emu["worst"], emu["at"], bound))
    cl = lambda v: v.permute(0, 2, 1).contiguous()    # noqa: E731
    whole = frame_errors(cl(case["y1"]), cl(case["y64"]))
    lines.append("%-52s %-11s emulation tensor %.2e worst frame %.2e at %s; bound %.2e (tensor: 3e-2)" %
                 ("y (whole forward, every operand one plane)", "forward", whole["rel_l2"], whole["worst"], whole["at"], 2 * whole["worst"]))
    _report("one-plane emulation vs fp64, cfg1 B=%d T=%d L=%d (inputs: the fp64 oracle's intermediates)" % case["shape"], lines)
    assert whole["rel_l2"] < 3e-2 and whole["floored_ok"], whole["rel_l2"]


def _fault_table(case):
    rows = {}
    for name, kind, _, fn in case["stretches"]:
        faults = {"attn1": ("beta_sign", "mean_from_bf16", "p_fp16"), "attn2": ("beta_sign", "mean_from_bf16", "mask_tail", "p_fp16"),
                  "ff": ("beta_sign", "mean_from_bf16"), "resnet": ("tscale",), "resnet+skip": ("tscale", "skip_stats")}.get(kind, ())
        if not faults:
            continue
        ref = fn(False)
        bound = isolated_bound(fn("bf16"), ref, "bf16")
        for f in faults:
            rows.setdefault((f, kind), []).append((name, frame_errors(fn("bf16", fault=f), ref)["worst"], bound))
    return rows


def test_planted_faults_exceed_the_bound_or_are_listed(case):
    """Every block of every shape; at L = 33 the last 32-key sub-tile holds ONE key.  mask_tail is planted where the mask has a
    masked key in that sub-tile (the B = 1 shape has none: utterance 0 is all valid).  The table goes to the report."""
    rows = _fault_table(case)
    L = case["shape"][2]
    if not bool((~case["mask"][:, (L - 1) // 32 * 32:]).any()):
        rows = {k: v for k, v in rows.items() if k[0] != "mask_tail"}
    lines, missed = [], []
    for (f, kind), items in sorted(rows.items()):
        seen = sum(w > b for _, w, b in items)
        worst_margin = min(w / b for _, w, b in items)
        lines.append("%-15s %-12s exceeds the bound on %2d of %2d stretches; smallest fault / bound %.2f" % (f, kind, seen, len(items), worst_margin))
        if f in NOT_DETECTABLE:
            continue
        assert kind in DETECTED[f], (f, kind)
        missed += [(f, n, w, b) for n, w, b in items if not w > b]
    _report("planted faults at one plane, cfg1 B=%d T=%d L=%d; not detectable at one plane: %s" % (case["shape"] + (", ".join(NOT_DETECTABLE),)), lines)
    assert not missed, missed[:6]
