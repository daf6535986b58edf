"""GPU: enrolled voices (dv_voice_capture / dv_unet_bind_voices, UNetEngine.enroll / bind_voices, NaturalSpeech2.enroll_voice /
sample_from_prior(voices=)) against the path they replace: dv_unet_set_cond on the same prompts.

A voice is a snapshot of what set_cond wrote and a bind copies it back - no arithmetic - so EVERY comparison here is
torch.equal.  The denoiser is the production configuration with synthetic weights at B = 3, T = 64, L = 40 (no multiple of 32:
the last key tile is partial) and prompts of 40 / 17 / 1 valid frames (full, ragged, the one-key edge)."""
import ctypes as C

import numpy as np
import pytest
import torch

from diff_vits_amd import _lib, synth
from diff_vits_amd.engine import Voice

pytestmark = pytest.mark.gpu

KW = dict(in_channels=208, out_channels=80, block_out_channels=(128, 256, 384, 512), norm_num_groups=8, cross_attention_dim=128,
          attention_head_dim=8, addition_embed_type="text", resnet_time_scale_shift="scale_shift")
B, T, L = 3, 64, 40
LENGTHS = (40, 17, 1)


def make_unet():
    from diff_vits_amd.unet1d.unet_1d_condition import UNet1DConditionModel
    with torch.device("meta"):
        shapes = {k: tuple(v.shape) for k, v in UNet1DConditionModel(**KW).state_dict().items()}
    m = UNet1DConditionModel(backend="hip", **KW).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(shapes, seed=7).items()})
    return m.cuda()


def prompts(tag, lengths=LENGTHS, n_keys=L):
    """(enc [n, L, 128] with zero padding frames, bool mask [n, L]) as the prompt encoder hands them over."""
    n = len(lengths)
    mask = torch.arange(n_keys)[None, :] < torch.tensor(lengths)[:, None]
    enc = torch.from_numpy(synth.normal(11, "voices." + tag, (n, n_keys, 128))) * mask.unsqueeze(-1)
    return enc.cuda(), mask.cuda()


def inputs(n, frames):
    x = torch.from_numpy(synth.normal(11, "voices.x", (n, 80, frames))).cuda()
    cond = torch.from_numpy(synth.normal(11, "voices.cond", (n, 128, frames))).cuda()
    t = torch.tensor([949.05, 311.0, 17.5][:n]).cuda()
    return x, cond, t


class Case:
    """One engine, the prompt sets P (the voices) and Q (what clobbers them), and set_cond references computed once."""

    def __init__(self):
        self.m = make_unet()
        self.eng = self.m.hip_engine()
        self.P, self.Pm = prompts("P")
        self.Q, self.Qm = prompts("Q", (23, 40, 8))
        self.x, self.cond, self.t = inputs(B, T)
        self.eng.prepare(B, T, L)
        self.y_P = self.ref(self.P, self.Pm)
        self.y_Q = self.ref(self.Q, self.Qm)
        self.voices = self.eng.enroll(self.P, self.bias(self.Pm))

    def bias(self, mask):
        return self.m._bias_from_mask(mask, torch.float32)

    def ref(self, enc, mask):
        """The oracle: set_cond on the stacked prompts, one forward."""
        self.eng.set_cond(enc, self.bias(mask))
        return self.fwd()

    def fwd(self, x=None, cond=None, t=None):
        y = self.eng.eval(self.x if x is None else x, self.cond if cond is None else cond, self.t if t is None else t)
        torch.cuda.synchronize()
        return y


@pytest.fixture(scope="module")
def case():
    return Case()


def test_round_trip(case):
    eng = case.eng
    assert len(case.voices) == B and all(isinstance(v, Voice) and v.L == L and v.rebuilds == 0 for v in case.voices)
    sig = eng.cond_signature()
    assert sig != 0 and all(v.signature == sig for v in case.voices)
    assert all(v.nbytes > 0 and v.nbytes % 16 == 0 and v.nbytes == case.voices[0].nbytes for v in case.voices)
    eng.prepare(B, T, L)
    serial = eng.cond_serial
    eng.set_cond(case.Q, case.bias(case.Qm))                   # clobber
    eng.bind_voices([0, 1, 2], case.voices)
    assert eng.cond_serial == serial + 2
    assert torch.equal(case.fwd(), case.y_P)
    assert not torch.equal(case.y_P, case.y_Q)


def test_any_row_and_repeats(case):
    eng = case.eng
    eng.prepare(B, T, L)
    order = [2, 0, 2]
    y_ref = case.ref(case.P[order], case.Pm[order])
    eng.set_cond(case.Q, case.bias(case.Qm))
    eng.bind_voices([0, 1, 2], [case.voices[i] for i in order])
    assert torch.equal(case.fwd(), y_ref)


def test_partial_bind_keeps_the_other_rows(case):
    eng = case.eng
    eng.prepare(B, T, L)
    enc, mask = case.Q.clone(), case.Qm.clone()
    enc[1], mask[1] = case.P[1], case.Pm[1]
    y_ref = case.ref(enc, mask)
    eng.set_cond(case.Q, case.bias(case.Qm))
    eng.bind_voices([1], [case.voices[1]])
    y = case.fwd()
    assert torch.equal(y, y_ref)
    assert torch.equal(y[0], case.y_Q[0]) and torch.equal(y[2], case.y_Q[2]) and not torch.equal(y[1], case.y_Q[1])


def test_voices_outlive_their_schedule_and_know_their_weights(monkeypatch):
    """Enrolled one at a time at (B = 1, T = 32), bound at (B = 2, T = 96) on an engine that keeps ONE schedule
    (DVITS_PLAN_CACHE=1, read when the engine is made): the first schedule's native handle is re-planned (its arena freed)
    before the bind.  Then the weight check."""
    monkeypatch.setenv("DVITS_PLAN_CACHE", "1")
    m = make_unet()
    eng = m.hip_engine()
    P, Pm = prompts("P")
    bias = m._bias_from_mask(Pm, torch.float32)
    eng.prepare(1, 32, L)
    voices = [eng.enroll(P[i:i + 1], bias[i:i + 1])[0] for i in (0, 1)]
    eng.prepare(2, 96, L)
    assert eng.plan_builds == 2 and len(eng._plans) == 1       # the (1, 32) schedule is gone
    x, cond, t = inputs(2, 96)
    eng.set_cond(P[:2], bias[:2])
    y_ref = eng.eval(x, cond, t)
    eng.set_cond(P[1:], bias[1:])
    eng.bind_voices([0, 1], voices)
    assert torch.equal(eng.eval(x, cond, t), y_ref)
    assert [v.rebuilds for v in voices] == [0, 0] and voices[0].signature == eng.cond_signature()

    # a weight changed after enrolment: once the engine holds the new weights the voices are
    # refused, naming the row, with nothing launched; the engine works
    with torch.no_grad():
        m.conv_in.bias.add_(0.0)
    eng = m.hip_engine()                                       # (sync_weights: the engine takes the new weights)
    eng.prepare(2, 96, L)
    with pytest.raises(RuntimeError, match="row 0.*weights changed"):
        eng.bind_voices([0, 1], voices)
    eng.set_cond(P[:2], bias[:2])
    assert torch.equal(eng.eval(x, cond, t), y_ref)


def test_layout_change_rebuilds_the_record(case, monkeypatch):
    """DVITS_ATTN_FRAG=0 at prepare time keeps the prompt's K / V of the blocks outside the chain kernel as fp32 rows (+ the
    mask bias) instead of MFMA fragments: another segment table, another signature.  Binding a voice recorded under the
    default layout re-derives its record (one conditioning pass) - also in the middle of a batch whose other rows are kept,
    and without conditioning rows that were not.  (The variable is read per prepare; an engine of this test's own, so that no
    other test meets the fragment-less schedule in a plan cache.)"""
    eng = make_unet().hip_engine()

    def fwd(*a):
        y = eng.eval(*a)
        torch.cuda.synchronize()
        return y

    eng.prepare(B, T, L)
    fresh = eng.enroll(case.P, case.bias(case.Pm))
    old_sig = fresh[0].signature
    monkeypatch.setenv("DVITS_ATTN_FRAG", "0")
    x, cond, t = inputs(B, 48)
    eng.prepare(B, 48, L)
    assert eng.cond_signature() not in (0, old_sig)
    enc, mask = case.Q.clone(), case.Qm.clone()
    enc[1], mask[1] = case.P[1], case.Pm[1]
    eng.set_cond(enc, case.bias(mask))
    y_mixed = fwd(x, cond, t)
    eng.set_cond(case.P, case.bias(case.Pm))
    y_P = fwd(x, cond, t)
    eng.set_cond(case.Q, case.bias(case.Qm))
    eng.bind_voices([1], [fresh[1]])                           # rebuild with rows 0 and 2 saved and restored
    assert torch.equal(fwd(x, cond, t), y_mixed)
    assert [v.rebuilds for v in fresh] == [0, 1, 0] and fresh[1].signature == eng.cond_signature()
    eng.bind_voices([0, 1, 2], fresh)
    assert torch.equal(fwd(x, cond, t), y_P)
    assert [v.rebuilds for v in fresh] == [1, 1, 1]
    eng.bind_voices([2, 1, 0], fresh[::-1])                    # same layout now: no further rebuild
    assert torch.equal(fwd(x, cond, t), y_P) and [v.rebuilds for v in fresh] == [1, 1, 1]

    # a rebuild on a freshly planned schedule: the pass went through rows 0 and 2, but only row 1 is conditioned afterwards
    monkeypatch.delenv("DVITS_ATTN_FRAG")
    eng.prepare(B, T, L)
    late, = eng.enroll(case.P[1:2], case.bias(case.Pm[1:2]))   # knows the default layout only
    monkeypatch.setenv("DVITS_ATTN_FRAG", "0")
    x, cond, t = inputs(B, 80)
    eng.prepare(B, 80, L)
    eng.bind_voices([1], [late])
    assert late.rebuilds == 1 and eng._cond_rows() == [False, True, False]
    y = torch.empty((B, 80, 80), device="cuda")
    assert _lib.lib().dv_unet_forward(eng.handle, _lib.ptr(x), 80, _lib.ptr(cond), _lib.ptr(t), _lib.ptr(y), _lib.stream_ptr()) == -3
    eng.bind_voices([0, 2], [fresh[0], fresh[2]])
    y = fwd(x, cond, t)
    eng.set_cond(case.P, case.bias(case.Pm))
    assert torch.equal(fwd(x, cond, t), y)


def test_another_gemm_tile_is_another_signature():
    """The K / V projections of the cond schedule are GEMMs over M = B x L rows and the launcher picks their tile from the tile
    counts.  Enrolled at B = 1 / L = 256 (M = 256: the small tiles), bound at B = 16 (M = 4096: 128-row tiles, the 128 x 128 x 32
    tile for the wide blocks), a copied record would differ from set_cond in the last bits (measured: the forward is not
    torch.equal) - so the tile is part of the signature: the voices get a second record there, once, and the result is exact;
    back at B = 1 the first record still serves."""
    m = make_unet()
    eng = m.hip_engine()
    n, Lk, frames = 16, 256, 32
    P, Pm = prompts("L256", tuple(256 - 17 * b for b in range(n)), Lk)
    bias = m._bias_from_mask(Pm, torch.float32)
    eng.prepare(1, frames, Lk)
    voices = [eng.enroll(P[i:i + 1], bias[i:i + 1])[0] for i in range(n)]
    sig1, bytes1 = voices[0].signature, voices[0].nbytes
    x = torch.from_numpy(synth.normal(11, "voices.x16", (n, 80, frames))).cuda()
    cond = torch.from_numpy(synth.normal(11, "voices.cond16", (n, 128, frames))).cuda()
    t = torch.linspace(950.0, 20.0, n).cuda()
    eng.set_cond(P[3:4], bias[3:4])
    y1_ref = eng.eval(x[:1], cond[:1], t[:1])

    eng.prepare(n, frames, Lk)
    assert eng.cond_signature() not in (0, sig1)
    eng.set_cond(P, bias)
    y_ref = eng.eval(x, cond, t)
    eng.set_cond(P.flip(0).contiguous(), bias.flip(0).contiguous())
    eng.bind_voices(range(n), voices)
    assert torch.equal(eng.eval(x, cond, t), y_ref)
    assert all(v.rebuilds == 1 and v.nbytes == 2 * bytes1 for v in voices)
    eng.bind_voices(range(n), voices[::-1])
    assert all(v.rebuilds == 1 for v in voices)

    eng.prepare(1, frames, Lk)                                 # the first signature again: its record was kept
    eng.bind_voices([0], [voices[3]])
    assert torch.equal(eng.eval(x[:1], cond[:1], t[:1]), y1_ref) and voices[3].rebuilds == 1


def _native_bind(eng, rows, voices):
    n = len(rows)
    return _lib.lib().dv_unet_bind_voices(eng.handle, (C.c_int32 * n)(*rows), (C.c_void_p * n)(*[v._h.value for v in voices]), n,
                                          _lib.stream_ptr())


def test_refusals_leave_the_engine_as_it_was(case):
    eng, v = case.eng, case.voices
    eng.prepare(B, T, L)
    eng.set_cond(case.Q, case.bias(case.Qm))
    serial = eng.cond_serial
    with pytest.raises(ValueError, match="outside"):
        eng.bind_voices([0, 3], v[:2])
    with pytest.raises(ValueError, match="twice"):
        eng.bind_voices([1, 1], v[:2])
    with pytest.raises(ValueError, match="row 2.*CPU"):
        eng.bind_voices([0, 2], [v[0], Voice(case.P[:1].cpu())])
    with pytest.raises(ValueError):
        eng.bind_voices([0, 1], v)
    # the native layer refuses the same on its own, before it launches anything
    assert _native_bind(eng, [0, 3], v[:2]) == -1 and b"outside" in _lib.lib().dv_last_error()
    assert _native_bind(eng, [0, -1], v[:2]) == -1
    assert _native_bind(eng, [1, 1], v[:2]) == -1 and b"twice" in _lib.lib().dv_last_error()
    assert eng.cond_serial == serial
    assert torch.equal(case.fwd(), case.y_Q)                   # rows 0 and 1 were never touched

    # another key length: another signature (native), a ValueError naming the row (host)
    eng.prepare(B, T, 48)
    assert eng.cond_signature() != v[0].signature
    assert _native_bind(eng, [0], v[:1]) == -1 and b"layout" in _lib.lib().dv_last_error()
    with pytest.raises(ValueError, match="row 0.*L = 40"):
        eng.bind_voices([0, 1], v[:2])

    # a freshly planned schedule with one row bound: forward is a state error until every row is conditioned
    eng.prepare(B, 80, L)
    x, cond, t = inputs(B, 80)
    eng.bind_voices([0], v[:1])
    y = torch.empty((B, 80, 80), device="cuda")
    rc = _lib.lib().dv_unet_forward(eng.handle, _lib.ptr(x), 80, _lib.ptr(cond), _lib.ptr(t), _lib.ptr(y), _lib.stream_ptr())
    assert rc == -3 and b"before" in _lib.lib().dv_last_error()
    with pytest.raises(RuntimeError, match="-3"):
        eng.eval(x, cond, t)
    eng.bind_voices([2, 1], [v[2], v[1]])
    y = case.fwd(x, cond, t)
    eng.set_cond(case.P, case.bias(case.Pm))
    assert torch.equal(case.fwd(x, cond, t), y)

    eng.prepare(B, T, L)                                       # ... and the first schedule still works
    assert torch.equal(case.ref(case.P, case.Pm), case.y_P)


def test_sampler_graph_replays_with_bound_voices(case):
    """3-step DPM-Solver++ as one hipGraph: a run with bound voices equals the run conditioned by set_cond on the same noise,
    again after other voices are bound, and the plan keeps its captured graph (bind writes the addresses set_cond writes)."""
    from diff_vits_amd.sampler import dpm_solver
    ns = dpm_solver.NoiseScheduleVP("discrete", betas=torch.from_numpy(synth.make_betas()))
    nm = dpm_solver.NativeUNetModel(case.m, case.cond, case.P, case.Pm)
    solver = dpm_solver.DPM_Solver(dpm_solver.model_wrapper(nm, ns, model_type="x_start"), ns, algorithm_type="dpmsolver++")

    def run():
        with torch.no_grad():
            out = solver.sample(case.x, steps=3, order=2, skip_type="time_uniform", method="multistep")
        torch.cuda.synchronize()
        return out

    def nodes():
        return [p.graph_nodes() for plan in solver._plans.values() for p in plan._per_shape.values()]

    mel_P = run()
    n0 = nodes()
    assert len(n0) == 1 and n0[0] > 0
    builds = case.eng.plan_builds
    nm.voices = case.voices
    assert torch.equal(run(), mel_P) and nodes() == n0
    order = [1, 2, 0]
    nm.voices = [case.voices[i] for i in order]
    mel_v = run()
    nm.voices, nm.enc, nm.mask = None, case.P[order], case.Pm[order]
    mel_ref = run()
    assert torch.equal(mel_v, mel_ref) and not torch.equal(mel_v, mel_P)
    assert nodes() == n0 and case.eng.plan_builds == builds    # one plan, one graph, never re-captured or re-planned


def test_bind_is_capturable(case):
    eng = case.eng
    eng.prepare(B, T, L)
    eng.set_cond(case.Q, case.bias(case.Qm))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.bind_voices([0, 1, 2], case.voices)
    eng.set_cond(case.Q, case.bias(case.Qm))                   # (whatever the capture left behind is overwritten)
    assert torch.equal(case.fwd(), case.y_Q)
    g.replay()
    assert torch.equal(case.fwd(), case.y_P)


def test_product_voices_equal_refer_and_skip_the_prompt_encoder(gold):
    from test_prompt_cpu import diffusion_state_dict, sample_case
    g, cfg, NaturalSpeech2, content, refer, noise = sample_case(gold)
    m = NaturalSpeech2(cfg, backend="hip").eval()
    m.diff_model.load_state_dict({k: torch.from_numpy(v) for k, v in diffusion_state_dict(cfg["diffusion_encoder"]).items()})
    m = m.cuda()
    content, refer, noise = (torch.from_numpy(a).cuda() for a in (content, refer, noise))
    lengths = torch.from_numpy(g["spec_lengths"]).cuda()
    voices = m.enroll_voice(refer, lengths)
    assert all(v.nbytes > 0 and v.rebuilds == 0 for v in voices)
    calls = []
    pe = m.diff_model.prompt_encoder
    enc_fn = pe.encode_channels_last
    pe.encode_channels_last = lambda *a, **k: (calls.append(1), enc_fn(*a, **k))[1]
    try:
        _, mel_v = m.sample_from_prior(content, voices=voices, sample_method="dpmsolver", noise=noise)
        assert not calls                                       # the voice path never ran the prompt encoder
        _, mel_ref = m.sample_from_prior(content, refer, None, lengths, None, "dpmsolver", noise=noise)
        assert len(calls) == 1
        _, mel_v2 = m.sample_from_prior(content, voices=voices, sample_method="dpmsolver", noise=noise)
        assert len(calls) == 1
    finally:
        del pe.encode_channels_last
    assert torch.isfinite(mel_ref).all() and torch.equal(mel_v, mel_ref) and torch.equal(mel_v2, mel_ref)
    assert all(v.rebuilds == 0 for v in voices)
    with pytest.raises(ValueError, match="guidance"):
        m.sample_from_prior(content, voices=voices, noise=noise, guidance_scale=2.0)
    assert np.isfinite(mel_v.cpu().numpy()).all()
