"""GPU: the host paths of the three encoder engines (dv_tenc_*, dv_qenc_*, dv_penc_*) that no parity test reaches: a missing
weight, a shape mismatch, the argument checks of set_weight, a re-plan that keeps the packed weights, a weight changed in
place, the probe calls, the stats.  Written against the public Python classes and the C ABI through ctypes alone.

Shapes are the smallest the engines accept:
  text encoder       H = 64, 2 heads (d = 32), filter 64, 2 layers, k = 3, window 4, gin 32 in front of layer 1, out 16, vocab 20;
                     B = 2, T = 33 then T = 5, lengths [T, T - 3]
  posterior encoder  H = 256 (the only instantiated width), k = 5, 2 layers, in 20, out 16, gin 32; B = 2, T = 65 then 64 (one
                     frame past a 64-row tile, exactly one tile), lengths [T, T - 3]
  prompt encoder     flavour D of tests/prompt_cases.py (100 -> 128 -> 128, 8 heads) with n_layers = 1; B = 2, L = 40 then 24
                     (a second length of its own choosing: the issue names one), lengths [L, L - 3]
Weights: synth.make_state_dict on the module's own shapes (the generator of the *_cases modules), weight norm as in
tests/qenc_cases.py.  Bounds: those of tests/test_gpu_tenc.py / test_gpu_qenc.py / test_gpu_prompt.py (whole tensor < 2e-4, padding
exactly zero; the posterior encoder also every frame < FRAME_BOUND).

Run-to-run determinism, measured on the commit before the engines shared their host core (profiles/engine_lifecycle.txt): all
three schedules repeat bit for bit, so "equal" below means torch.equal."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import parity_metrics as pm
from conftest import ROOT, rel_l2
from diff_vits_amd import _lib, synth

pytestmark = pytest.mark.gpu

OK, INVALID, MISSING = 0, -1, -4          # DV_OK, DV_ERR_INVALID, DV_ERR_MISSING_WEIGHT (include/dvits_hip.h)
# dv_*_stats of the commit before the refactor: {kind: {(B, T): (launches, flops)}} (profiles/engine_lifecycle.txt)
STATS = {
    "tenc": {(2, 33): (19, 12207104.0), (2, 5): (19, 1713152.0)},
    "qenc": {(2, 65): (6, 395497472.0), (2, 64): (6, 389414912.0)},
    "penc": {(2, 40): (11, 121651200.0), (2, 24): (11, 72597504.0)},
}


def _seeded(module, seed=77):
    """Seeded weights for `module`'s own state dict; weight-normed convolutions get g = ||v|| per output channel."""
    shapes = {(k[:-2] if k.endswith(".weight_v") else k): tuple(v.shape) for k, v in module.state_dict().items() if not k.endswith(".weight_g")}
    sd = {}
    for k, v in synth.make_state_dict(shapes, seed=seed).items():
        if k + "_v" in module.state_dict():
            sd[k + "_v"] = torch.from_numpy(v)
            sd[k + "_g"] = torch.from_numpy(np.sqrt((v.astype(np.float64) ** 2).sum((1, 2), keepdims=True)).astype(np.float32))
        else:
            sd[k] = torch.from_numpy(v)
    module.load_state_dict(sd)
    return module.eval()


def _rand(shape, tag, std=1.0):
    return torch.from_numpy(synth.normal(77, tag, shape, std=std)).cuda()


class Tenc:
    abi, shapes = "dv_tenc", ((2, 33), (2, 5))
    missing, changed, probe_out = "encoder.attn_layers.1.conv_o.weight", "encoder.ffn_layers.0.conv_1.weight", "proj"

    def module(self, backend):
        from diff_vits_amd.model3 import Encoder, TextEncoder
        m = TextEncoder(20, 16, 64, 64, 2, 2, 3, 0.0, gin_channels=0, n_tones=11, n_languages=3, backend=backend)
        m.encoder = Encoder(64, 64, 2, 2, 3, 0.0, window_size=4, gin_channels=32, cond_layer_idx=1)   # (the ctor's own default is layer 2)
        return m

    def cfg(self):
        return _lib.TencCfg(20, 11, 3, 64, 64, 16, 2, 2, 3, 4, 32, 1)

    def weights(self, m):
        return {k: v.detach().float().contiguous() for k, v in m.state_dict().items()}

    def inputs(self, B, T):
        idx = lambda tag, n: ((_rand((B, T), "te." + tag).abs() * 7).long() % n).contiguous()       # noqa: E731
        return dict(ids=idx("ids", 20), tone=idx("tone", 11), lang=idx("lang", 3), lengths=torch.tensor([T, T - 3]).cuda(),
                    g=_rand((B, 32, 1), "te.g"))

    def run(self, m, i):
        return m(i["ids"], i["lengths"], i["tone"], i["lang"], i["g"])[:3]

    def run_raw(self, h, i):
        B, T = i["ids"].shape
        x, m, logs = torch.empty((B, 64, T)).cuda(), torch.empty((B, 16, T)).cuda(), torch.empty((B, 16, T)).cuda()
        g = i["g"].reshape(B, 32).contiguous()
        rc = _lib.lib().dv_tenc_forward(h, _lib.ptr(i["ids"]), _lib.ptr(i["tone"]), _lib.ptr(i["lang"]), _lib.ptr(i["lengths"]), _lib.ptr(g),
                                        _lib.ptr(x), _lib.ptr(m), _lib.ptr(logs), _lib.stream_ptr())
        return rc, (x, m, logs)

    def within(self, got, want, lengths):
        for a, b in zip(got, want):
            r = rel_l2(a.cpu().numpy(), b.cpu().numpy())
            print("rel_l2 %.3e" % r)
            assert a.shape == b.shape and r < 2e-4, r
            for n, row in zip(lengths.tolist(), a):
                assert bool((row[:, n:] == 0).all()), "a padding frame is not zero"

    def probe_want(self, out):
        return torch.cat([out[1], out[2]], 1).transpose(1, 2)

    def planes_probe(self, m_t, i):
        """('layer0.ffn1', the torch route's relu(conv_1) of layer 0 under the mask [B, T, F]): the one probe kept as hi / lo planes."""
        kept = {}
        h = m_t.encoder.ffn_layers[0].conv_1.register_forward_hook(lambda mod, inp, out: kept.update(v=torch.relu(out)))
        with torch.no_grad():
            self.run(m_t, i)
        h.remove()
        T = i["ids"].shape[1]
        mask = (torch.arange(T).cuda()[None, :] < i["lengths"][:, None]).float()
        return "layer0.ffn1", (kept["v"] * mask[:, None, :]).transpose(1, 2)


class Qenc(Tenc):
    abi, shapes = "dv_qenc", ((2, 65), (2, 64))
    missing, changed, probe_out = "enc.in_layers.1.weight_v", "enc.in_layers.0.weight_g", "proj"
    planes_probe = None

    def module(self, backend):
        from diff_vits_amd.model3 import PosteriorEncoder
        return PosteriorEncoder(20, 16, 256, 5, 1, 2, gin_channels=32, backend=backend)

    def cfg(self):
        return _lib.QencCfg(20, 16, 256, 5, 1, 2, 32)

    def inputs(self, B, T):
        return dict(y=_rand((B, 20, T), "qe.y"), lengths=torch.tensor([T, T - 3]).cuda(), g=_rand((B, 32, 1), "qe.g", 0.5),
                    noise=_rand((B, 16, T), "qe.noise"))

    def run(self, m, i):
        return m(i["y"], i["lengths"], i["g"], noise=i["noise"])[:3]

    def run_raw(self, h, i):
        B, _, T = i["y"].shape
        out = torch.empty((3, B, 16, T)).cuda()
        g = i["g"].reshape(B, 32).contiguous()
        rc = _lib.lib().dv_qenc_forward(h, _lib.ptr(i["y"]), _lib.ptr(i["lengths"]), _lib.ptr(g), _lib.ptr(i["noise"]), _lib.ptr(out[0]),
                                        _lib.ptr(out[1]), _lib.ptr(out[2]), _lib.stream_ptr())
        return rc, (out[0], out[1], out[2])

    def within(self, got, want, lengths):
        for a, b in zip(got, want):
            fe = pm.masked_frame_errors(a.transpose(1, 2).cpu().numpy(), b.transpose(1, 2).cpu().numpy(), lengths.cpu().numpy())
            print("tensor %.3e, worst frame %.3e" % (fe["rel_l2"], fe["worst"]))
            assert fe["padding_zero"], fe["first_nonzero"]
            assert fe["rel_l2"] < 2e-4 and fe["worst"] < pm.FRAME_BOUND


class Penc(Tenc):
    abi, shapes = "dv_penc", ((2, 40), (2, 24))
    missing, changed, probe_out = "layers.0.op.self_attn.out_proj.weight", "layers.0.op.ffn.ffn_2.weight", None

    def module(self, backend):
        from diff_vits_amd.model3 import PromptEncoder
        return PromptEncoder(100, 128, 128, 1, 0.2, backend=backend or "torch")

    def cfg(self):
        return _lib.PencCfg(100, 128, 128, 1, 8, 9)

    def weights(self, m):
        """As PromptEncoderEngine hands them over: ConvTBC [1, C_in, C_out] -> [C_out, C_in] (include/dvits_hip.h)."""
        return {k: (v[0].t() if k.endswith("conv.weight") else v).detach().float().contiguous() for k, v in m.state_dict().items()}

    def inputs(self, B, L):
        lengths = torch.tensor([L, L - 3]).cuda()
        return dict(prompt=_rand((B, 100, L), "pe.prompt"), lengths=lengths,
                    keep=(torch.arange(L).cuda()[None, :] < lengths[:, None]).float().contiguous())

    def run(self, m, i):
        return (m.encode_channels_last(i["prompt"], i["lengths"]).transpose(1, 2),)

    def run_raw(self, h, i):
        B, _, L = i["prompt"].shape
        out = torch.empty((B, L, 128)).cuda()
        rc = _lib.lib().dv_penc_forward(h, _lib.ptr(i["prompt"]), _lib.ptr(i["keep"]), _lib.ptr(out), _lib.stream_ptr())
        return rc, (out.transpose(1, 2),)

    def planes_probe(self, m_t, i):
        """('out_proj', the torch route's out_proj under the mask [B, L, C]): an intermediate, not an output."""
        kept = {}
        h = m_t.out_proj.register_forward_hook(lambda mod, inp, out: kept.update(v=out))
        with torch.no_grad():
            self.run(m_t, i)
        h.remove()
        return "out_proj", kept["v"].permute(1, 0, 2) * i["keep"][:, :, None]


KINDS = {"tenc": Tenc(), "qenc": Qenc(), "penc": Penc()}
_SHARED = {}


@pytest.fixture(params=sorted(KINDS))
def kind(request):
    """(name, kind, native module, torch-route module with the same weights, inputs per shape): built once per kind and shared -
    a test that changes a weight changes it back."""
    name = request.param
    if name not in _SHARED:
        k = KINDS[name]
        native = _seeded(k.module("hip")).cuda()
        plain = k.module(None).eval()
        plain.load_state_dict(native.state_dict())
        _SHARED[name] = (name, k, native, plain.cuda(), [k.inputs(*s) for s in k.shapes])
    return _SHARED[name]


def _fn(k, what):
    return getattr(_lib.lib(), "%s_%s" % (k.abi, what))


def _err():
    return _lib.lib().dv_last_error().decode()


class Raw:
    """One native handle through the C ABI alone."""

    def __init__(self, k, weights=None, skip=()):
        self.k, self.h = k, C.c_void_p()
        assert _fn(k, "create")(C.byref(k.cfg()), C.byref(self.h)) == OK, _err()
        for name, t in (weights or {}).items():
            if name not in skip and not name.startswith("g_proj."):
                assert self.set(name, t) == OK, _err()

    def set(self, name, t, shape=None, ndim=None, null=False):
        shape = list(t.shape) if shape is None else shape
        arr = (C.c_int64 * max(len(shape), 1))(*shape)
        return _fn(self.k, "set_weight")(self.h, name.encode(), None if null else _lib.ptr(t), arr, len(shape) if ndim is None else ndim)

    def prepare(self, B, T):
        return _fn(self.k, "prepare")(self.h, B, T, _lib.PREC_BF16X3)

    def run(self, i):
        rc, out = self.k.run_raw(self.h, i)
        assert rc == OK, _err()
        torch.cuda.synchronize()
        return out

    def stats(self):
        n, f = C.c_int64(), C.c_double()
        assert _fn(self.k, "stats")(self.h, C.byref(n), C.byref(f)) == OK, _err()
        return n.value, f.value

    def close(self):
        torch.cuda.synchronize()
        _fn(self.k, "destroy")(self.h)


def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_missing_weight_is_named_and_the_handle_recovers(kind):
    name, k, native, plain, inputs = kind
    B, T = k.shapes[0]
    w = {n: t.cuda() for n, t in k.weights(native).items()}
    r = Raw(k, w, skip=(k.missing,))
    assert r.prepare(B, T) == MISSING and _err() == "missing weight: " + k.missing, _err()
    assert r.set(k.missing, w[k.missing]) == OK and r.prepare(B, T) == OK, _err()
    fresh = Raw(k, w)
    assert fresh.prepare(B, T) == OK, _err()
    assert _equal(r.run(inputs[0]), fresh.run(inputs[0]))
    # one element column too many
    wrong = torch.zeros((w[k.missing].shape[0], w[k.missing].shape[1] + 1) + tuple(w[k.missing].shape[2:])).cuda()
    assert r.set(k.missing, wrong) == OK, _err()
    assert r.prepare(B, T) == MISSING and _err() == "weight shape mismatch: " + k.missing, _err()
    r.close()
    fresh.close()


def test_set_weight_argument_checks(kind):
    """dv_tenc / dv_qenc always refused a zero dimension; dv_penc (and dv_unet, whose set_weight it shares: the next test) do since
    the engines share one set_weight body - for those two the last assertion is the one of this file that the commit before
    does not pass."""
    name, k, native, plain, inputs = kind
    r = Raw(k)
    t = torch.ones((4, 4)).cuda()
    assert r.set("w", t, ndim=0) == INVALID and "bad argument" in _err()
    assert r.set("w", t, shape=[1, 1, 1, 4, 4]) == INVALID and "bad argument" in _err()
    assert r.set("w", t, null=True) == INVALID and "bad argument" in _err()
    assert r.set("w", t, shape=[4, 0]) == INVALID and "non-positive dimension" in _err(), _err()
    r.close()


def test_unet_set_weight_rejects_a_zero_dimension():
    """The denoiser handle's set_weight is the same body (new with the shared core, like dv_penc's)."""
    from conftest import UNET_CASES
    from diff_vits_amd.unet1d.unet_1d_condition import UNet1DConditionModel
    from diff_vits_amd.engine import UNetEngine
    eng = UNetEngine(UNet1DConditionModel(backend="hip", **UNET_CASES["tiny"][0]))       # (a handle; nothing is uploaded)
    t = torch.ones((4, 4)).cuda()
    rc = _lib.lib().dv_unet_set_weight(eng.handle, b"w", _lib.ptr(t), (C.c_int64 * 2)(4, 0), 2)
    assert rc == INVALID and "non-positive dimension" in _err(), _err()


def test_replan_keeps_the_weights(kind):
    name, k, native, plain, inputs = kind
    with torch.no_grad():
        first = [t.clone() for t in k.run(native, inputs[0])]
        again = [t.clone() for t in k.run(native, inputs[0])]
        assert _equal(first, again), "the schedule does not repeat bit for bit"
        other = k.run(native, inputs[1])
        k.within(other, k.run(plain, inputs[1]), inputs[1]["lengths"])
        third = k.run(native, inputs[0])
    torch.cuda.synchronize()
    assert _equal(first, third)


def test_weight_changed_in_place_is_seen(kind):
    name, k, native, plain, inputs = kind
    params = [dict(m.named_parameters())[k.changed] for m in (native, plain)]
    with torch.no_grad():
        before = [t.clone() for t in k.run(native, inputs[0])]
        for p in params:
            p.mul_(1.5)
        try:
            after = [t.clone() for t in k.run(native, inputs[0])]
            k.within(after, k.run(plain, inputs[0]), inputs[0]["lengths"])
            assert not any(torch.equal(a, b) for a, b in zip(after, before))
        finally:
            for p in params:
                p.div_(1.5)
        k.within(k.run(native, inputs[0]), k.run(plain, inputs[0]), inputs[0]["lengths"])


def test_probes(kind, monkeypatch):
    name, k, native, plain, inputs = kind
    monkeypatch.setenv("DVITS_KEEP_INTERMEDIATES", "1")
    fresh = k.module("hip").eval()
    fresh.load_state_dict(native.state_dict())
    fresh = fresh.cuda()
    i = inputs[0]
    B, T = k.shapes[0]
    with torch.no_grad():
        out = k.run(fresh, i)
    eng, probe = fresh.hip_engine(), _fn(k, "probe")
    checks = []
    if k.probe_out:
        checks.append((k.probe_out, k.probe_want(out), True))
    if k.planes_probe:
        checks.append(k.planes_probe(plain, i) + (False,))
    for pname, want, exact in checks:
        dims = (C.c_int64 * 3)()
        assert probe(eng._h, pname.encode(), None, 0, dims) == OK and list(dims) == [B, T, want.shape[2]], (_err(), list(dims))
        small = torch.empty(want.numel() - 1)
        assert probe(eng._h, pname.encode(), C.c_void_p(small.data_ptr()), small.numel(), dims) == INVALID and _err() == "probe buffer too small"
        got = eng.probe(pname)
        if exact:
            assert torch.equal(got, want.cpu())
        else:
            r = rel_l2(got.numpy(), want.cpu().numpy())
            print("%s: rel_l2 %.3e" % (pname, r))
            assert r < 2e-4, (pname, r)
    assert probe(eng._h, b"nope", None, 0, (C.c_int64 * 3)()) == INVALID
    assert _err() == "no probe named nope (prepare with DVITS_KEEP_INTERMEDIATES=1)", _err()


def test_stats_are_those_of_the_copied_engines(kind):
    name, k, native, plain, inputs = kind
    r = Raw(k, {n: t.cuda() for n, t in k.weights(native).items()})
    for shape in k.shapes:
        assert r.prepare(*shape) == OK, _err()
        got = r.stats()
        print("%s %s: %d launches, %.1f flops" % (name, shape, got[0], got[1]))
        assert got == STATS[name][shape], (name, shape, got)
    r.close()


_SYNC_CHILD = """
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import torch
import test_gpu_engine_lifecycle as L
k = L.KINDS[sys.argv[1]]
m = L._seeded(k.module("hip")).cuda()
with torch.no_grad():
    k.run(m, k.inputs(*k.shapes[0]))
torch.cuda.synchronize()
print("launches", m.hip_engine().stats()[0])
"""


@pytest.mark.parametrize("name,what", [("tenc", "text encoder"), ("qenc", "posterior encoder")])
def test_sync_ops_announces_every_launch(name, what):
    """DVITS_SYNC_OPS=1 (read once per process: a child of its own) names every operation of a forward on stderr - since the
    engines share run_ops the two newer ones do too."""
    env = dict(os.environ, DVITS_SYNC_OPS="1")
    p = subprocess.run([sys.executable, "-c", _SYNC_CHILD % (ROOT, os.path.join(ROOT, "tests")), name], env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    n = int(p.stdout.split("launches")[1])
    lines = [ln for ln in p.stderr.splitlines() if ln.startswith("[dvits] %s op " % what)]
    assert n == STATS[name][KINDS[name].shapes[0]][0] and len(lines) == n, (n, len(lines))
    assert [int(ln.split(" op ")[1].split()[0]) for ln in lines] == list(range(n))
