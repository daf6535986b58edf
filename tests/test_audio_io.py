"""CPU: audio.read_wav / audio.write_wav and the opt-in audio arguments of tts_infer.  Every file is written byte by byte here with
`struct` (no fixture files) and must decode to exact expected floats: integers scaled by 2^(bits - 1), 8-bit offset by 128 first -
the values torchaudio.load documents (torchaudio itself is not installed where this project runs)."""
import struct

import numpy as np
import pytest
import torch

import resample_cases as rc
from diff_vits_amd import tts_infer
from diff_vits_amd.audio import Resample, read_wav, write_wav
from diff_vits_amd.mel import reference_mel_prompt

PCM, FLOAT, EXTENSIBLE = 1, 3, 0xFFFE
GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")


def chunk(cid, body):
    return cid + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def fmt_chunk(tag, channels, rate, bits, extensible=False):
    block = channels * bits // 8
    if extensible:
        return chunk(b"fmt ", struct.pack("<HHIIHHHHI", EXTENSIBLE, channels, rate, rate * block, block, bits, 22, bits, 0) + struct.pack("<H", tag) + GUID_TAIL)
    return chunk(b"fmt ", struct.pack("<HHIIHH", tag, channels, rate, rate * block, block, bits))


def riff(*chunks, form=b"WAVE", magic=b"RIFF"):
    body = form + b"".join(chunks)
    return magic + struct.pack("<I", len(body)) + body


def put(tmp_path, data, name="a.wav"):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def int24(v):
    return struct.pack("<i", v)[:3]


FORMATS = {
    "pcm8": (PCM, 8, [0, 128, 255, 64], lambda v: struct.pack("<B", v), lambda v: (v - 128) / 128.0),
    "pcm16": (PCM, 16, [-32768, 0, 32767, 12345], lambda v: struct.pack("<h", v), lambda v: v / 32768.0),
    "pcm24": (PCM, 24, [-8388608, 0, 8388607, -1234567], int24, lambda v: v / 8388608.0),
    "pcm32": (PCM, 32, [-2 ** 31, 0, 2 ** 31 - 1, 123456789], lambda v: struct.pack("<i", v), lambda v: v / 2.0 ** 31),
    "float32": (FLOAT, 32, [-1.0, 0.0, 0.333, 1.5], lambda v: struct.pack("<f", v), lambda v: v),
    "float64": (FLOAT, 64, [-1.0, 0.0, 0.333, 1e-3], lambda v: struct.pack("<d", v), lambda v: v),
}


@pytest.mark.parametrize("extensible", [False, True], ids=["plain", "extensible"])
@pytest.mark.parametrize("name", list(FORMATS))
def test_every_format_decodes_to_exact_floats(tmp_path, name, extensible):
    tag, bits, values, pack, scale = FORMATS[name]
    data = riff(fmt_chunk(tag, 1, 22050, bits, extensible), chunk(b"data", b"".join(pack(v) for v in values)))
    x, sr = read_wav(put(tmp_path, data))
    assert sr == 22050 and x.dtype == torch.float32 and x.shape == (1, len(values))
    assert np.array_equal(x[0].numpy(), np.array([scale(v) for v in values], dtype=np.float64).astype(np.float32))


def test_stereo_chunk_order_and_odd_padding(tmp_path):
    frames = [(1, -1), (2, -2), (3, -3)]
    body = b"".join(struct.pack("<hh", l, r) for l, r in frames)
    # a LIST chunk ahead of fmt, an unknown odd-sized chunk (padded to even) between fmt and data, junk behind the data
    data = riff(chunk(b"LIST", b"INFOISFT\x05\x00\x00\x00abcde\x00"), fmt_chunk(PCM, 2, 48000, 16), chunk(b"odd ", b"xyz"), chunk(b"data", body),
                chunk(b"junk", b"12"))
    x, sr = read_wav(put(tmp_path, data))
    assert sr == 48000 and x.shape == (2, 3)
    assert np.array_equal(x.numpy(), np.array([[1, 2, 3], [-1, -2, -3]], np.float32) / 32768.0)
    # an odd-sized data chunk of 8-bit samples, with its pad byte, then another chunk
    data = riff(fmt_chunk(PCM, 1, 8000, 8), chunk(b"data", bytes([128, 129, 130])), chunk(b"tail", b"zz"))
    x, _ = read_wav(put(tmp_path, data, "b.wav"))
    assert x.tolist() == [[0.0, 1 / 128.0, 2 / 128.0]]
    # five channels
    data = riff(fmt_chunk(PCM, 5, 8000, 16), chunk(b"data", struct.pack("<10h", *range(10))))
    x, _ = read_wav(put(tmp_path, data, "c.wav"))
    assert x.shape == (5, 2) and x[3].tolist() == [3 / 32768.0, 8 / 32768.0]


def test_refusals_name_the_reason(tmp_path):
    ok_fmt, ok_data = fmt_chunk(PCM, 1, 8000, 16), chunk(b"data", struct.pack("<2h", 1, 2))
    truncated = riff(ok_fmt, b"data" + struct.pack("<I", 100) + b"\0\0\0\0")
    cases = [
        (b"", "not a RIFF"),
        (b"OggS" + b"\0" * 40, "not a RIFF"),
        (riff(ok_fmt, ok_data, magic=b"RIFX"), "not a RIFF"),
        (riff(ok_fmt, ok_data, form=b"AVI "), "not WAVE"),
        (truncated, "truncated data chunk"),
        (riff(ok_fmt, chunk(b"data", b"\0\0\0")), "truncated data chunk"),                       # no whole number of sample frames
        (riff(ok_fmt), "no data chunk"),
        (riff(ok_data), "before the fmt"),
        (riff(chunk(b"LIST", b"abcd")), "no fmt chunk"),
        (riff(chunk(b"fmt ", b"\1\0\1\0"), ok_data), "truncated fmt"),
        (riff(fmt_chunk(0x0055, 1, 44100, 16), ok_data), "compressed or unknown format 0x0055"),
        (riff(fmt_chunk(0x0007, 1, 8000, 8), ok_data), "mu-law"),
        (riff(fmt_chunk(0x0002, 1, 8000, 16, extensible=True), ok_data), "compressed or unknown format 0x0002"),
        (riff(fmt_chunk(PCM, 1, 8000, 12), ok_data), "12-bit"),
        (riff(fmt_chunk(FLOAT, 1, 8000, 16), ok_data), "16-bit float"),
        (riff(chunk(b"fmt ", struct.pack("<HHIIHH", PCM, 2, 8000, 16000, 2, 16)), ok_data), "block align"),
        (riff(chunk(b"fmt ", struct.pack("<HHIIHHHHI", EXTENSIBLE, 1, 8000, 16000, 2, 16, 22, 16, 0) + b"\1\0" + b"\xff" * 14), ok_data), "SubFormat"),
    ]
    for i, (data, word) in enumerate(cases):
        with pytest.raises(ValueError, match=word):
            read_wav(put(tmp_path, data, "bad%d.wav" % i))


def test_round_trips(tmp_path):
    x = torch.from_numpy(np.stack([rc.signal("noise", 1001, 1), rc.signal("tone", 1001, 2)]))
    x[0, :4] = torch.tensor([1.5, -1.5, 32767.4 / 32768, -1.0])           # clipped, clipped, rounds down to the top code, the bottom code
    write_wav(str(tmp_path / "f.wav"), x, 24000, bits=32)
    y, sr = read_wav(str(tmp_path / "f.wav"))
    assert sr == 24000 and torch.equal(y, x)                              # float32: exact
    write_wav(str(tmp_path / "p.wav"), x, 16000)
    y, sr = read_wav(str(tmp_path / "p.wav"))
    assert sr == 16000 and y.shape == x.shape
    assert y[0, :4].tolist() == [32767 / 32768.0, -1.0, 32767 / 32768.0, -1.0]
    inside = x.abs() <= 32767 / 32768.0
    assert float((y - x)[inside].abs().max()) <= 0.5 / 32768.0            # PCM 16: half an LSB
    codes = (y * 32768.0).numpy()
    assert np.array_equal(codes, np.rint(codes))
    write_wav(str(tmp_path / "m.wav"), x[1], 8000)                        # a plain vector is one channel
    assert read_wav(str(tmp_path / "m.wav"))[0].shape == (1, 1001)
    with pytest.raises(ValueError):
        write_wav(str(tmp_path / "x.wav"), x, 8000, bits=24)
    with pytest.raises(ValueError):
        write_wav(str(tmp_path / "x.wav"), x[None], 8000)


def test_refer_prompt_native_route_and_unchanged_defaults(tmp_path):
    x = torch.from_numpy(rc.signal("noise", 9000, 4))[None, :] * 0.5
    path = str(tmp_path / "prompt.wav")
    write_wav(path, x, 44100, bits=32)
    with pytest.raises(ImportError):
        tts_infer.refer_prompt(path, "cpu")                               # the default still asks for torchaudio
    with pytest.raises(ValueError):
        tts_infer.refer_prompt(path, "cpu", audio_backend="soundfile")
    want = reference_mel_prompt(Resample(44100, 24000)(x))
    got = tts_infer.refer_prompt(path, "cpu", audio_backend="native")
    assert got.shape == (1, 100, 1 + rc.output_length(9000, 147, 80) // 256) and torch.equal(got, want)
    assert torch.equal(tts_infer.refer_prompt(x, "cpu", sample_rate=44100), want)
    # a tensor without sample_rate is 24 kHz audio, as before; sample_rate=24000 says the same
    assert torch.equal(tts_infer.refer_prompt(x, "cpu"), reference_mel_prompt(x))
    assert torch.equal(tts_infer.refer_prompt(x, "cpu", sample_rate=24000), reference_mel_prompt(x))


def test_recording_mels_with_rates_and_save_wav(tmp_path):
    rates, ns = [44100, 16000, 24000], [3000, 1200, 1700]
    waves = np.zeros((3, 3000), np.float32)
    for b, n in enumerate(ns):
        waves[b, :n] = rc.signal("noise", n, 60 + b)
    y, yl = tts_infer.recording_mels(waves, ns, "cpu", sample_rates=rates)
    conv, cl = Resample(rates, 24000)(torch.from_numpy(waves), torch.tensor(ns))
    assert cl.tolist() == [rc.output_length(3000, 147, 80), 1800, 1700] and yl.tolist() == [1 + int(v) // 256 for v in cl]
    for b in range(3):
        alone = reference_mel_prompt(conv[b:b + 1, :int(cl[b])])[0]
        assert torch.equal(y[b, :, :alone.shape[-1]], alone) and not y[b, :, alone.shape[-1]:].any()
    one, ol = tts_infer.recording_mels(waves[:1], ns[:1], "cpu", sample_rates=44100)
    assert torch.equal(one[0, :, :int(ol[0])], y[0, :, :int(yl[0])])
    # without sample_rates nothing changes
    a, al = tts_infer.recording_mels(waves, ns, "cpu")
    b_, bl = reference_mel_prompt(torch.from_numpy(waves), lengths=torch.tensor(ns))
    assert torch.equal(a, b_) and torch.equal(al, bl)
    # save_wav: 24 kHz samples as they are, or converted first
    samples = torch.from_numpy(rc.signal("noise", 2400, 9))[None, :] * 0.5
    tts_infer.save_wav(str(tmp_path / "o.wav"), samples)
    back, sr = read_wav(str(tmp_path / "o.wav"))
    assert sr == 24000 and float((back - samples).abs().max()) <= 0.5 / 32768.0
    tts_infer.save_wav(str(tmp_path / "t.wav"), samples, out_rate=16000, bits=32)
    back, sr = read_wav(str(tmp_path / "t.wav"))
    assert sr == 16000 and torch.equal(back, Resample(24000, 16000)(samples))
