"""Where audio enters and leaves the package: WAV files and sample-rate conversion (the reference's `torchaudio.load(path)` and
`torchaudio.transforms.Resample(sr, 24000)`, `tts_infer.py:54-56`).

PARITY: torchaudio is not installed in the build container or on the GPU box, so `Resample` is a restatement of its documented
defaults (`resampling_method="sinc_interp_hann"`, `lowpass_filter_width=6`, `rolloff=0.99`) written from the published source and
still NOT compared with torchaudio OUTPUT.  It is pinned to the fp64 restatement of that definition (tests/resample_cases.py: explicit
index map, no convolution routine; profiles/resample_reference.txt, profiles/resample_parity.txt).  `read_wav` returns the values
`torchaudio.load` documents (integers scaled by 2^(bits - 1), 8-bit offset by 128 first).

The definition, with o = orig / gcd and n = new / gcd: base = min(o, n) * 0.99, width = ceil(6 o / base), K = 2 width + o,
    t = clamp((-p / n + (j - width) / o) * base, -6, 6),  h[p][j] = sinc(t) * cos(pi t / 12)^2 * base / o     (p < n, j < K)
computed in fp64 and rounded ONCE to fp32 (torchaudio computes the kernel in double and casts), and
    y[q n + p] = sum_j h[p][j] x[q o - width + j],  x = 0 outside [0, N),  N_out = ceil(n N / o);  orig == new: the input unchanged.

Two backends.  None: torch ops on the caller's device - the table as a conv1d weight with stride o and the interleave of the phases,
torchaudio's algorithm.  "hip" (opt-in): the native kernel (csrc/kernels_resample.hip, dv_resample_*), a ragged batch whose rows
have their own lengths AND their own rate pairs in one launch; GPU float32 tensors only, never a fall-back.  With `lengths` both
backends return (out, out_lengths) and compute every row from its own samples alone, zeros behind out_lengths[b].
"""
import math
import struct

import numpy as np
import torch

LOWPASS_FILTER_WIDTH, ROLLOFF = 6, 0.99
MAX_REDUCED_RATE = 1024          # backend="hip": o and n after reduction (the table is staged in LDS)


def reduce_pair(orig_freq, new_freq):
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if orig_freq < 1 or new_freq < 1:
        raise ValueError("sample rates must be positive integers, got %r -> %r" % (orig_freq, new_freq))
    g = math.gcd(orig_freq, new_freq)
    return orig_freq // g, new_freq // g


def output_length(n_samples, o, n):
    """ceil(n N / o) in integers."""
    return -((-int(n_samples) * n) // o)


def filter_table(o, n):
    """(h float32 [n, K], width): the taps in fp64, torchaudio's order of operations, rounded once.  o == n: the delta (identity)."""
    base = min(o, n) * ROLLOFF
    width = int(math.ceil(LOWPASS_FILTER_WIDTH * o / base))
    K = 2 * width + o
    if o == n:
        h = np.zeros((n, K), np.float32)
        h[:, width] = 1.0
        return h, width
    idx = np.arange(-width, width + o, dtype=np.float64)[None, :] / o
    t = np.arange(0, -n, -1, dtype=np.float64)[:, None] / n + idx
    t = np.clip(t * base, -LOWPASS_FILTER_WIDTH, LOWPASS_FILTER_WIDTH)
    window = np.cos(t * math.pi / LOWPASS_FILTER_WIDTH / 2.0) ** 2
    t = t * math.pi
    scale = base / o
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(t == 0.0, 1.0, np.sin(t) / t)
    return (k * (window * scale)).astype(np.float32), width


class Resample(torch.nn.Module):
    """torchaudio.transforms.Resample(orig_freq, new_freq) with its defaults: waveform [..., N] -> [..., ceil(n N / o)].
    `orig_freq` may be a sequence of B rates: row b of a `[B, n_max]` batch is then converted from orig_freq[b] (needs `lengths`)."""

    def __init__(self, orig_freq, new_freq=24000, backend=None):
        super().__init__()
        if backend not in (None, "hip"):
            raise ValueError("backend must be None or 'hip'")
        self.backend, self.new_freq = backend, int(new_freq)
        self.per_row = not isinstance(orig_freq, (int, np.integer)) and not (isinstance(orig_freq, torch.Tensor) and orig_freq.dim() == 0)
        rates = [int(r) for r in (orig_freq.tolist() if isinstance(orig_freq, torch.Tensor) else orig_freq)] if self.per_row else [int(orig_freq)]
        if not rates:
            raise ValueError("orig_freq is empty")
        self.orig_freq = rates if self.per_row else rates[0]
        self.pairs, self.row_pair = [], []               # distinct reduced pairs, and every row's index into them
        for r in rates:
            pr = reduce_pair(r, self.new_freq)
            if pr not in self.pairs:
                self.pairs.append(pr)
            self.row_pair.append(self.pairs.index(pr))
        if backend == "hip":
            bad = [pr for pr in self.pairs if max(pr) > MAX_REDUCED_RATE]
            if bad:
                raise ValueError("backend='hip' needs orig / gcd and new / gcd <= %d, got %d : %d" % ((MAX_REDUCED_RATE,) + bad[0]))
        self._tables, self._hip, self._pair_dev = {}, None, {}

    # ------------------------------------------------------------------------------------------------------------- torch ops
    def _kernel(self, pair, like):
        key = (pair, like.device, like.dtype)
        if key not in self._tables:
            h, width = filter_table(*pair)
            self._tables[key] = (torch.from_numpy(h).to(device=like.device, dtype=like.dtype)[:, None, :], width)
        return self._tables[key]

    def _resample_torch(self, x, pair):
        """x [R, N] -> [R, ceil(n N / o)]: pad (width, width + o), conv1d with stride o, interleave the n phases, cut."""
        o, n = pair
        if o == n:
            return x
        kernel, width = self._kernel(pair, x)
        N = x.shape[-1]
        y = torch.nn.functional.conv1d(torch.nn.functional.pad(x, (width, width + o))[:, None, :], kernel, stride=o)
        return y.transpose(1, 2).reshape(x.shape[0], -1)[:, :output_length(N, o, n)]

    def out_width(self, n_max):
        """Width of a ragged call's output buffer: the largest ceil(n n_max / o) over this module's pairs."""
        return max(output_length(n_max, o, n) for o, n in self.pairs)

    def check_lengths(self, waveform, lengths):
        """One host read: every n_b in [0, n_max]."""
        v = [int(a) for a in lengths.tolist()]
        bad = [(b, a) for b, a in enumerate(v) if a < 0 or a > waveform.shape[-1]]
        if bad:
            raise ValueError("lengths must be in [0, %d] (the buffer's width); row %d has %d" % (waveform.shape[-1], bad[0][0], bad[0][1]))
        return v

    def _ragged_args(self, waveform, lengths):
        if waveform.dim() != 2:
            raise ValueError("with lengths the waveform must be [B, n_max], got %s" % (tuple(waveform.shape),))
        lengths = torch.as_tensor(lengths)
        if lengths.dtype not in (torch.int64, torch.int32) or lengths.shape != (waveform.shape[0],):
            raise ValueError("lengths must be an integer tensor [B]")
        if self.per_row and len(self.row_pair) != waveform.shape[0]:
            raise ValueError("orig_freq names %d rows, the batch has %d" % (len(self.row_pair), waveform.shape[0]))
        return lengths

    def _row_pairs(self, B):
        return self.row_pair if self.per_row else [0] * B

    def forward(self, waveform, lengths=None, validate=True):
        """lengths=None: a plain batch [..., N] -> [..., N_out].  With `lengths` [B] (samples per row of a [B, n_max] batch): returns
        (out [B, out_width(n_max)], out_lengths int64 [B]), each row computed from its own samples alone, zeros behind it."""
        if self.backend == "hip":
            return self._forward_hip(waveform, lengths, validate)
        if lengths is None:
            if self.per_row:
                raise ValueError("per-row rates need lengths (the rows' outputs differ in length)")
            if self.pairs[0][0] == self.pairs[0][1]:
                return waveform                                  # orig == new: the input unchanged
            shape = waveform.shape
            y = self._resample_torch(waveform.reshape(-1, shape[-1]), self.pairs[0])
            return y.reshape(shape[:-1] + y.shape[-1:])
        lengths = self._ragged_args(waveform, lengths)
        v = self.check_lengths(waveform, lengths)                # the torch route needs the integers anyway
        B, n_max = waveform.shape
        out = waveform.new_zeros(B, self.out_width(n_max))
        n_out = []
        for b, pi in enumerate(self._row_pairs(B)):
            y = self._resample_torch(waveform[b:b + 1, :v[b]], self.pairs[pi])[0]
            out[b, :y.shape[0]] = y
            n_out.append(y.shape[0])
        return out, torch.tensor(n_out, dtype=torch.int64, device=waveform.device)

    # ------------------------------------------------------------------------------------------------------------- the kernel
    def _forward_hip(self, waveform, lengths, validate):
        import ctypes as C

        from . import _lib
        if not (isinstance(waveform, torch.Tensor) and waveform.is_cuda and waveform.dtype == torch.float32):
            raise ValueError("backend='hip' needs a float32 GPU waveform (there is no fall-back)")
        ragged = lengths is not None
        if not ragged and self.per_row:
            raise ValueError("per-row rates need lengths (the rows' outputs differ in length)")
        shape = waveform.shape
        if not ragged and self.pairs[0][0] == self.pairs[0][1]:
            return waveform                                      # orig == new: the input unchanged
        x = (waveform if ragged else waveform.reshape(-1, shape[-1])).contiguous()
        if ragged:
            lengths = self._ragged_args(x, lengths)
            if not lengths.is_cuda or lengths.dtype != torch.int64:
                raise ValueError("backend='hip' needs int64 GPU lengths")
            if validate:
                self.check_lengths(x, lengths)
            lengths = lengths.contiguous()
        else:
            lengths = torch.full((x.shape[0],), shape[-1], dtype=torch.int64, device=x.device)
        B, n_max = x.shape
        if n_max < 1:
            raise ValueError("the waveform is empty")
        L = _lib.lib()
        if self._hip is None:
            o = np.array([p[0] for p in self.pairs], dtype=np.int32)
            n = np.array([p[1] for p in self.pairs], dtype=np.int32)
            h = C.c_void_p()
            _lib.check(L.dv_resample_create(o.ctypes.data_as(C.c_void_p), n.ctypes.data_as(C.c_void_p), len(self.pairs), C.byref(h)),
                       "dv_resample_create")
            self._hip = _ResampleHandle(h)
        pair = None
        if self.per_row:
            if x.device not in self._pair_dev:
                self._pair_dev[x.device] = torch.tensor(self.row_pair, dtype=torch.int32, device=x.device)
            pair = self._pair_dev[x.device]
        n_out_max = self.out_width(n_max)
        out = torch.empty(B, n_out_max, dtype=torch.float32, device=x.device)
        n_out = torch.empty(B, dtype=torch.int64, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(L.dv_resample_forward(self._hip.h, _lib.ptr(x), _lib.ptr(lengths), _lib.ptr(pair), B, n_max, _lib.ptr(out), n_out_max,
                                             _lib.ptr(n_out), _lib.stream_ptr()), "dv_resample_forward")
        if ragged:
            return out, n_out
        return out.reshape(shape[:-1] + out.shape[-1:])


class _ResampleHandle:
    """Owner of a dv_resample handle (the device tables of the native kernel)."""

    def __init__(self, h):
        self.h = h

    def __del__(self):
        try:
            from . import _lib
            _lib.lib().dv_resample_destroy(self.h)
        except Exception:
            pass


def resample(waveform, orig_freq, new_freq=24000, lengths=None, backend=None):
    """`Resample(orig_freq, new_freq, backend)(waveform, lengths)` for a one-off call."""
    return Resample(orig_freq, new_freq, backend=backend)(waveform, lengths)


# ----------------------------------------------------------------------------------------------------------------- WAV files
WAVE_FORMAT_PCM, WAVE_FORMAT_IEEE_FLOAT, WAVE_FORMAT_EXTENSIBLE = 0x0001, 0x0003, 0xFFFE
# the tail of every WAVE_FORMAT_EXTENSIBLE SubFormat GUID whose first two bytes are a plain format tag (KSDATAFORMAT_SUBTYPE_*)
_GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")
_FORMAT_NAMES = {0x0002: "ADPCM", 0x0006: "A-law", 0x0007: "mu-law", 0x0011: "IMA ADPCM", 0x0031: "GSM 6.10", 0x0055: "MPEG layer 3"}


def read_wav(path):
    """A RIFF / WAVE file -> (float32 [channels, n], sample_rate).  PCM 8-bit unsigned ((v - 128) / 128), 16 / 24 / 32-bit signed
    (v / 2^(bits - 1)), IEEE float 32 / 64, WAVE_FORMAT_EXTENSIBLE over any of them, any channel count; unknown chunks are skipped
    (odd sizes padded to even).  ValueError naming the reason for anything else: not RIFF / WAVE, a compressed format, a missing
    or truncated chunk."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 12 or data[:4] != b"RIFF":
        raise ValueError("%s: not a RIFF file%s" % (path, " (RF64 / RIFX are not read)" if data[:4] in (b"RF64", b"RIFX") else ""))
    if data[8:12] != b"WAVE":
        raise ValueError("%s: a RIFF file of form %r, not WAVE" % (path, data[8:12]))
    pos, fmt, payload = 12, None, None
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], struct.unpack_from("<I", data, pos + 4)[0]
        body = pos + 8
        if cid == b"fmt ":
            if size < 16 or body + size > len(data):
                raise ValueError("%s: truncated fmt chunk (%d bytes)" % (path, min(size, len(data) - body)))
            fmt = data[body:body + size]
        elif cid == b"data":
            if fmt is None:
                raise ValueError("%s: the data chunk comes before the fmt chunk" % (path,))
            if body + size > len(data):
                raise ValueError("%s: truncated data chunk: the header promises %d bytes, the file holds %d" % (path, size, len(data) - body))
            payload = data[body:body + size]
            break
        pos = body + size + (size & 1)
    if fmt is None:
        raise ValueError("%s: no fmt chunk" % (path,))
    if payload is None:
        raise ValueError("%s: no data chunk" % (path,))
    tag, channels, rate, _, block, bits = struct.unpack_from("<HHIIHH", fmt, 0)
    if tag == WAVE_FORMAT_EXTENSIBLE:
        if len(fmt) < 40 or struct.unpack_from("<H", fmt, 16)[0] < 22:
            raise ValueError("%s: truncated WAVE_FORMAT_EXTENSIBLE fmt chunk (%d bytes)" % (path, len(fmt)))
        if fmt[26:40] != _GUID_TAIL:
            raise ValueError("%s: unknown WAVE_FORMAT_EXTENSIBLE SubFormat %s" % (path, fmt[24:40].hex()))
        tag = struct.unpack_from("<H", fmt, 24)[0]
    if tag not in (WAVE_FORMAT_PCM, WAVE_FORMAT_IEEE_FLOAT):
        raise ValueError("%s: compressed or unknown format 0x%04x%s: only PCM and IEEE float are read"
                         % (path, tag, " (%s)" % _FORMAT_NAMES[tag] if tag in _FORMAT_NAMES else ""))
    if channels < 1 or rate < 1:
        raise ValueError("%s: %d channels at %d Hz" % (path, channels, rate))
    if (tag == WAVE_FORMAT_PCM and bits not in (8, 16, 24, 32)) or (tag == WAVE_FORMAT_IEEE_FLOAT and bits not in (32, 64)):
        raise ValueError("%s: %d-bit %s samples are not read" % (path, bits, "PCM" if tag == WAVE_FORMAT_PCM else "float"))
    width = bits // 8
    if block != channels * width:
        raise ValueError("%s: block align %d, expected channels * bytes per sample = %d" % (path, block, channels * width))
    if len(payload) % block:
        raise ValueError("%s: truncated data chunk: %d bytes are no whole number of %d-byte sample frames" % (path, len(payload), block))
    raw = np.frombuffer(payload, dtype=np.uint8)
    if tag == WAVE_FORMAT_IEEE_FLOAT:
        x = raw.view("<f4" if bits == 32 else "<f8").astype(np.float32)
    elif bits == 8:
        x = (raw.astype(np.float32) - 128.0) / 128.0
    elif bits == 24:
        b = raw.reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        x = ((v ^ 0x800000) - 0x800000).astype(np.float32) / 8388608.0
    else:
        x = raw.view("<i2" if bits == 16 else "<i4").astype(np.float64) / float(1 << (bits - 1))
        x = x.astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(x.reshape(-1, channels).T)), int(rate)


def write_wav(path, wave, sample_rate, bits=16):
    """float [channels, n] (or [n]) -> a WAVE file: bits=16 PCM (round to nearest of 32768 x, clipped to -32768 .. 32767) or
    bits=32 IEEE float.  `read_wav` returns the float32 input exactly for bits=32 and within half an LSB (2^-16) for in-range PCM."""
    if bits not in (16, 32):
        raise ValueError("bits must be 16 (PCM) or 32 (IEEE float)")
    x = torch.as_tensor(wave).detach().to("cpu")
    if x.dim() == 1:
        x = x[None, :]
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[0] > 65535:
        raise ValueError("wave must be [channels, n] or [n], got %s" % (tuple(x.shape),))
    sample_rate = int(sample_rate)
    if sample_rate < 1:
        raise ValueError("sample_rate must be positive")
    channels = x.shape[0]
    frames = x.to(torch.float32).numpy().T                      # [n, channels]: interleaved
    if bits == 16:
        body = np.clip(np.rint(frames.astype(np.float64) * 32768.0), -32768, 32767).astype("<i2").tobytes()
        fmt = struct.pack("<HHIIHH", WAVE_FORMAT_PCM, channels, sample_rate, sample_rate * channels * 2, channels * 2, 16)
        extra = b""
    else:
        body = np.ascontiguousarray(frames, dtype="<f4").tobytes()
        fmt = struct.pack("<HHIIHHH", WAVE_FORMAT_IEEE_FLOAT, channels, sample_rate, sample_rate * channels * 4, channels * 4, 32, 0)
        extra = b"fact" + struct.pack("<II", 4, frames.shape[0])
    chunks = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + extra + b"data" + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")
    if len(chunks) > 0xFFFFFFFF:
        raise ValueError("more than 4 GiB of samples do not fit a RIFF file")
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(chunks)) + chunks)
