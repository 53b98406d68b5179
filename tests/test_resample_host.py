"""Host side of the prompt resampler (packing.sinc_resample_taps, frontend.load_wav): no GPU needed.

The taps are held to two float64 statements of torchaudio's sinc_interp_hann resampler written here — (a) the framed convolution the kernel implements,
(b) the continuous-time sum it discretises — which must agree with each other to 1e-12; tests/test_gpu_resample.py imports (a) as the reference of
the device result."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from flowmirror_hydravox_amd import packing

LPW, ROLLOFF = 6, 0.99
# (orig_freq, new_freq) -> (phases, K) where the issue states them
PAIRS = [(44100, 16000), (44100, 24000), (48000, 16000), (48000, 24000), (32000, 24000), (24000, 16000), (22050, 24000), (16000, 24000)]
KNOWN = {(44100, 16000): (160, 475), (44100, 24000): (80, 171), (48000, 16000): (1, 41), (22050, 24000): (160, 161)}


def reduced(orig_freq, new_freq):
    g = math.gcd(orig_freq, new_freq)
    return orig_freq // g, new_freq // g


def taps64(orig_freq, new_freq):
    """float64 [new][K] taps + width, by the formula of torchaudio's _get_sinc_resample_kernel (sinc_interp_hann)"""
    orig, new = reduced(orig_freq, new_freq)
    base = min(orig, new) * ROLLOFF
    width = int(math.ceil(LPW * orig / base))
    k = torch.arange(2 * width + orig, dtype=torch.float64)
    p = torch.arange(new, dtype=torch.float64)
    t = ((-p[:, None] / new + (k[None, :] - width) / orig) * base).clamp(-LPW, LPW)
    window = torch.cos(t * math.pi / LPW / 2) ** 2
    t = t * math.pi
    return torch.where(t == 0, torch.ones_like(t), torch.sin(t) / t) * window * (base / orig), width


def framed_reference(x, taps, width, orig, new):
    """(a): y[j * new + p] = sum_k h[p][k] * xpad[j * orig + k] in float64, xpad = x with `width` zeros in front and `width + orig` behind, cut to
    ceil(new * L / orig).  x: (rows, L), taps: [new][K] (any float dtype; converted exactly)."""
    x, taps = x.double(), taps.double()
    L = x.shape[1]
    xpad = torch.nn.functional.pad(x, (width, width + orig))
    y = torch.nn.functional.conv1d(xpad[:, None, :], taps[:, None, :], stride=orig)           # (rows, new, frames)
    return y.transpose(1, 2).reshape(x.shape[0], -1)[:, :-(-new * L // orig)]


def continuous_reference(x, orig_freq, new_freq):
    """(b): y[n] = sum_m x[m] * h((m / orig_freq - n / new_freq) * base_freq), h(t) = sinc(pi t) cos^2(pi t / (2 LPW)) base / orig on |t| <= LPW, 0 outside"""
    x = x.double()
    L = x.shape[1]
    base = min(orig_freq, new_freq) * ROLLOFF
    n = torch.arange(-(-new_freq * L // orig_freq), dtype=torch.float64)
    m = torch.arange(L, dtype=torch.float64)
    t = ((m[None, :] / orig_freq - n[:, None] / new_freq) * base).clamp(-LPW, LPW)              # (at the clamp the window is cos^2(pi / 2) = 0)
    h = torch.special.sinc(t) * torch.cos(math.pi * t / (2 * LPW)) ** 2 * (base / orig_freq)
    return x @ h.t()


@pytest.mark.parametrize('orig_freq,new_freq', PAIRS)
def test_taps_match_two_float64_statements(orig_freq, new_freq):
    orig, new = reduced(orig_freq, new_freq)
    taps, width, o, n = packing.sinc_resample_taps(orig_freq, new_freq)
    t64, w64 = taps64(orig_freq, new_freq)
    assert (o, n, width) == (orig, new, w64) and taps.dtype == torch.float32 and tuple(taps.shape) == (new, 2 * width + orig)
    if (orig_freq, new_freq) in KNOWN:
        assert tuple(taps.shape) == KNOWN[(orig_freq, new_freq)]
    g = torch.Generator().manual_seed(orig_freq + new_freq)
    L = 3 * orig + 2 * width + 5                                   # a few frames whose taps lie inside the signal, and both zero-padded edges
    x = torch.rand(2, L, generator=g, dtype=torch.float64) * 2 - 1
    a = framed_reference(x, t64, width, orig, new)
    b = continuous_reference(x, orig_freq, new_freq)
    assert a.shape == b.shape == (2, -(-new * L // orig))
    err = (a - b).abs().max().item()
    print('%d -> %d: framed vs continuous %.3g' % (orig_freq, new_freq, err))
    assert err <= 1e-12, err
    assert torch.equal(taps, t64.float())                          # what ships = the float64 taps rounded to float32


def test_output_length_rule():
    for orig_freq, new_freq in PAIRS:
        orig, new = reduced(orig_freq, new_freq)
        t64, width = taps64(orig_freq, new_freq)
        for L in (1, orig - 1, orig, orig + 1, 10 * orig):
            if L < 1:
                continue
            want = math.ceil(Fraction(new_freq * L, orig_freq))
            assert packing.sinc_resample_len(L, orig, new) == want == packing.sinc_resample_len(L, orig_freq, new_freq)
            assert framed_reference(torch.ones(1, L), t64, width, orig, new).shape[1] == want
            assert new * (L // orig + 1) >= want                   # the frames the padding (width in front, width + orig behind) yields cover it


def test_refusals():
    from flowmirror_hydravox_amd import frontend
    with pytest.raises(ValueError) as e:
        packing.sinc_resample_taps(44101, 16000)                   # gcd 1: 16000 x 44135 floats
    assert '44101' in str(e.value) and '16000' in str(e.value) and '64 MiB' in str(e.value)
    with pytest.raises(ValueError):
        frontend.HvxResample(44101, 16000)                         # (before any device work)
    assert packing.sinc_resample_taps(44100, 16000)[0].numel() * 4 <= 64 << 20
    with pytest.raises(AssertionError) as e:
        frontend.load_wav((torch.zeros(1, 800), 8000), 16000)
    assert str(e.value) == 'wav sample rate 8000 must be greater than 16000'        # (the reference's message, file_utils.py:73)
    for path in ('prompt.wav', b'prompt.wav'):
        with pytest.raises(NotImplementedError):
            frontend.load_wav(path, 16000)
    import pathlib
    with pytest.raises(NotImplementedError):
        frontend.load_wav((pathlib.Path('prompt.wav'), 44100), 16000)


def test_load_wav_forms_that_need_no_resampling():
    """rate as int / float / numpy scalar / 0-d tensor, bare tensor and ndarray, stereo -> mono: with the rate already at target nothing runs on a device"""
    from flowmirror_hydravox_amd.frontend import load_wav
    g = torch.Generator().manual_seed(2)
    st = torch.rand(2, 50, generator=g) * 2 - 1
    mono = st.mean(0, keepdim=True)
    for sr in (16000, 16000.0, np.int64(16000), np.float32(16000), torch.tensor(16000)):
        got = load_wav((st, sr), 16000, device='cpu')
        assert got.dtype == torch.float32 and torch.equal(got, mono)
    assert torch.equal(load_wav(st[0], 24000, device='cpu'), st[:1])                      # a bare tensor is taken as already at target_sr
    assert torch.equal(load_wav(st.numpy(), 24000, device='cpu'), mono)
    assert torch.equal(load_wav([st[1].double().numpy(), 24000], 24000, device='cpu'), st[1:].float())
