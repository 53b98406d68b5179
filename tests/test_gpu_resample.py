"""The device sinc resampler (csrc/resample.hip: hvx_op_resample_sinc, frontend.HvxResample) against the float64 framed convolution of
tests/test_resample_host.py, its bit-level properties and refusals, and the frontend built on it (frontend.load_wav, HvxFrontEnd) up to a waveform
out of HvxModelManager."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_resample_host import PAIRS, framed_reference, reduced      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _inputs(L, seed):
    """(4, L) float32: seeded uniform [-1, 1], a unit impulse at sample 0 and at sample L - 1 (the zero-padded edges), all ones"""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(4, L)
    x[0] = torch.rand(L, generator=g) * 2 - 1
    x[1, 0] = 1.0
    x[2, L - 1] = 1.0
    x[3] = 1.0
    return x


@pytest.mark.parametrize('orig_freq,new_freq', PAIRS)
def test_resample_matches_float64_within_the_fp32_dot_product_bound(orig_freq, new_freq):
    """Every output of every case against reference (a) evaluated in float64 on the float32 taps and the float32 input.  The bound is derived, per phase p:
    |err| <= (K + 2) * 2^-24 * sum_k |h[p][k]| * max|x| — the forward error of a K-term fp32 dot product accumulated in any order (gamma_K ~ K u, u = 2^-24,
    with the FMA's one rounding per term) plus the rounding of the result; nothing measured goes into it.  Lengths: 1, 17 (shorter than width), orig,
    10 orig -+ 1, 44101, 132301 (several tiles, the last one ragged); one row at a time, and three rows at once from a buffer whose row stride exceeds the
    length — which must also equal the one-row results bit for bit."""
    from flowmirror_hydravox_amd import packing
    from flowmirror_hydravox_amd.frontend import HvxResample
    orig, new = reduced(orig_freq, new_freq)
    taps, width, _, _ = packing.sinc_resample_taps(orig_freq, new_freq)
    K = taps.shape[1]
    rs = HvxResample(orig_freq, new_freq, device=DEV)
    per_phase = (K + 2) * 2.0 ** -24 * taps.double().abs().sum(1)                    # [new]
    worst = 0.0
    for L in (1, 17, orig, 10 * orig - 1, 10 * orig + 1, 44101, 132301):
        x = _inputs(L, seed=L + orig_freq)
        ref = framed_reference(x, taps, width, orig, new)                             # (4, n_out) float64
        n_out = packing.sinc_resample_len(L, orig, new)
        assert ref.shape == (4, n_out)
        bound = per_phase[torch.arange(n_out) % new][None, :] * x.abs().amax(1, keepdim=True).double()
        xd = x.to(DEV)
        single = [rs(xd[i]) for i in range(4)]
        for i in range(4):
            assert single[i].shape == (n_out,) and single[i].dtype == torch.float32 and single[i].is_cuda
            err = (single[i].cpu().double() - ref[i]).abs()
            assert bool((err <= bound[i]).all()), (L, i, err.max().item(), bound[i].max().item(), int((err > bound[i]).nonzero()[0]))
            worst = max(worst, (err / bound[i]).max().item())
        wide = torch.full((3, L + 5), 7.0, device=DEV)                                # row stride L + 5 > L; the slack must not be read as audio
        wide[:, :L] = xd[[0, 2, 3]]
        many = rs(wide[:, :L])
        assert many.shape == (3, n_out)
        for r, i in enumerate((0, 2, 3)):
            assert torch.equal(many[r], single[i]), (L, i)
    print('%d -> %d: K %d, bound %.2g .. %.2g, worst error / bound %.3f' % (orig_freq, new_freq, K, per_phase.min().item(), per_phase.max().item(), worst))


@pytest.mark.parametrize('orig_freq,new_freq', PAIRS)
def test_outputs_do_not_depend_on_what_lies_behind_their_taps(orig_freq, new_freq):
    """the first outputs of a waveform equal, bit for bit, those of its own prefix, for every output whose taps end before the cut (the two calls tile
    differently: other frame counts, other tile sizes for the small-orig pairs)"""
    from flowmirror_hydravox_amd import packing
    from flowmirror_hydravox_amd.frontend import HvxResample
    orig, new = reduced(orig_freq, new_freq)
    _, width, _, _ = packing.sinc_resample_taps(orig_freq, new_freq)
    rs = HvxResample(orig_freq, new_freq, device=DEV)
    g = torch.Generator().manual_seed(9)
    x = (torch.rand(132301, generator=g) * 2 - 1).to(DEV)
    full = rs(x)
    for cut in (44101, 10 * orig + 1):
        part = rs(x[:cut])
        # frame j reads x[j * orig - width, j * orig + width + orig): inside the prefix while j * orig + width + orig <= cut
        n_frames = (cut - width - orig) // orig + 1 if cut >= width + orig else 0
        assert n_frames > 0 and n_frames * new <= part.numel()
        assert torch.equal(part[:n_frames * new], full[:n_frames * new])
        assert not torch.equal(part, full[:part.numel()])                             # (the tail does see the cut)


def test_equal_rates_return_the_input():
    from flowmirror_hydravox_amd.frontend import HvxResample
    x = torch.rand(2, 100)
    assert HvxResample(24000, 24000, device=DEV)(x) is x


def test_launcher_refuses_what_it_cannot_tile():
    """each refusal returns an error and launches nothing: the output buffer keeps its fill"""
    from flowmirror_hydravox_amd import _lib, packing
    lib = _lib.load()
    _lib.require_gpu()
    taps, width, orig, new = packing.sinc_resample_taps(24000, 16000)                 # orig 3, new 2
    tp = taps.t().contiguous().to(DEV)
    x = torch.rand(2, 300, device=DEV)
    y = torch.full((2, 256), -5.0, device=DEV)
    ok = dict(x=x.data_ptr(), rows=2, len=300, x_rs=300, taps=tp.data_ptr(), orig=orig, new=new, width=width, y=y.data_ptr(), out_len=200, y_rs=256)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.hvx_op_resample_sinc(C.c_void_p(a['x']), a['rows'], a['len'], a['x_rs'], C.c_void_p(a['taps']), a['orig'], a['new'], a['width'],
                                        C.c_void_p(a['y']), a['out_len'], a['y_rs'], _lib.stream_ptr())

    bad = [(dict(x=None), 'null'), (dict(taps=None), 'null'), (dict(y=None), 'null'),
           (dict(rows=0), 'positive'), (dict(rows=-1), 'positive'), (dict(len=0), 'positive'), (dict(out_len=0), 'positive'), (dict(out_len=-3), 'positive'),
           (dict(orig=0), 'positive'), (dict(new=0), 'positive'), (dict(width=0), 'positive'), (dict(width=-1), 'positive'),
           (dict(rows=65536), 'rows'),
           (dict(out_len=201), 'exceeds ceil'),                                       # ceil(2 * 300 / 3) = 200
           (dict(x_rs=299), 'strides'), (dict(y_rs=199), 'strides'),                  # rows would overlap
           (dict(orig=16385 - 2 * width, out_len=1), '64 KB'),                        # one frame spans 16385 floats: over 64 KB of LDS
           (dict(orig=20000, width=25000, out_len=1), '64 KB'),
           (dict(new=1 << 23), '64 MiB')]                                             # a tap table of (2 * width + 3) * 2^23 floats
    for kw, why in bad:
        assert call(**kw) != 0, kw
        assert why in lib.hvx_last_error().decode(), (kw, lib.hvx_last_error())
    # the bound on out_len is computed in 64-bit: 2 * 1.5e9 wraps in 32-bit, the true bound is 1e9
    assert call(len=1500000000, x_rs=1500000000, out_len=1000000001, y_rs=1000000001) != 0
    assert b'1000000000' in lib.hvx_last_error()
    torch.cuda.synchronize()
    assert bool((y == -5.0).all())
    assert call() == 0                                                                # (the unmodified call is fine, and writes only out_len samples per row)
    torch.cuda.synchronize()
    assert bool((y[:, 200:] == -5.0).all()) and bool((y[:, :200] != -5.0).all())
    bound = (taps.shape[1] + 2) * 2.0 ** -24 * taps.double().abs().sum(1).max().item()      # (the derived bound of the accuracy test, max|x| <= 1)
    assert (y[:, :200].cpu().double() - framed_reference(x.cpu(), taps, width, orig, new)).abs().max().item() <= bound


# ---- composition ------------------------------------------------------------------------------------------------------------------------------------
def _graphs():
    import onnx_synth
    from flowmirror_hydravox_amd import onnx_graph as og
    # the synthetic assets at the real widths; ids in [0, 81) fit the tiny config's 96 speech tokens, the embedding its 192-wide speaker input
    return og.save_onnx(onnx_synth.tokenizer_like(n_mels=128, with_length=True)), og.save_onnx(onnx_synth.campplus_like(emb=192))


def _tokenize(text):
    return [(ord(ch) * 7) % 500 for ch in text]


KEYS = {'text', 'text_len', 'prompt_text', 'prompt_text_len', 'llm_prompt_speech_token', 'llm_prompt_speech_token_len', 'flow_prompt_speech_token',
        'flow_prompt_speech_token_len', 'prompt_speech_feat', 'prompt_speech_feat_len', 'llm_embedding', 'flow_embedding'}


def test_frontend_zero_shot_composes_the_device_stages():
    """HvxFrontEnd over the synthetic graphs of tests/onnx_synth.py at the real widths (128 mels, 80 fbank bins, 192-wide embedding), a stereo 44.1 kHz
    prompt: the reference's key set, dtypes and [1][N] shapes, every tensor bit-equal to the stages called by hand on HvxResample outputs, and
    prompt_speech_feat_len == 2 * llm_prompt_speech_token_len.
    The trim takes min(int(feat / 2), tokens).  The synthetic tokenizer emits 50 tokens per second (a stride-2 stem on 100 whisper frames per second; the
    real asset emits 25) against 50 mel frames per second, so tokens ~ feat here and int(feat / 2) is the smaller side at every prompt length the graph's
    128-row position table admits: the `tokens` side is unreachable with it.  Both prompt lengths below therefore take the `feat` side (one with an odd
    frame count, one with an even one); the `tokens` side is taken by the third case, which swaps in a tokenizer that returns fewer tokens."""
    from flowmirror_hydravox_amd.frontend import HvxFrontEnd, HvxMelSpectrogram, HvxResample, HvxSpeakerEncoder, HvxSpeechTokenizer, load_wav
    tok_model, spk_model = _graphs()
    fe = HvxFrontEnd(_tokenize, tok_model, spk_model, device=DEV)
    tk, enc, mel = HvxSpeechTokenizer(tok_model), HvxSpeakerEncoder(spk_model), HvxMelSpectrogram()
    to16, to24 = HvxResample(44100, 16000, device=DEV), HvxResample(44100, 24000, device=DEV)
    g = torch.Generator().manual_seed(21)
    for seconds in (1.3, 0.97):
        stereo = (0.2 * torch.randn(2, int(44100 * seconds), generator=g)).clamp(-1, 1)
        mi = fe.frontend_zero_shot('hello there', 'a prompt', (stereo, 44100), 24000, '')
        assert set(mi) == KEYS
        mono = stereo.mean(0, keepdim=True).to(DEV)
        w16, w24 = to16(mono), to24(mono)
        assert torch.equal(load_wav((stereo, 44100.0), 16000), w16) and torch.equal(load_wav((stereo.numpy(), torch.tensor(44100)), 24000), w24)
        tokens, _ = tk(w16)
        feat = mel(w24).transpose(1, 2)
        n = min(int(feat.shape[1] / 2), tokens.shape[1])
        assert n == int(feat.shape[1] / 2) < tokens.shape[1]                         # (the `feat` side of the min, see above)
        assert torch.equal(mi['llm_prompt_speech_token'], tokens[:, :n]) and torch.equal(mi['flow_prompt_speech_token'], tokens[:, :n])
        assert torch.equal(mi['prompt_speech_feat'], feat[:, :2 * n]) and tuple(mi['prompt_speech_feat'].shape) == (1, 2 * n, 80)
        assert mi['llm_prompt_speech_token_len'].tolist() == [n] == mi['flow_prompt_speech_token_len'].tolist()
        assert mi['prompt_speech_feat_len'].tolist() == [2 * n]
        emb = enc(w16)
        assert torch.equal(mi['llm_embedding'], emb) and torch.equal(mi['flow_embedding'], emb) and tuple(emb.shape) == (1, 192)
        assert mi['text'].tolist() == [_tokenize('hello there')] and mi['text_len'].tolist() == [11]
        assert mi['prompt_text'].tolist() == [_tokenize('a prompt')] and mi['prompt_text_len'].tolist() == [8]
        for k in ('text', 'text_len', 'prompt_text', 'prompt_text_len', 'llm_prompt_speech_token', 'llm_prompt_speech_token_len', 'prompt_speech_feat_len'):
            assert mi[k].dtype == torch.int32 and mi[k].is_cuda, k
        assert mi['prompt_speech_feat'].dtype == mi['llm_embedding'].dtype == torch.float32
        # another resample_rate: no trim (frontend.py:169)
        raw = fe.frontend_zero_shot('hello there', 'a prompt', (stereo, 44100), 22050, '')
        assert torch.equal(raw['llm_prompt_speech_token'], tokens) and torch.equal(raw['prompt_speech_feat'], feat)
    # the `tokens` side of the min
    fe.speech_tokenizer = lambda speech: (tokens[:, :7].clone(), torch.tensor([7], dtype=torch.int32, device=DEV))
    mi = fe.frontend_zero_shot('x', 'y', (stereo, 44100), 24000, '')
    assert mi['llm_prompt_speech_token_len'].tolist() == [7] and mi['prompt_speech_feat_len'].tolist() == [14]
    assert torch.equal(mi['prompt_speech_feat'], feat[:, :14]) and torch.equal(mi['llm_prompt_speech_token'], tokens[:, :7])
    # a stored speaker: the spk2info branch and frontend_sft
    stored = {k: v for k, v in mi.items() if k not in ('text', 'text_len')}
    fe.spk2info = {'anna': dict(stored, embedding=emb)}
    again = fe.frontend_zero_shot('hello', '', None, 24000, 'anna')
    assert set(again) == KEYS | {'embedding'} and again['text'].tolist() == [_tokenize('hello')] and again['prompt_speech_feat'] is stored['prompt_speech_feat']
    assert 'text' not in fe.spk2info['anna']
    sft = fe.frontend_sft('hello', 'anna')
    assert set(sft) == {'text', 'text_len', 'llm_embedding', 'flow_embedding'} and sft['flow_embedding'] is emb
    assert fe.text_normalize('a. b', split=True) == ['a. b'] and fe.text_normalize('a. b', split=False) == 'a. b'


def test_inference_zero_shot_from_a_raw_48k_prompt(tiny_cfg, tmp_path):
    """inference_zero_shot on an HvxModelManager at the tiny config (the model directory of test_queue_worker_serves_the_continuous_engine) whose frontend is
    HvxFrontEnd: a 48 kHz prompt tensor in, a finite waveform out, the same for the same seed, and equal to `_synthesize` on frontend_zero_shot's dict."""
    import argparse
    import dataclasses
    import json
    from flowmirror_hydravox_amd import weights as W
    from flowmirror_hydravox_amd.frontend import HvxFrontEnd
    from flowmirror_hydravox_amd.model_manager import HvxModelManager, _synthesize, inference_zero_shot
    c = tiny_cfg
    d = tmp_path / 'model'
    d.mkdir()
    torch.save(W.make_llm_state(c.llm, seed=5, init='fan_in'), d / 'llm.pt')
    torch.save(W.make_flow_state(c.flow, seed=6, init='fan_in'), d / 'flow.pt')
    torch.save(W.make_hift_state(c.hift, seed=7, init='fan_in'), d / 'hift.pt')
    (d / 'hvx_config.json').write_text(json.dumps({'llm': dataclasses.asdict(c.llm), 'flow': dataclasses.asdict(c.flow), 'hift': dataclasses.asdict(c.hift)}))
    tok_model, spk_model = _graphs()
    mm = HvxModelManager(frontend_factory=lambda args, cfg: HvxFrontEnd(_tokenize, tok_model, spk_model))
    mm.load_models(argparse.Namespace(config=None, model_dir=str(d), bf16=True, fp16=False, cpu=False))
    assert isinstance(mm.frontend, HvxFrontEnd)
    g = torch.Generator().manual_seed(4)
    prompt = (0.2 * torch.randn(1, 48000, generator=g)).clamp(-1, 1)                  # 1 s at 48 kHz
    torch.manual_seed(31)
    wav = inference_zero_shot(mm, 'hello world', 'the prompt', prompt, 48000)
    assert wav.dim() == 2 and wav.shape[0] == 1 and wav.shape[1] > 0 and bool(torch.isfinite(wav).all())
    torch.manual_seed(31)
    assert torch.equal(inference_zero_shot(mm, 'hello world', 'the prompt', prompt, 48000), wav)
    mi = mm.frontend.frontend_zero_shot('hello world', 'the prompt', (prompt, 48000), 24000, zero_shot_spk_id='')
    assert mi['prompt_speech_feat_len'].item() == 2 * mi['llm_prompt_speech_token_len'].item() > 0
    torch.manual_seed(31)
    assert torch.equal(_synthesize(mm, mi, 1.0, zero_shot=True), wav)
