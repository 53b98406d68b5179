"""The streaming vocoder, host side (no GPU): `hift_left_context` against the CPU oracle's own dependency reach, the piece-length arithmetic of
`hvx_hift_stream_piece_samples` against the lengths `HvxHift.inference` documents, `StreamSession` / `stream_tts` on stand-in models with the
`incremental_vocoder` switch on and off, the refusals that need no device, and the new `_lib.SYMBOLS` entries against include/hvx.h.

The native handle of the host tests is built from CPU tensors: hvx_hift_create / hvx_hift_stream_create / hvx_hift_stream_bind only record pointers, and
every refusal of hvx_hift_stream_plan / hvx_hift_stream_piece tested here comes before the first launch."""
import ctypes as C
import os
import re
import weakref

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOK = 3


# ------------------------------------------------------------------------------------------------------------------------
# the context against the oracle
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def reach(tiny_cfg):
    """the oracle on a random mel and a random source, and on the same two with frame T0 (and its 480 source samples) perturbed -> per-frame largest
    change of the F0 and of the decoded samples, and the scale of each.  The source is part of the input: decode_frames is the reach of the mel frames
    AND of their source samples, and the longest path of the generator is a source branch (hift_left_context)."""
    from flowmirror_hydravox_amd import weights as W
    from oracle import hift_ref
    c = tiny_cfg.hift
    sd = W.make_hift_state(c, seed=3, init='fan_in')
    T, t0, up = 64, 8, c.upsample_total
    g = torch.Generator().manual_seed(5)
    mel = torch.randn(1, 80, T, generator=g)
    s = torch.rand(1, 1, T * up, generator=g) * 0.2 - 0.1
    mel2, s2 = mel.clone(), s.clone()
    mel2[:, :, t0] += 2 * torch.randn(80, generator=g)
    s2[:, :, t0 * up:(t0 + 1) * up] = 0.3 - s2[:, :, t0 * up:(t0 + 1) * up]
    a, b = (hift_ref.decode(m, x, sd, c, finalize=False) for m, x in ((mel, s), (mel2, s2)))
    fa, fb = (hift_ref.f0_predictor(m, sd, finalize=False) for m in (mel, mel2))
    assert a.shape == (1, (T - c.conv_pre_look_right - 1) * up) and fa.shape == (1, T - 3)
    return dict(t0=t0, wav=(a - b).abs()[0].reshape(-1, up).amax(1), wav_scale=float(a.abs().max()), f0=(fa - fb).abs()[0], f0_scale=float(fa.abs().max()))


def test_left_context_covers_the_oracles_reach_and_three_quarters_of_it_do_not(tiny_cfg, reach):
    from flowmirror_hydravox_amd.hift import hift_left_context
    f0_frames, decode_frames = hift_left_context(tiny_cfg.hift)
    t0 = reach['t0']
    eps = 2.0 ** -23                                                    # fp32 round-off, relative to the signal's scale
    # beyond the context nothing moves (the perturbed frame enters no arithmetic of those frames: the change is 0, not merely small)
    assert float(reach['f0'][t0 + f0_frames + 1:].max()) <= 4 * eps * reach['f0_scale']
    assert float(reach['wav'][t0 + decode_frames + 1:].max()) <= 4 * eps * reach['wav_scale']
    assert reach['wav'][t0 + decode_frames + 1:].numel() >= 8 and reach['f0'][t0 + f0_frames + 1:].numel() >= 8
    # three quarters of it are too short: frames beyond them still move, by far more than round-off
    short_f0, short_dec = f0_frames - f0_frames // 4, decode_frames - decode_frames // 4
    assert short_f0 < f0_frames and short_dec < decode_frames
    assert float(reach['f0'][t0 + short_f0 + 1:].max()) > 1e-3 * reach['f0_scale'], reach['f0'][t0:t0 + f0_frames + 2]
    assert float(reach['wav'][t0 + short_dec + 1:].max()) > 1e-3 * reach['wav_scale'], reach['wav'][t0:t0 + decode_frames + 2]
    # the look-ahead is the other side of the window: frames before t0 - 3 (F0) / t0 - conv_pre_look_right (decode; the source branches see a few
    # samples of the next frame) do not move either
    assert float(reach['f0'][:t0 - 3].max()) == 0.0 and float(reach['wav'][:t0 - tiny_cfg.hift.conv_pre_look_right - 1].max()) == 0.0


def test_left_context_of_the_cv3_configuration():
    """the figures of the docstring's derivation: 8 frames of F0 context, the source branch of stage 0 is the longest decode path (3435 / 120 frames)"""
    import dataclasses
    from flowmirror_hydravox_amd.config import HiftConfig
    from flowmirror_hydravox_amd.hift import hift_left_context
    c = HiftConfig()
    assert hift_left_context(c) == (8, 29)
    # one stage at rate 1 and no dilation: iSTFT 2 + conv_post 6 + pad 1, then main 2 * (k - 1) and source 2 * (k - 1) ResBlock reach, STFT 2; up conv (k - 1)
    one = dataclasses.replace(c, upsample_rates=[1], upsample_kernel_sizes=[3], resblock_kernel_sizes=[3], resblock_dilations=[[0, 0, 0]],
                              source_resblock_kernel_sizes=[5], source_resblock_dilations=[[0, 0, 0]])
    assert hift_left_context(one) == (8, max(9 + 6 + 12 + 0 + 2, 9 + 6 + 2))
    # a longer dilation lengthens it, a larger first rate shortens the share of the later stages
    assert hift_left_context(dataclasses.replace(c, resblock_dilations=[[1, 3, 9]] * 3))[1] > 29
    assert hift_left_context(dataclasses.replace(c, upsample_rates=[16, 5, 3]))[1] < 29


# ------------------------------------------------------------------------------------------------------------------------
# a native handle without a device
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def host_hift(tiny_cfg):
    from flowmirror_hydravox_amd import _lib, weights as W
    from flowmirror_hydravox_amd.hift import HvxHift, pack_hift_weights
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libhvx.so is not built (python -m flowmirror_hydravox_amd.build)')
    c = tiny_cfg.hift
    h = HvxHift.__new__(HvxHift)                                         # (the constructor insists on a device; what is tested here never launches)
    h.lib, h.cfg, h.device, h.exact_fp32, h.up = _lib.load(), c, torch.device('cpu'), False, c.upsample_total
    h._h = h._ws = None
    h._streams = weakref.WeakSet()
    h._stream_ws = None
    h.sine_table = torch.zeros(100 * c.upsample_total, c.nb_harmonics + 1)          # a noise table of 100 frames
    h.load_packed(pack_hift_weights(W.make_hift_state(c, seed=3, init='fan_in'), c, 'cpu'))
    return h


def test_piece_samples_against_the_documented_lengths(tiny_cfg, host_hift):
    """HvxHift.inference: finalize=False -> (fill - 3 - conv_pre_look_right - 1) * up samples (decode_chunk's docstring), finalize=True -> fill * up; a
    piece is the difference to what the previous, non-final pass returned"""
    from flowmirror_hydravox_amd._lib import HvxError
    c, up = tiny_cfg.hift, tiny_cfg.hift.upsample_total
    hold = 3 + c.conv_pre_look_right + 1
    assert hold == 8 and up == 480

    def whole(fill, final):
        return fill * up if final else (fill - hold) * up
    ps = host_hift.piece_samples
    assert ps(0, 12, False) == whole(12, False) == 4 * up                # the first piece
    assert ps(0, 9, False) == up and ps(0, 5, True) == 5 * up            # the shortest non-final pass; a short utterance in one final pass
    assert ps(37, 38, False) == up                                       # a growth of one frame
    assert ps(38, 38, False) == 0                                        # ... of none
    assert ps(160, 160, True) == whole(160, True) - whole(160, False) == hold * up          # a final call with no new frame hands out what was held back
    assert ps(90, 160, True) == (160 - 82) * up
    assert ps(5, 9, False) == up                                         # (a previous fill too small to have handed anything out counts as nothing)
    fills, handed = [12, 37, 38, 90, 160], 0
    for prev, (fill, final) in zip([0] + fills, [(f, False) for f in fills] + [(160, True)]):
        n = ps(prev, fill, final)
        assert handed + n == whole(fill, final)
        handed += n
    for bad in ((0, 8, False), (0, 0, False), (12, 11, False), (12, 11, True), (-1, 4, True)):
        with pytest.raises(HvxError):
            ps(*bad)


def test_refusals_before_any_launch(tiny_cfg, host_hift):
    from flowmirror_hydravox_amd import _lib
    from flowmirror_hydravox_amd._lib import HvxError
    lib, up = host_hift.lib, host_hift.up
    st = host_hift.stream(120)
    assert host_hift.live_streams == 1
    mel = torch.zeros(80, 128)
    with pytest.raises(HvxError, match='exceeds'):
        st.piece(mel, 121, False)                                        # fill > max_frames
    with pytest.raises(HvxError, match='needs more than 8'):
        st.piece(mel, 8, False)                                          # what HvxHift.inference(finalize=False) raises on
    with pytest.raises(HvxError, match='noise table'):
        st.piece(mel, 104, False)                                        # 101 source frames, a table of 100
    with pytest.raises(HvxError, match='noise table'):
        st.piece(mel, 101, True)
    plan = (C.c_int64 * 4)()
    assert lib.hvx_hift_stream_plan(st._st, 103, 0, plan) == 0 and list(plan) == [95 * up, 103, 100, 0]      # a first window starts at frame 0
    assert lib.hvx_hift_stream_plan(st._st, 100, 1, plan) == 0 and list(plan) == [100 * up, 100, 100, 0]
    # the piece call itself: a buffer that is too small, a mel plane narrower than fill, a stream of another handle, a stream without memory
    ws = torch.zeros(lib.hvx_hift_stream_workspace_bytes(host_hift._h, 12), dtype=torch.uint8)
    out = torch.zeros(4 * up)

    def piece(stream, fill, cap, ld=128):
        return lib.hvx_hift_stream_piece(host_hift._h, None, _lib.ptr(ws), ws.numel(), stream, _lib.ptr(mel), ld, fill, 0, _lib.ptr(out), cap)
    assert piece(st._st, 12, 4 * up - 1) == -1 and b'samples for a buffer' in lib.hvx_last_error()
    assert piece(st._st, 12, 4 * up, ld=11) == -1 and b'row stride' in lib.hvx_last_error()
    assert piece(None, 12, 4 * up) == -1
    bare = C.c_void_p()
    assert lib.hvx_hift_stream_create(host_hift._h, 64, C.byref(bare)) == 0
    assert piece(bare, 12, 4 * up) == -1 and b'no state bound' in lib.hvx_last_error()
    small = torch.zeros(16, dtype=torch.uint8)
    assert lib.hvx_hift_stream_bind(bare, _lib.ptr(small), small.numel(), _lib.ptr(host_hift.sine_table), 100 * up) == -1
    lib.hvx_hift_stream_destroy(bare)
    assert lib.hvx_hift_stream_create(host_hift._h, 0, C.byref(bare)) == -1
    # nothing above advanced the stream
    info = (C.c_int64 * 8)()
    assert lib.hvx_hift_stream_info(st._st, info) == 0 and list(info)[:4] == [0, 0, 0, 0]
    # the workspace is a function of the window alone, the state of max_frames alone (40 bytes a frame at 9 harmonics, plus alignment)
    assert lib.hvx_hift_stream_workspace_bytes(host_hift._h, 50) < lib.hvx_hift_stream_workspace_bytes(host_hift._h, 100)
    per_frame = (lib.hvx_hift_stream_state_bytes(host_hift._h, 4096) - lib.hvx_hift_stream_state_bytes(host_hift._h, 2048)) / 2048.0
    assert per_frame == 4 * (1 + tiny_cfg.hift.nb_harmonics + 1)
    st.close()
    st.close()
    assert host_hift.live_streams == 0


def test_native_context_is_the_python_derivation(tiny_cfg, host_hift):
    from flowmirror_hydravox_amd.hift import hift_left_context
    a, b = C.c_int32(), C.c_int32()
    assert host_hift.lib.hvx_hift_left_context(host_hift._h, C.byref(a), C.byref(b)) == 0
    assert (a.value, b.value) == hift_left_context(tiny_cfg.hift)


# ------------------------------------------------------------------------------------------------------------------------
# StreamSession / stream_tts on stand-in models
# ------------------------------------------------------------------------------------------------------------------------
class FakeFlow:
    """frame j (counted after the prompt) of the mel it returns holds the value j (tests/test_stream_serve_host.py)"""
    token_mel_ratio = 2
    pre_lookahead_len = LOOK
    device = 'cpu'

    def inference(self, token, token_len, embedding, finalize=True, prompt_token=None, prompt_token_len=None, prompt_feat=None, prompt_feat_len=None,
                  streaming=False):
        n = int(token.shape[1])
        n_out = n if finalize else n - self.pre_lookahead_len
        return torch.arange(self.token_mel_ratio * n_out, dtype=torch.float32).expand(1, 80, -1).clone(), None


class FakeStream:
    def __init__(self, owner, max_frames):
        self.owner, self.max_frames, self.handed, self.closed = owner, max_frames, 0, False

    def piece(self, mel, fill, finalize):
        assert not self.closed and fill <= self.max_frames
        assert [int(v) for v in mel[0, 0, :fill].tolist()] == list(range(fill))           # the whole cache so far, in order
        self.owner.piece_calls.append((int(fill), bool(finalize)))
        total = 480 * (fill if finalize else fill - 8)
        out = torch.arange(self.handed, total, dtype=torch.float32)[None]
        self.handed = total
        return out

    def close(self):
        self.closed = True


class FakeHift:
    """sample k holds the value k; finalize=False holds back 8 frames as the causal vocoder does"""
    max_stream_frames = 4096

    def __init__(self):
        self.inference_calls, self.piece_calls, self.streams = [], [], []

    def inference(self, speech_feat, finalize=True):
        n = int(speech_feat.shape[2])
        self.inference_calls.append((n, bool(finalize)))
        return torch.arange(480 * (n if finalize else max(n - 8, 0)), dtype=torch.float32)[None], None

    def stream(self, max_frames):
        self.streams.append(FakeStream(self, max_frames))
        return self.streams[-1]


def _run(n_prompt, n_tokens, hop, **kw):
    from flowmirror_hydravox_amd.streaming import stream_tts
    flow, hift = FakeFlow(), FakeHift()
    toks = torch.randint(0, 96, (n_tokens,), generator=torch.Generator().manual_seed(n_tokens)).tolist()
    pieces = list(stream_tts(iter(toks), flow, hift, torch.zeros(1, n_prompt, dtype=torch.int32), torch.zeros(1, 2 * n_prompt, 80), torch.zeros(1, 192),
                             token_hop_len=hop, **kw))
    return hift, pieces


@pytest.mark.parametrize('n_prompt,n_tokens', [(0, 3 * 25 + LOOK + 1), (26, 81), (24, 1)])
def test_stream_tts_calls_piece_once_per_job(n_prompt, n_tokens):
    from flowmirror_hydravox_amd.streaming import ChunkSchedule
    hop = 25
    sched = ChunkSchedule(n_prompt, hop, LOOK)
    jobs = [(n, False) for n, _ in sched.feed(range(n_tokens))] + [(sched.finish()[0], True)]
    fills = [(2 * (n if fin else n - LOOK), fin) for n, fin in jobs]                      # frames in the cache after the job's solve
    off, off_pieces = _run(n_prompt, n_tokens, hop)
    on, on_pieces = _run(n_prompt, n_tokens, hop, incremental_vocoder=True)
    # off: inference over the whole cache, as before, and no stream is ever made
    assert off.inference_calls == fills and off.piece_calls == [] and off.streams == []
    # on: one piece call per job with (fill, finalize), never the whole-cache pass; one stream for the utterance, released at the end
    assert on.piece_calls == fills and on.inference_calls == []
    assert len(on.streams) == 1 and on.streams[0].closed and on.streams[0].max_frames == FakeHift.max_stream_frames
    # the same pieces
    assert len(on_pieces) == len(off_pieces) == len(jobs)
    assert all(torch.equal(a, b) for a, b in zip(on_pieces, off_pieces))
    assert torch.equal(torch.cat(on_pieces, dim=1)[0], torch.arange(960 * n_tokens, dtype=torch.float32))


def test_session_switch_speed_and_early_stop():
    from flowmirror_hydravox_amd.streaming import StreamSession, stream_tts
    flow, hift = FakeFlow(), FakeHift()
    args = (torch.zeros(1, 0, dtype=torch.int32), torch.zeros(1, 0, 80), torch.zeros(1, 192))
    # the switch without stream=True is refused
    with pytest.raises(ValueError):
        list(stream_tts(iter(range(30)), flow, hift, *args, stream=False, incremental_vocoder=True))
    assert hift.streams == []
    # a consumer that stops after the first piece leaves no stream behind
    gen = stream_tts(iter(range(90)), flow, hift, *args, incremental_vocoder=True)
    next(gen)
    assert len(hift.streams) == 1 and not hift.streams[0].closed
    gen.close()
    assert hift.streams[0].closed
    # the speed != 1.0 answer is the one of the switch-off path
    for kw in (dict(), dict(incremental_vocoder=True)):
        sess = StreamSession(flow, FakeHift(), *args, max_frames=64, **kw)
        with pytest.raises(AssertionError, match='speed change only support non-stream inference mode'):
            sess.push(torch.zeros(1, 40, dtype=torch.int32), 0, stream=True, finalize=False, speed=1.5)
        if kw:
            assert sess.hift.streams[0].max_frames == 64
        sess.close()


def test_serving_layers_refuse_the_switch_without_stream():
    from flowmirror_hydravox_amd.pipeline import HvxPipeline
    from flowmirror_hydravox_amd.worker import serve_queue
    pipe = HvxPipeline.__new__(HvxPipeline)                              # (refused before the pipeline is looked at)
    pipe.acoustic_batch = 1
    with pytest.raises(ValueError, match='stream=True'):
        list(pipe.serve(None, incremental_vocoder=True))
    with pytest.raises(ValueError, match='stream=True'):
        serve_queue(None, None, {}, incremental_vocoder=True)


# ------------------------------------------------------------------------------------------------------------------------
# the binding against the header
# ------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_bound():
    from flowmirror_hydravox_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'hvx.h')).read(), flags=re.S)
    new = {'hvx_hift_left_context': 3, 'hvx_hift_stream_piece_samples': 4, 'hvx_hift_stream_create': 3, 'hvx_hift_stream_destroy': 1,
           'hvx_hift_stream_reset': 1, 'hvx_hift_stream_state_bytes': 2, 'hvx_hift_stream_bind': 5, 'hvx_hift_stream_set_context': 3,
           'hvx_hift_stream_set_inputs': 3, 'hvx_hift_stream_workspace_bytes': 2, 'hvx_hift_stream_plan': 4, 'hvx_hift_stream_info': 2,
           'hvx_hift_stream_piece': 11}
    assert sorted(n for n in _lib.SYMBOLS if n.startswith('hvx_hift_stream_') or n == 'hvx_hift_left_context') == sorted(new)
    for name, n_args in new.items():
        m = re.search(r'\b%s\s*\(([^;]*?)\)\s*;' % name, src, flags=re.S)
        assert m, name
        assert len(m.group(1).split(',')) == n_args == len(_lib.SYMBOLS[name][1]), name
    assert _lib.HVX_ABI_VERSION == 8                                     # additive: the version existing tests pin stays
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert all(hasattr(lib, n) for n in new)
