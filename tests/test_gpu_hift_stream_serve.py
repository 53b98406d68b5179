"""`HvxPipeline.serve(stream=True)` and `stream_tts` with the `incremental_vocoder` switch off and on: same pieces (counts, lengths, `final`, tokens), audio
within the end-to-end bound of the vocoder (2e-2, the F0 -> phase amplification), fewer frames through the vocoder, and no vocoder stream left behind by a
finished or a cancelled utterance."""
import threading

import pytest
import torch

pytestmark = pytest.mark.gpu
RATIO = 15                               # tokens per text token (min = max: the lengths are fixed): 120 .. 180 tokens, 5 .. 8 pieces per utterance
CANCELLED = 501                          # the seed of the utterance that is cancelled when its first piece arrives


class _Src:
    def __init__(self, items):
        self.it = iter(items)

    def poll(self, block):
        return next(self.it)


def _utts(cfg, hop):
    from flowmirror_hydravox_amd.pipeline import synthetic_utterance
    utts = [synthetic_utterance(cfg, 500, 8), synthetic_utterance(cfg, CANCELLED, 12), synthetic_utterance(cfg, 502, 10, n_prompt_speech=hop + 1, n_prompt_text=4)]
    for u in utts:
        u.max_token_text_ratio = u.min_token_text_ratio = RATIO
    utts[1].cancel = threading.Event()
    return utts


def _serve(pipe, cfg, hop, **kw):
    utts = _utts(cfg, hop)
    pieces, errors, live_seen = {}, {}, []
    for u, piece, info in pipe.serve(_Src(utts), lm_slots=3, stream=True, **kw):
        live_seen.append(pipe.hift.live_streams)
        if isinstance(piece, BaseException):
            errors[u.seed] = piece
            continue
        pieces.setdefault(u.seed, []).append((piece.clone(), info))
        if u.seed == CANCELLED:
            u.cancel.set()
    return dict(pieces=pieces, errors=errors, stats=dict(pipe.last_continuous), live_seen=live_seen, live_after=pipe.hift.live_streams)


@pytest.fixture(scope='module')
def served(tiny_cfg):
    from flowmirror_hydravox_amd.pipeline import HvxPipeline
    hop = tiny_cfg.flow.static_chunk_size // tiny_cfg.flow.token_mel_ratio
    pipe = HvxPipeline(tiny_cfg, llm_dtype=torch.float32, flow_dtype=torch.float32, max_batch=3, max_ctx=512, max_t=1024, seed=7, init='fan_in',
                       inference_head_num=2)
    off = _serve(pipe, tiny_cfg, hop)
    on = _serve(pipe, tiny_cfg, hop, incremental_vocoder=True)
    return dict(pipe=pipe, hop=hop, off=off, on=on)


def test_serve_gives_the_same_pieces_with_the_switch_on(served):
    from flowmirror_hydravox_amd.llm import Cancelled
    off, on = served['off'], served['on']
    for seed in (500, 502):
        a, b = off['pieces'][seed], on['pieces'][seed]
        assert len(a) == len(b) >= 4, (seed, len(a), len(b))
        assert [i for _, i in a] == [i for _, i in b]                              # index, final and, on the last piece, the tokens
        assert [i['final'] for _, i in b] == [False] * (len(b) - 1) + [True] and len(b[-1][1]['tokens']) == RATIO * (8 if seed == 500 else 10)
        assert [p.numel() for p, _ in a] == [p.numel() for p, _ in b], seed
        err = max(float((p - q).abs().max()) for (p, _), (q, _) in zip(a, b))
        print('utterance %d: %d pieces, max abs %.3e' % (seed, len(a), err))
        assert err < 2e-2, (seed, err)
        assert sum(p.numel() for p, _ in b) == 960 * RATIO * (8 if seed == 500 else 10)
    # the cancelled utterance: the pieces both runs handed out before the cancellation took hold are the same, and it comes back once as Cancelled
    for run in (off, on):
        assert isinstance(run['errors'].get(CANCELLED), Cancelled) and list(run['errors']) == [CANCELLED]
        assert run['stats']['cancelled'] == 1 and run['stats']['abandoned'] == []
        got = run['pieces'][CANCELLED]
        assert 1 <= len(got) < 8 and not any(i['final'] for _, i in got)
    for (p, i), (q, j) in zip(off['pieces'][CANCELLED], on['pieces'][CANCELLED]):
        assert i == j and p.numel() == q.numel() and float((p - q).abs().max()) < 2e-2


def test_vocoder_frames_and_released_streams(served):
    off, on = served['off'], served['on']
    print('vocoder_frames: off %d, on %d' % (off['stats']['vocoder_frames'], on['stats']['vocoder_frames']))
    assert 0 < on['stats']['vocoder_frames'] < off['stats']['vocoder_frames']
    # switch off: no stream ever exists; on: at most one per utterance in flight, none once the call has ended — the cancelled one's included
    assert max(off['live_seen']) == 0 and off['live_after'] == 0
    assert 1 <= max(on['live_seen']) <= 3 and on['live_after'] == 0
    # after the cancelled utterance has come back, the streams alive belong to the utterances still in flight
    pipe = served['pipe']
    assert pipe.hift.live_streams == 0


def test_stream_tts_with_the_switch(tiny_cfg, served):
    from flowmirror_hydravox_amd.streaming import stream_tts
    pipe, hop = served['pipe'], served['hop']
    toks = served['on']['pieces'][500][-1][1]['tokens']
    u = _utts(tiny_cfg, hop)[0]
    args = (torch.zeros(1, 0, dtype=torch.int32), torch.zeros(1, 0, 80), u.embedding[None])
    a = list(stream_tts(iter(toks), pipe.flow, pipe.hift, *args, token_hop_len=hop))
    b = list(stream_tts(iter(toks), pipe.flow, pipe.hift, *args, token_hop_len=hop, incremental_vocoder=True))
    assert len(a) == len(b) >= 4 and [p.shape for p in a] == [p.shape for p in b]
    err = max(float((p - q).abs().max()) for p, q in zip(a, b))
    print('stream_tts: %d pieces, max abs %.3e' % (len(a), err))
    assert err < 2e-2
    assert torch.equal(a[0], b[0])                                                 # the first window starts at frame 0: today's launches
    assert pipe.hift.live_streams == 0
    # ... and serve's pieces of that utterance are stream_tts's, switch on (the relation test_serve_stream_equals_stream_tts_alone holds with it off)
    got = served['on']['pieces'][500]
    assert [int(p.numel()) for p, _ in got] == [int(q.shape[1]) for q in b]
    assert float((torch.cat([p for p, _ in got]) - torch.cat(b, dim=1)[0]).abs().max()) < 2e-2
    with pytest.raises(ValueError):
        list(stream_tts(iter(toks), pipe.flow, pipe.hift, *args, token_hop_len=hop, stream=False, incremental_vocoder=True))
