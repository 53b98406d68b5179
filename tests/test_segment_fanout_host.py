"""Segmented long texts in the decode grid and per-request cancel, host side (no GPU): `worker._TaskSource(segment_fanout=True)` expanding a task into
its segments, `worker.serve_queue` assembling / failing / streaming a fanned-out task over a scripted pipeline, and the `cancel` task."""
import os
import queue
import random
import types

import pytest
import torch

from test_host_cpu import _QueueFrontend

TEXT = 'alpha beta gamma, delta epsilon zeta. eta theta iota; kappa lambda mu! nu xi omicron pi? rho sigma tau upsilon.'
CHARS = 100
SR = 24000
EP = dict(top_p=0.8, top_k=25, win_size=10, tau_r=0.1, inference_head_num=2)


def _mm(**kw):
    return types.SimpleNamespace(frontend=_QueueFrontend(), configs={'sample_rate': SR}, is_loaded=True, get_available_speakers=lambda: ['s', 'tt'], **kw)


def _long(**kw):
    return dict(dict(id='long', task_type='tts', text=TEXT, speaker_id='s', extra_params=dict(EP, speed=1.25), seed=300), **kw)


def _short(i, text='tail'):
    return dict(id='short%d' % i, task_type='tts', text=text, speaker_id='s', extra_params=dict(EP), seed=900 + i)


def _gaps(seed, n):
    random.seed(seed)
    return [int(random.uniform(50, 150) * SR / 1000) for _ in range(n)]


def _segments():
    from flowmirror_hydravox_amd.model_manager import merge_short_segments, split_text_by_punctuation
    segs = merge_short_segments(split_text_by_punctuation(TEXT, 30, 10), 10)
    assert len(TEXT) == 111 and len(segs) == 6 and ''.join(segs) == TEXT and all(10 <= len(s) <= 30 for s in segs)
    return segs


# ---- 1: expansion -----------------------------------------------------------------------------------------------------------------------------
def test_task_source_expands_a_segmented_task_into_its_segments():
    from flowmirror_hydravox_amd.worker import _TaskSource, segment_seeds
    segs = _segments()
    assert segment_seeds(300, 6) == [300, 301, 302, 303, 304, 305] and segment_seeds(2 ** 31 - 1, 3) == [2 ** 31 - 1, 0, 1] and segment_seeds(None, 2) == [None, None]
    q, results = queue.Queue(), {}
    q.put(_short(1))
    random.seed(41)
    src = _TaskSource(_mm(), q, results, _long(), lambda s: s, 0, segment_fanout=True, segmented_text_chars=CHARS)
    got = [src.poll(False) for _ in range(7)]
    assert src.poll(False) is None and not src.closed and results == {}
    six, tail = got[:6], got[6]
    assert [u.tag['id'] for u in got] == ['long'] * 6 + ['short1'] and [u.segment[1] for u in six] == list(range(6))
    fe = _QueueFrontend()
    for k, u in enumerate(six):                                                 # built as inference_tts builds a segment, with the task's knobs
        assert u.text.tolist() == fe._ids(segs[k])[0].tolist() and u.speaker_id == 's' and u.speed == 1.25 and u.prompt_text is None
        assert float(u.embedding[0]) == pytest.approx(0.01)
    assert [u.seed for u in six] == segment_seeds(300, 6)
    fan = six[0].segment[0]
    assert all(u.segment[0] is fan and u.cancel is fan.cancel for u in six) and not fan.cancel.is_set() and hasattr(fan.cancel, 'is_set')
    assert tail.cancel is not fan.cancel and getattr(tail, 'segment', None) is None
    assert fan.segments == segs and fan.gaps == _gaps(41, 5) and src.n_fanned == 1
    # a task without a seed: every segment draws its own
    src = _TaskSource(_mm(), queue.Queue(), {}, _long(seed=None), lambda s: s, 0, segment_fanout=True, segmented_text_chars=CHARS)
    assert [src.poll(False).seed for _ in range(6)] == [None] * 6
    # a set cancel (a failed sibling, a cancel task): what still waits never joins, the queue is read on
    q = queue.Queue()
    q.put(_short(2))
    src = _TaskSource(_mm(), q, {}, _long(), lambda s: s, 0, segment_fanout=True, segmented_text_chars=CHARS)
    first = src.poll(False)
    first.cancel.set()
    assert src.poll(False).tag['id'] == 'short2' and not src.pending
    # a segment the frontend refuses fails the task once, with the 1-based number, and retires the siblings
    q, results = queue.Queue(), {}
    q.put(_short(3))
    src = _TaskSource(_mm(), q, results, _long(text=TEXT.replace('eta theta', 'eta BAD theta')), lambda s: s, 0, segment_fanout=True, segmented_text_chars=CHARS)
    a, b, c = src.poll(False), src.poll(False), src.poll(False)
    assert (a.segment[1], b.segment[1], c.tag['id']) == (0, 1, 'short3') and a.cancel.is_set()
    assert set(results) == {'long'} and results['long']['error'].startswith('TTS failed: segment 3 failed: cannot tokenise')
    # the switch off: the same queue closes the epoch at the long task (tests/test_host_cpu.py expects the same of a 5001-character text)
    q = queue.Queue()
    for t in (_long(), _short(1)):
        q.put(t)
    src = _TaskSource(_mm(), q, {}, _short(0), lambda s: s, 0, segmented_text_chars=CHARS)
    assert src.poll(False).tag['id'] == 'short0'
    with pytest.raises(StopIteration):
        src.poll(False)
    assert src.carry['id'] == 'long' and not src.stop and q.qsize() == 1 and src.n_fanned == 0
    # ... and with the switch on, a long task whose parameters do not fit the epoch is still a boundary
    q = queue.Queue()
    q.put(_long(extra_params=dict(EP, top_k=10)))
    src = _TaskSource(_mm(), q, {}, _short(0), lambda s: s, 0, segment_fanout=True, segmented_text_chars=CHARS)
    assert src.poll(False).tag['id'] == 'short0'
    with pytest.raises(StopIteration):
        src.poll(False)
    assert src.carry['id'] == 'long'


# ---- a scripted pipeline under serve_queue -------------------------------------------------------------------------------------------------
class _Log(dict):
    """a result dict that remembers every write in order"""

    def __init__(self):
        super().__init__()
        self.writes = []

    def __setitem__(self, k, v):
        self.writes.append(k)
        super().__setitem__(k, v)


class _ScriptedPipe:
    """HvxPipeline.serve over a script: takes everything the source has, then yields what `script(utterances by (task id, segment), kwargs)` says"""

    def __init__(self, script):
        self.script, self.llm = script, None

    def serve(self, source, **kw):
        utts = {}
        while True:
            try:
                u = source.poll(False)
            except StopIteration:
                break
            if u is None:
                break
            utts[(u.tag['id'], getattr(u, 'segment', (None, None))[1])] = u
        yield from self.script(utts, kw)


def _serve(monkeypatch, tasks, script, results=None, **kw):
    from flowmirror_hydravox_amd import pipeline, worker
    monkeypatch.setattr(pipeline.HvxPipeline, 'from_models', classmethod(lambda cls, *a, **k: _ScriptedPipe(script)))
    llm = types.SimpleNamespace(max_batch=3, sampling=None, inference_head_num=2, head_num=3)
    mm = _mm(hvx_config=None, models=dict(llm=llm, flow=None, hift=None))
    q = queue.Queue()
    for t in tasks:
        q.put(t)
    q.put(None)
    results = _Log() if results is None else results
    tokens = {}
    stats = worker.serve_queue(mm, q, results, lm_slots=3, normalise=lambda s: s, token_log=tokens, segmented_text_chars=CHARS, **kw)
    return results, tokens, stats


def _wav(k, n=0):
    return torch.full((100 + 7 * k + n,), float(10 * (k + 1) + n))


# ---- 2: assembly and failure ------------------------------------------------------------------------------------------------------------------
def test_serve_queue_assembles_a_fanned_out_task_in_text_order(monkeypatch):
    segs = _segments()

    def script(utts, kw):
        assert 'stream' not in kw
        for key in (('long', 3), ('long', 0), ('short1', None), ('long', 5), ('long', 1), ('long', 4), ('long', 2)):
            k = key[1] if key[1] is not None else 9
            yield utts[key], _wav(k), [k, k + 1]
    random.seed(7)
    results, tokens, stats = _serve(monkeypatch, [_long(extra_params=dict(EP)), _short(1)], script, segment_fanout=True)
    gaps = _gaps(7, 5)
    assert results.writes == ['short1', 'long'] and (stats['epochs'], stats['epoch_boundaries'], stats['fanned_out'], stats['cancelled']) == (1, 0, 1, 0)
    r = results['long']
    assert set(r) == {'output_audio', 'sample_rate', 'format', 'duration', 'speaker_id', 'segments_info'} == set(results['short1'])
    parts = []
    for k in range(6):
        if k:
            parts.append(torch.zeros(1, gaps[k - 1]))
        parts.append(_wav(k)[None])
    want = torch.cat(parts, dim=-1)
    assert r['output_audio'].shape == want.shape and torch.equal(r['output_audio'], want)
    assert r['segments_info'] == {'total_segments': 6, 'segments': segs} and r['duration'] == want.shape[-1] / SR
    assert (r['sample_rate'], r['format'], r['speaker_id']) == (SR, 'wav', 's') and results['short1']['segments_info'] is None
    assert tokens == {'long': [[k, k + 1] for k in range(6)], 'short1': [9, 10]}
    # the switch off: the long task is a boundary and takes the one-by-one path (here: it fails, nothing is loaded), the short one is served after it
    results, tokens, stats = _serve(monkeypatch, [_short(0), _long(extra_params=dict(EP)), _short(1)],
                                    lambda utts, kw: ((u, _wav(9), [9, 10]) for u in utts.values()))
    assert (stats['epochs'], stats['epoch_boundaries'], stats['fanned_out']) == (2, 1, 0)
    assert results.writes == ['short0', 'long', 'short1'] and 'error' in results['long']


def test_serve_queue_answers_a_failed_segment_once_and_retires_the_siblings(monkeypatch):
    from flowmirror_hydravox_amd.llm import Cancelled
    seen = {}

    def script(utts, kw):
        fan = utts[('long', 0)].segment[0]
        seen['fan'] = fan
        yield utts[('long', 0)], _wav(0), [0]
        assert not fan.cancel.is_set()
        yield utts[('long', 2)], RuntimeError('boom'), []
        assert fan.cancel.is_set()                                              # siblings in flight are retired through the shared flag
        yield utts[('long', 1)], _wav(1), [1]                                   # ... and whatever they still deliver is discarded
        yield utts[('long', 3)], Cancelled([5, 6]), [5, 6]
        yield utts[('long', 4)], RuntimeError('late'), []
        yield utts[('short1', None)], _wav(9), [9]
        yield utts[('long', 5)], _wav(5), [5]
    results, tokens, stats = _serve(monkeypatch, [_long(extra_params=dict(EP)), _short(1)], script, segment_fanout=True)
    assert results.writes == ['long', 'short1'] and results['long'] == {'error': 'TTS failed: segment 3 failed: boom'}
    assert 'long' not in tokens and 'output_audio' in results['short1'] and stats['fanned_out'] == 1 and stats['cancelled'] == 0


# ---- 3: streamed ordering ----------------------------------------------------------------------------------------------------------------------
def test_serve_queue_streams_a_fanned_out_task_in_text_order(monkeypatch):
    from flowmirror_hydravox_amd.worker import stream_result_key
    segs = _segments()
    arrivals = [(1, 0, False), (0, 0, False), (1, 1, True), (2, 0, True), (0, 1, True), (5, 0, True), (4, 0, True), (3, 0, True)]

    def script(utts, kw):
        assert kw.get('stream') is True
        for k, n, final in arrivals:
            yield utts[('long', k)], _wav(k, n), dict(dict(index=n, final=final), **({'tokens': [k, n]} if final else {}))
    random.seed(3)
    results, tokens, stats = _serve(monkeypatch, [_long(extra_params=dict(EP))], script, segment_fanout=True, stream=True)
    gaps = _gaps(3, 5)
    order = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (3, 0), (4, 0), (5, 0)]      # text order, whatever the arrival order
    assert results.writes == [stream_result_key('long', i) for i in range(8)] and 'long' not in results
    for i, (k, n) in enumerate(order):
        m = results[stream_result_key('long', i)]
        assert set(m) == {'output_audio', 'sample_rate', 'format', 'duration', 'speaker_id', 'segments_info', 'piece_index', 'final'}
        assert m['piece_index'] == i and m['final'] == (i == 7)
        gap = gaps[k - 1] if k and n == 0 else 0                                 # the gap rides at the front of a later segment's first piece
        a = m['output_audio']
        assert a.shape == (1, gap + _wav(k, n).numel()) and not a[0, :gap].any() and torch.equal(a[0, gap:], _wav(k, n))
        assert m['duration'] == a.shape[1] / SR
        assert m['segments_info'] == ({'total_segments': 6, 'segments': segs} if i == 7 else None)
    assert tokens == {'long': [[0, 1], [1, 1], [2, 0], [3, 0], [4, 0], [5, 0]]}
    # held pieces: nothing of segment 1 left before segment 0 was final (arrival 5 of 8 is the first to release them)
    assert stats['fanned_out'] == 1


# ---- 4: the cancel task ------------------------------------------------------------------------------------------------------------------------
def test_cancel_task_in_an_epoch_unknown_target_and_outside_an_epoch(monkeypatch):
    from flowmirror_hydravox_amd.worker import CANCELLED_RESULT, _TaskSource
    assert CANCELLED_RESULT == {'error': 'cancelled', 'cancelled': True}
    # the target is in flight: its flag is set, both are answered, the epoch goes on
    q, results = queue.Queue(), {}
    src = _TaskSource(_mm(), q, results, _short(0), lambda s: s, 0)
    u0 = src.poll(False)
    assert not u0.cancel.is_set()
    for t in (dict(task_type='cancel', id='c1', target_id='short0'), dict(task_type='cancel', id='c2', target_id='nobody'),
              dict(task_type='cancel', id='c3', target_id='short0'), _short(1)):
        q.put(t)
    u1 = src.poll(False)
    assert u1.tag['id'] == 'short1' and not src.closed and src.carry is None and u0.cancel.is_set() and not u1.cancel.is_set()
    assert results == {'short0': CANCELLED_RESULT, 'c1': {'cancelled': True}, 'c2': {'cancelled': False}, 'c3': {'cancelled': False}}
    assert src.n_cancelled == 1 and not src.answer('short0', {'late': 1}) and results['short0'] == CANCELLED_RESULT
    # the target is still being expanded: the shared flag, and the cancel task is found although segments are waiting in front of the queue
    q, results = queue.Queue(), {}
    src = _TaskSource(_mm(), q, results, _long(), lambda s: s, 0, segment_fanout=True, segmented_text_chars=CHARS)
    s0 = src.poll(False)
    q.put(dict(task_type='cancel', id='c', target_id='long'))
    q.put(_short(1))
    nxt = src.poll(False)
    assert nxt.tag['id'] == 'short1' and s0.cancel.is_set() and results == {'long': CANCELLED_RESULT, 'c': {'cancelled': True}}
    # the look-ahead is bounded (the queue may be shared with other workers): it stops at the first item that is no cancel task and holds that one only
    q, results = queue.Queue(), {}
    src = _TaskSource(_mm(), q, results, _long(), lambda s: s, 0, segment_fanout=True, segmented_text_chars=CHARS)
    s0 = src.poll(False)
    for t in (_short(1), None, _short(2), None):
        q.put(t)
    s1 = src.poll(False)
    assert s1.segment[1] == 1 and [t['id'] for t in src.backlog] == ['short1'] and q.qsize() == 3
    assert [src.poll(False).segment[1] for _ in range(4)] == [2, 3, 4, 5] and q.qsize() == 3 and len(src.backlog) == 1
    assert src.poll(False).tag['id'] == 'short1' and q.qsize() == 3
    with pytest.raises(StopIteration):
        src.poll(False)
    assert src.stop and q.qsize() == 2 and not src.backlog                         # one sentinel taken, as a blocking get() takes one: the rest stays for the peers
    # through serve_queue: the cancelled task keeps its one answer whatever the engine still hands back for it; outside an epoch the answer is False
    from flowmirror_hydravox_amd.llm import Cancelled

    def script(utts, kw):
        assert utts[('short0', None)].cancel.is_set() and not utts[('short1', None)].cancel.is_set()
        yield utts[('short0', None)], Cancelled([1, 2]), [1, 2]
        yield utts[('short1', None)], _wav(9), [9]
    tasks = [dict(task_type='cancel', id='early', target_id='short0'), _short(0), dict(task_type='cancel', id='c', target_id='short0'), _short(1),
             dict(task_type='load_pt', id='swap', llm_pt='x', flow_pt='y'), dict(task_type='cancel', id='late', target_id='short1')]
    results, tokens, stats = _serve(monkeypatch, tasks, script)
    assert results['early'] == {'cancelled': False} and results['c'] == {'cancelled': True} and results['late'] == {'cancelled': False}
    assert results['short0'] == CANCELLED_RESULT and results.writes.count('short0') == 1 and 'output_audio' in results['short1']
    assert (stats['epochs'], stats['epoch_boundaries'], stats['cancelled'], stats['fanned_out']) == (1, 1, 1, 0) and set(tokens) == {'short1'}


# ---- the engine's and the pipeline's side, as far as the host can tell ------------------------------------------------------------------------
def test_serve_hands_a_cancelled_utterance_back_once_on_stand_in_models(tiny_cfg):
    """HvxPipeline.serve over stand-in models with a scripted LM: an utterance whose flag is set between its last token and its solve never reaches the
    acoustic stage and comes back as (utterance, Cancelled, ids); streamed, a cancelled utterance's unsolved chunk jobs are dropped and it comes back
    once as (utterance, Cancelled, {}); `cancelled` is counted and nothing is abandoned."""
    import threading
    from flowmirror_hydravox_amd.llm import Cancelled
    from flowmirror_hydravox_amd.pipeline import HvxPipeline, synthetic_utterance
    from test_stream_serve_host import FakeHift, ListSource, ScriptedLM, ServeFlow
    assert issubclass(Cancelled, Exception) and Cancelled([1, 2]).tokens == [1, 2] and Cancelled().tokens == []
    lengths = {0: 40, 1: 30, 2: 20}
    utts = [synthetic_utterance(tiny_cfg, k, 8) for k in range(3)]
    utts[1].cancel = threading.Event()
    utts[1].cancel.set()
    pipe = HvxPipeline.from_models(tiny_cfg, ScriptedLM(lengths), ServeFlow(), FakeHift(), acoustic_batch=4)
    out = {u.seed: (w, t) for u, w, t in pipe.serve(ListSource(utts), lm_slots=3)}
    want = torch.randint(0, 96, (30,), generator=torch.Generator().manual_seed(1)).tolist()
    assert isinstance(out[1][0], Cancelled) and out[1][0].tokens == out[1][1] == want
    assert all(isinstance(out[k][0], torch.Tensor) and out[k][0].numel() == 960 * lengths[k] for k in (0, 2))
    assert pipe.last_continuous['cancelled'] == 1 and pipe.last_continuous['abandoned'] == []

    class CancellingLM(ScriptedLM):
        def generate_stream(self, requests, n_slots=None, stream_tokens=False, **kw):
            d0, d1 = requests.poll(False), requests.poll(False)
            assert d0['cancel'] is utts[0].cancel and 'cancel' not in d1
            yield d0['tag'], list(range(30)), False                                         # a chunk of request 0 is ready ...
            d0['cancel'].set()                                                              # ... when its caller cancels it
            yield d1['tag'], list(range(30)), False
            yield d0['tag'], Cancelled(list(range(30))), True
            yield d1['tag'], list(range(30)), True
    utts = [synthetic_utterance(tiny_cfg, k, 8) for k in range(2)]
    utts[0].cancel = threading.Event()
    pipe = HvxPipeline.from_models(tiny_cfg, CancellingLM({}), ServeFlow(), FakeHift(), acoustic_batch=4)
    out = list(pipe.serve(ListSource(utts), lm_slots=2, stream=True))
    back = [(u.seed, p, i) for u, p, i in out if isinstance(p, BaseException)]
    assert len(back) == 1 and back[0][0] == 0 and isinstance(back[0][1], Cancelled) and back[0][2] == {}
    assert sum(p.numel() for u, p, _ in out if u.seed == 1) == 960 * 30
    assert pipe.last_continuous['cancelled'] == 1 and pipe.last_continuous['abandoned'] == []


def test_the_leave_export_is_declared_at_abi_7():
    """(the refusals of the native call — a null block, slots -1 and 3 — are asserted where the library certainly exists: tests/test_gpu_segment_fanout.py)"""
    from flowmirror_hydravox_amd import _lib
    assert len(_lib.SYMBOLS['hvx_llm_decode_leave'][1]) == 4 and _lib.HVX_ABI_VERSION >= 7
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'hvx.h')) as f:
        assert 'int hvx_llm_decode_leave(hvx_llm* h, hvx_stream s, const hvx_decode_args* a, int32_t slot);' in f.read()
