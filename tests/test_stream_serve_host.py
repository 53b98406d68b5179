"""Streaming from the continuous-batching server, host side (no GPU): the chunk schedule (`streaming.ChunkSchedule`) against the call log of the
`stream_tts` it was factored out of, `stream_tts` on stand-in models before and after the rewrite, `HvxPipeline.serve(stream=True)` on stand-in
models with a scripted LM, and the argument refusals of `ops.mel_cache_append`.

The fixture tests/golden/stream_schedule_calls.json is the call log of `stream_tts` as it stood BEFORE `ChunkSchedule` existed, recorded with the
stand-ins below (`python tests/test_stream_serve_host.py --mint` re-records it from whatever `stream_tts` is checked out).
"""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'stream_schedule_calls.json')
LOOK = 3


class FakeFlow:
    """records every call; frame j (counted after the prompt) of the mel it returns holds the value j in every row, so that the frames a
    session keeps tell which prefix it took as covered"""
    token_mel_ratio = 2
    pre_lookahead_len = LOOK
    device = 'cpu'

    def __init__(self):
        self.calls = []

    def inference(self, token, token_len, embedding, finalize=True, prompt_token=None, prompt_token_len=None, prompt_feat=None, prompt_feat_len=None,
                  streaming=False):
        n = int(token.shape[1])
        assert int(token_len[0]) == n
        self.calls.append([n, 0 if prompt_token is None else int(prompt_token.shape[1]), bool(streaming), bool(finalize)])
        n_out = n if finalize else n - self.pre_lookahead_len
        assert n_out > 0
        return torch.arange(self.token_mel_ratio * n_out, dtype=torch.float32).expand(1, 80, -1).clone(), None


class FakeHift:
    """records the frame ids it is given; finalize=False holds back 8 frames as the causal vocoder does; sample k holds the value k"""
    def __init__(self):
        self.calls = []

    def inference(self, speech_feat, finalize=True):
        ids = [int(v) for v in speech_feat[0, 0].tolist()]
        self.calls.append([ids, bool(finalize)])
        n = len(ids) if finalize else max(len(ids) - 8, 0)
        return torch.arange(480 * n, dtype=torch.float32)[None], None


def hop_of(cfg):
    return cfg.flow.static_chunk_size // cfg.flow.token_mel_ratio


def schedule_cases(hop):
    return [(p, n) for p in (0, 1, hop - 1, hop, hop + 1) for n in (1, hop + LOOK - 1, hop + LOOK, 3 * hop + LOOK + 1)]


def run_stream_tts(n_prompt, n_tokens, hop):
    """stream_tts on the stand-ins -> (jobs [(tokens in the piece, covered, chunk mask, final)], piece lengths, first sample of every piece)"""
    from flowmirror_hydravox_amd.streaming import stream_tts
    flow, hift = FakeFlow(), FakeHift()
    g = torch.Generator().manual_seed(1000 * n_prompt + n_tokens)
    toks = torch.randint(0, 96, (n_tokens,), generator=g).tolist()
    pieces = list(stream_tts(iter(toks), flow, hift, torch.zeros(1, n_prompt, dtype=torch.int32), torch.zeros(1, 2 * n_prompt, 80), torch.zeros(1, 192),
                             token_hop_len=hop))
    assert len(flow.calls) == len(hift.calls) == len(pieces)
    jobs, have = [], 0
    for (n, n_p, streaming, fin), (ids, hfin) in zip(flow.calls, hift.calls):
        assert n_p == n_prompt and hfin == fin
        fresh = ids[have:]
        assert ids[:have] == list(range(have)) and fresh == list(range(fresh[0], fresh[0] + len(fresh))) if fresh else True
        covered = (fresh[0] if fresh else have) // 2
        jobs.append([n, covered, streaming, fin])
        have = len(ids)
    return jobs, [int(p.shape[1]) for p in pieces], [int(p[0, 0]) if p.shape[1] else -1 for p in pieces]


def mint():
    from flowmirror_hydravox_amd.config import tiny_config
    hop = hop_of(tiny_config())
    cases = []
    for p, n in schedule_cases(hop):
        jobs, lens, firsts = run_stream_tts(p, n, hop)
        cases.append(dict(n_prompt=p, n_tokens=n, jobs=jobs, piece_lens=lens, piece_first=firsts))
    with open(FIXTURE, 'w') as f:
        json.dump(dict(token_hop_len=hop, pre_lookahead_len=LOOK, cases=cases), f, indent=0)
    print('wrote', FIXTURE, len(cases), 'cases')


# ------------------------------------------------------------------------------------------------------------------------
# 1 / 2: the schedule, and stream_tts on top of it, against the recorded call log
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def _schedule_jobs(n_prompt, n_tokens, hop, burst):
    from flowmirror_hydravox_amd.streaming import ChunkSchedule
    sched = ChunkSchedule(n_prompt, hop, LOOK)
    ids = list(range(n_tokens))
    jobs = []
    for a in range(0, n_tokens, burst):
        jobs += [[n, c, True, False] for n, c in sched.feed(ids[a:a + burst])]
    n, c = sched.finish()
    assert sched.tokens == ids
    return jobs + [[n, c, False, True]]


def test_chunk_schedule_reproduces_the_recorded_jobs(tiny_cfg, recorded):
    hop = hop_of(tiny_cfg)
    assert recorded['token_hop_len'] == hop == 25 and recorded['pre_lookahead_len'] == tiny_cfg.flow.pre_lookahead_len == LOOK
    assert [(c['n_prompt'], c['n_tokens']) for c in recorded['cases']] == schedule_cases(hop)
    assert max(len(c['jobs']) for c in recorded['cases']) >= 4             # (the longest case really has several chunks)
    for c in recorded['cases']:
        one = _schedule_jobs(c['n_prompt'], c['n_tokens'], hop, 1)
        eight = _schedule_jobs(c['n_prompt'], c['n_tokens'], hop, 8)
        assert one == c['jobs'], (c['n_prompt'], c['n_tokens'], one, c['jobs'])
        assert eight == one, (c['n_prompt'], c['n_tokens'])


def test_stream_tts_pieces_unchanged_by_the_rewrite(tiny_cfg, recorded):
    hop = hop_of(tiny_cfg)
    for c in recorded['cases']:
        jobs, lens, firsts = run_stream_tts(c['n_prompt'], c['n_tokens'], hop)
        assert jobs == c['jobs'] and lens == c['piece_lens'] and firsts == c['piece_first'], (c['n_prompt'], c['n_tokens'])


# ------------------------------------------------------------------------------------------------------------------------
# 3: serve(stream=True) over stand-in models and a scripted LM
# ------------------------------------------------------------------------------------------------------------------------
class ServeFlow(FakeFlow):
    """FakeFlow plus what the serving engine calls: encode / solve_stream_batch (streamed) and inference_batch (unstreamed)"""
    static_chunk_size = 50
    output_size = 80

    def __init__(self):
        super().__init__()
        self.solves = []

    def encode(self, token, embedding, finalize=True):
        n = int(token.numel()) - (0 if finalize else self.pre_lookahead_len)
        assert n > 0
        return torch.arange(2 * n, dtype=torch.float32).expand(80, -1).clone(), torch.zeros(80)

    def solve_stream_batch(self, mus, spks, conds, covered, caches, cache_fill, streaming=True):
        self.solves.append((len(mus), bool(streaming)))
        fresh = []
        for mu, cov, cache, fill in zip(mus, covered, caches, cache_fill):
            T = mu.shape[-1]
            assert 0 <= cov <= T and fill + T - cov <= cache.shape[1]
            cache[:, fill:fill + T - cov] = mu[:, cov:]
            fresh.append(T - cov)
        return fresh

    def inference_batch(self, tokens, embeddings, prompt_tokens=None, prompt_feats=None, streaming=False):
        return [torch.arange(2 * int(t.numel()), dtype=torch.float32).expand(1, 80, -1).clone() for t in tokens]


class ScriptedLM:
    """generate_stream of an LM whose requests decode side by side: request k gets `lengths[k]` ids, handed over in bursts of 8 per round"""
    device = 'cpu'
    max_batch = 4
    last_stats = {}

    def __init__(self, lengths):
        self.lengths = lengths

    def generate_stream(self, requests, n_slots=None, stream_tokens=False, **kw):
        reqs = []
        while True:
            try:
                d = requests.poll(False)
            except StopIteration:
                break
            if d is not None:
                reqs.append(d)
        ids = {d['tag']: torch.randint(0, 96, (self.lengths[int(d['seed'])],), generator=torch.Generator().manual_seed(int(d['seed']))).tolist() for d in reqs}
        sent = {t: 0 for t in ids}
        while sent:
            for t in list(sent):
                new = ids[t][sent[t]:sent[t] + 8]
                sent[t] += len(new)
                if stream_tokens and new:
                    yield t, new, False
                if sent[t] >= len(ids[t]):
                    del sent[t]
                    yield (t, ids[t], True) if stream_tokens else (t, ids[t])


class ListSource:
    def __init__(self, items):
        self.it = iter(items)

    def poll(self, block):
        return next(self.it)


def _stand_in_pipeline(tiny_cfg, lengths):
    from flowmirror_hydravox_amd.pipeline import HvxPipeline
    return HvxPipeline.from_models(tiny_cfg, ScriptedLM(lengths), ServeFlow(), FakeHift(), acoustic_batch=4)


def _utterances(tiny_cfg):
    from flowmirror_hydravox_amd.pipeline import synthetic_utterance
    utts = [synthetic_utterance(tiny_cfg, k, 8, n_prompt_speech=26 if k == 1 else 0, n_prompt_text=3 if k == 1 else 0) for k in range(4)]
    utts[3].speed = 1.5
    return utts


def test_serve_stream_on_stand_in_models(tiny_cfg):
    lengths = {0: 79, 1: 60, 2: 5, 3: 40}
    pipe = _stand_in_pipeline(tiny_cfg, lengths)
    utts = _utterances(tiny_cfg)
    got = {}
    refused = []
    ev = []
    for u, piece, info in pipe.serve(ListSource(utts), lm_slots=3, stream=True, event_log=ev):
        k = u.seed
        if isinstance(piece, BaseException):
            refused.append((k, piece, info))
            continue
        got.setdefault(k, []).append((piece, info))
    # the utterance with a speed change: the reference's assertion, the others complete
    assert [k for k, _, _ in refused] == [3] and isinstance(refused[0][1], AssertionError) and refused[0][2] == {}
    assert str(refused[0][1]) == 'speed change only support non-stream inference mode'
    assert sorted(got) == [0, 1, 2]
    hop = hop_of(tiny_cfg)
    total = 0
    for k in (0, 1, 2):
        infos = [i for _, i in got[k]]
        assert [i['index'] for i in infos] == list(range(len(infos)))                       # in order
        assert [i['final'] for i in infos] == [False] * (len(infos) - 1) + [True]           # exactly one final piece, the last
        assert all('tokens' not in i for i in infos[:-1])
        want = torch.randint(0, 96, (lengths[k],), generator=torch.Generator().manual_seed(k)).tolist()
        assert infos[-1]['tokens'] == want                                                  # ... and it carries the full token list
        # the pieces stream_tts hands out for these tokens alone
        from flowmirror_hydravox_amd.streaming import stream_tts
        n_p = 26 if k == 1 else 0
        alone = list(stream_tts(iter(want), FakeFlow(), FakeHift(), torch.zeros(1, n_p, dtype=torch.int32), torch.zeros(1, 2 * n_p, 80), torch.zeros(1, 192),
                                token_hop_len=hop))
        assert [int(p.numel()) for p, _ in got[k]] == [int(a.shape[1]) for a in alone], k
        assert torch.equal(torch.cat([p for p, _ in got[k]]), torch.cat(alone, dim=1)[0])
        total += len(infos)
    assert len(got[0]) == 4 and len(got[2]) == 1
    lc = pipe.last_continuous
    assert lc['pieces'] == total and lc['abandoned'] == [] and lc['pieces_out'] == []
    # (whether chunks of different utterances meet in one solve is a matter of timing with an LM that costs nothing: the GPU test asserts it)
    assert 0 < lc['chunk_solves'] == len(pipe.flow.solves) <= total and sum(n for n, _ in pipe.flow.solves) == total
    assert sorted(n for n, _ in lc['first_piece_seconds']) == [0, 1, 2] and all(s >= 0 for _, s in lc['first_piece_seconds'])
    assert 'events' not in lc
    assert lc['tokens'] == sum(lengths[k] for k in (0, 1, 2))
    # the log: every piece of an utterance after tokens of it, the first piece of utterance 0 before its 'done'
    assert ev.index(('piece', 0, 0, False)) > min(i for i, e in enumerate(ev) if e[0] == 'tokens' and e[1] == 0)


def test_serve_stream_sizes_the_mel_cache_from_the_call_ratio(tiny_cfg):
    """utterances without a ratio of their own decode up to text x serve's max_token_text_ratio tokens: the cache plane must hold them (it is the flow
    stand-in's assert, and the native call's refusal, that an overflow trips)"""
    from flowmirror_hydravox_amd.pipeline import synthetic_utterance
    utts = [synthetic_utterance(tiny_cfg, k, 2) for k in range(2)]
    assert all(u.max_token_text_ratio is None for u in utts)
    lengths = {0: 60, 1: 41}                                                                # 2 text tokens x ratio 30 = 60 > 2 x 20
    pipe = _stand_in_pipeline(tiny_cfg, lengths)
    planes = []
    solve = pipe.flow.solve_stream_batch
    pipe.flow.solve_stream_batch = lambda mus, spks, conds, covered, caches, fill, streaming=True: (planes.extend(c.shape[1] for c in caches),
                                                                                                  solve(mus, spks, conds, covered, caches, fill, streaming))[1]
    got = {}
    for u, piece, info in pipe.serve(ListSource(utts), lm_slots=2, stream=True, max_token_text_ratio=30):
        assert not isinstance(piece, BaseException), piece
        got.setdefault(u.seed, []).append(piece)
    assert {k: sum(p.numel() for p in v) for k, v in got.items()} == {0: 960 * 60, 1: 960 * 41}
    assert set(planes) == {2 * 60}
    # with max_out the plane is sized from it
    planes.clear()
    for u, piece, info in pipe.serve(ListSource(utts), lm_slots=2, stream=True, max_token_text_ratio=30, max_out=70):
        assert not isinstance(piece, BaseException), piece
    assert set(planes) == {2 * 70}


def test_serve_stream_drops_a_session_that_fails_after_its_tokens(tiny_cfg):
    """an error for a request whose chunks were already scheduled ends that request only"""
    class FailingLM(ScriptedLM):
        def generate_stream(self, requests, n_slots=None, stream_tokens=False, **kw):
            d0, d1 = requests.poll(False), requests.poll(False)
            yield d0['tag'], list(range(30)), False                                         # a chunk of request 0 is ready ...
            yield d0['tag'], RuntimeError('lost'), True                                     # ... when it fails
            yield d1['tag'], list(range(30)), False
            yield d1['tag'], list(range(30)), True
    from flowmirror_hydravox_amd.pipeline import HvxPipeline, synthetic_utterance
    pipe = HvxPipeline.from_models(tiny_cfg, FailingLM({}), ServeFlow(), FakeHift(), acoustic_batch=4)
    utts = [synthetic_utterance(tiny_cfg, k, 8) for k in range(2)]
    out = list(pipe.serve(ListSource(utts), lm_slots=2, stream=True))
    errs = [(u.seed, str(p)) for u, p, _ in out if isinstance(p, BaseException)]
    assert errs == [(0, 'lost')]
    assert all(u.seed == 1 for u, p, _ in out if not isinstance(p, BaseException))
    assert sum(p.numel() for u, p, _ in out if not isinstance(p, BaseException)) == 960 * 30
    assert pipe.last_continuous['abandoned'] == []


def test_serve_queue_stream_writes_one_message_per_piece(tiny_cfg):
    """worker.serve_queue(stream=True) over the stand-in pipeline: every piece under stream_result_key(id, index) with the unstreamed keys plus piece_index / final,
    the token log on the final piece, a failing request answered once under its task id"""
    import queue
    import types
    from flowmirror_hydravox_amd import worker

    class Frontend:
        def text_normalize(self, text, split=True, text_frontend=True):
            return [text] if split else text

        def frontend_sft(self, text, spk_id):
            return dict(text=torch.tensor([[ord(c) % 90 for c in text]], dtype=torch.int32), flow_embedding=torch.zeros(192))
    lengths = {0: 79, 1: 30, 2: 40}
    llm = ScriptedLM(lengths)
    llm.sampling, llm.inference_head_num = None, 2
    mm = types.SimpleNamespace(frontend=Frontend(), configs={'sample_rate': 24000}, is_loaded=True, get_available_speakers=lambda: ['s'], hvx_config=tiny_cfg,
                               models=dict(llm=llm, flow=ServeFlow(), hift=FakeHift()))
    q, results, tokens = queue.Queue(), {}, {}
    q.put(dict(id='a', task_type='tts', text='hello you', speaker_id='s', seed=0))
    q.put(dict(id='b', task_type='tts', text='and you', speaker_id='s', seed=1))
    q.put(dict(id='c', task_type='tts', text='too fast', speaker_id='s', seed=2,
               extra_params=dict(top_p=0.8, top_k=25, win_size=10, tau_r=0.1, inference_head_num=2, speed=1.5)))
    q.put(None)
    import functools
    from flowmirror_hydravox_amd.sampling import ras_sampling
    llm.sampling = functools.partial(ras_sampling, top_p=0.8, top_k=25, win_size=10, tau_r=0.1)
    stats = worker.serve_queue(mm, q, results, lm_slots=3, normalise=lambda s_: s_, token_log=tokens, stream=True)
    assert stats['epochs'] >= 1
    want = {k: torch.randint(0, 96, (lengths[k],), generator=torch.Generator().manual_seed(k)).tolist() for k in (0, 1)}
    for tid, k, n_pieces in (('a', 0, 4), ('b', 1, 2)):
        msgs = [results[worker.stream_result_key(tid, i)] for i in range(n_pieces)]
        assert worker.stream_result_key(tid, n_pieces) not in results and tid not in results
        assert [m['piece_index'] for m in msgs] == list(range(n_pieces)) and [m['final'] for m in msgs] == [False] * (n_pieces - 1) + [True]
        for m in msgs:
            assert set(m) == {'output_audio', 'sample_rate', 'format', 'duration', 'speaker_id', 'segments_info', 'piece_index', 'final'}
            assert m['output_audio'].dim() == 2 and m['duration'] == m['output_audio'].shape[1] / 24000 and m['format'] == 'wav'
        assert sum(m['output_audio'].shape[1] for m in msgs) == 960 * lengths[k]
        assert tokens[tid] == want[k]
    assert set(results['c']) == {'error'} and 'speed change only support non-stream inference mode' in results['c']['error']
    assert not any(str(key).startswith('c:') for key in results) and 'c' not in tokens


def test_serve_without_stream_is_unchanged_on_stand_in_models(tiny_cfg):
    lengths = {0: 79, 1: 60, 2: 5, 3: 40}
    pipe = _stand_in_pipeline(tiny_cfg, lengths)
    utts = _utterances(tiny_cfg)
    utts[3].speed = 1.0                                                                     # (the speed change of the unstreamed path is a device kernel)
    out = list(pipe.serve(ListSource(utts), lm_slots=3))
    assert len(out) == 4
    for item in out:
        assert isinstance(item, tuple) and len(item) == 3
        u, wav, toks = item
        want = torch.randint(0, 96, (lengths[u.seed],), generator=torch.Generator().manual_seed(u.seed)).tolist()
        assert toks == want and isinstance(wav, torch.Tensor) and wav.dim() == 1
        assert wav.numel() == 480 * 2 * len(want)
    assert set(pipe.last_continuous) == {'tokens', 'audio_seconds', 'acoustic_seconds', 'total_seconds', 'llm_seconds', 'llm', 'lm_slots', 'abandoned'}
    assert pipe.flow.solves == []                                                           # the streaming stage never ran


# ------------------------------------------------------------------------------------------------------------------------
# 4: refusals of the cache append, before any launch
# ------------------------------------------------------------------------------------------------------------------------
def test_mel_cache_append_refusals():
    import ctypes as C
    from flowmirror_hydravox_amd import _lib, ops
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libhvx.so is not built (python -m flowmirror_hydravox_amd.build)')
    lib = _lib.load()
        # (device memory where there is a device: if a check ever let one of these through, the launch would copy inside real planes and the assert below
    # would fail; without a device nothing can be launched at all)
    dev = 'cuda' if torch.cuda.is_available() else 'cpu'
    x = torch.zeros(2, 80, 37, device=dev)
    caches = [torch.zeros(80, 64, device=dev)[:, :16].contiguous() for _ in range(2)]

    def call(t_len, covered, fill, n=2):
        tl, cov, pa, ld, fl = ops.mel_append_block(t_len, covered, caches[:len(t_len)], fill)
        return lib.hvx_op_mel_cache_append(C.c_void_p(x.data_ptr()), n, 80, 37, tl, cov, pa, ld, fl, None)
    assert call([10, 20], [0, 3], [0, 0]) == -1 and b'overflow' in lib.hvx_last_error()             # 17 frames into a row of 16
    assert call([10, 17], [0, 1], [6, 1]) == -1 and b'overflow' in lib.hvx_last_error()             # 10 frames at column 6, and 16 at column 1
    assert call([10, 5], [0, 6], [0, 0]) == -1 and b'covered' in lib.hvx_last_error()               # covered > t_len
    assert call([10, 38], [0, 30], [0, 0]) == -1 and b't_len' in lib.hvx_last_error()               # longer than the planes of x
    assert call([], [], [], n=0) == -1 and b'sessions' in lib.hvx_last_error()
    assert call([10, 5], [0, 5], [0, 0], n=-1) == -1
    # the solve refuses the same before it touches its handle's state (a null handle is refused first of all)
    assert lib.hvx_cfm_solve_stream_batch(None, None, None, 0, 2, 37, None, None, None, None, None, 10, None, None, 0, None, None, None, None) == -1
    with pytest.raises(ValueError):
        ops.mel_append_block([1], [0, 0], caches, [0, 0])



if __name__ == '__main__':
    if '--mint' in sys.argv:
        sys.path.insert(0, ROOT)
        mint()
    sys.exit(0)
