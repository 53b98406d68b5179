"""Segmented long texts in the decode grid, and retiring ONE request of a running grid (sampler.hip: decode_leave_kernel, hvx_llm_decode_leave; llm.py:
Cancelled, the `cancel` object of a request; pipeline.py: Utterance.cancel; worker.serve_queue(segment_fanout=True)).

Everything runs on the tiny configuration with three slots.  Ids are compared exactly (fp32 LM; truth for the C-level test is oracle/llm_ref.py run per
request on the CPU), waveforms with torch.equal — the bound the project already uses for batched against serial synthesis."""
import ctypes as C
import os
import queue
import random
import sys
import threading
import types
from functools import partial

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))

SP = dict(top_k=25, top_p=0.8, win_size=10, tau_r=0.1)
WIN_CAP = 16
RATIO = 4                                # mixed_heads_cases.oracle_stream decodes min = max = 4 tokens per text token: the lengths are exact
TEXT = 'alpha beta gamma, delta epsilon zeta. eta theta iota; kappa lambda mu! nu xi omicron pi? rho sigma tau upsilon.'


@pytest.fixture(scope='module')
def lm(tiny_cfg):
    """one fp32 tiny LM (3 heads) and the state dict the oracle reads"""
    from flowmirror_hydravox_amd import weights as W
    from flowmirror_hydravox_amd.llm import HvxLLM
    from flowmirror_hydravox_amd.sampling import ras_sampling
    cfg = tiny_cfg.llm
    assert cfg.head_num == 3
    sd = W.make_llm_state(cfg, seed=5, init='fan_in', with_lm_head=True)
    llm = HvxLLM(cfg, sd, dtype=torch.float32, max_batch=3, max_ctx=512, inference_head_num=2)
    llm.sampling = partial(ras_sampling, **SP)
    return llm, sd


# ---- 5: hvx_llm_decode_leave ------------------------------------------------------------------------------------------------------------------
LEAVE = ((15, 11, 2), (17, 12, 3), (16, 13, 2))          # (text tokens, seed, heads) of the requests in slots 0, 1, 2


@pytest.fixture(scope='module')
def leave_case(tiny_cfg, lm):
    """texts and the oracle's ids of the three requests — computed once, shared, never modified"""
    from mixed_heads_cases import oracle_stream
    gen = torch.Generator().manual_seed(77)
    texts = [torch.randint(0, tiny_cfg.llm.text_vocab, (n,), generator=gen, dtype=torch.int32) for n, _, _ in LEAVE]
    ids = tuple(tuple(int(t) for t in oracle_stream(lm[1], tiny_cfg.llm, texts[i], LEAVE[i][1], dict(SP), LEAVE[i][2])) for i in range(3))
    assert [len(x) for x in ids] == [n * RATIO for n, _, _ in LEAVE]
    return texts, ids


def test_decode_leave_retires_one_slot_and_leaves_the_neighbours_alone(lm, leave_case):
    """Requests 0 and 2 (2 heads) decode in slots 0 and 2 of a 3-slot grid, request 1 (3 heads) in slot 1; after two blocks of 8 steps slot 1 is retired
    with hvx_llm_decode_leave and three more blocks run — with heads_live = 2, which no longer covers the retired slot's 3 heads.  Slots 0 and 2 give the
    oracle's ids with and without the leave; slot 1's row is "done, retired by the caller" with everything else as the leave found it, its ids a prefix of
    what it decodes when left alone (the oracle's); a leave of slot -1 or 3 is refused and launches nothing; the slot can be joined again."""
    from flowmirror_hydravox_amd import _lib
    from flowmirror_hydravox_amd.llm import _DecodeEngine, _Request
    from flowmirror_hydravox_amd.sampling import NoiseStream
    llm = lm[0]
    texts, want = leave_case

    def request(i):
        n = LEAVE[i][0]
        r = _Request(llm._encode_prefix(texts[i], None, None), n, n * RATIO, n * RATIO, NoiseStream(seed=LEAVE[i][1], chunk=8192))
        r.set_sampling(dict(SP))
        r.heads = LEAVE[i][2]
        return r

    def run(leave):
        eng = _DecodeEngine(llm, n_slots=3, max_out=128, max_prefix=64, mixed_sampling=True, win_cap=WIN_CAP, mixed_heads=True, head_cap=3)
        rs = [request(i) for i in range(3)]
        S, K = 3, 3
        info = {}
        with torch.cuda.stream(eng.stream):
            for slot in (0, 2, 1):
                eng._join(slot, rs[slot], 0)
            eng._publish_limits()
            s = C.c_void_p(eng.stream.cuda_stream)
            assert eng.seq_heads.cpu().tolist() == [2, 3, 2]

            def steps(heads_live):
                _lib.check(llm.lib.hvx_llm_decode_steps_mixed(llm._h, s, C.byref(eng.args), C.byref(eng.seq), C.byref(eng.hd), heads_live, 8), 'hvx_llm_decode_steps_mixed')

            def snapshot():
                eng.stream.synchronize()
                ctl = eng.ctl_dev.cpu()
                return dict(ctl=ctl, state=ctl[eng.o_state:eng.o_state + 8 * S].view(S, 8).clone(), tok=ctl[eng.o_tok:eng.o_tok + S * K].view(S, K).clone(),
                            ctrl=ctl[eng.o_ctrl:eng.o_ctrl + 5 * S].view(5, S).clone(), act=ctl[eng.o_act:eng.o_act + S].clone(),
                            hist=ctl[eng.o_hist:eng.o_hist + S * WIN_CAP].view(S, WIN_CAP).clone(), cur=eng.cur_dev.cpu(), out=eng.out_dev.cpu(),
                            heads=eng.seq_heads.cpu(), top_k=eng.seq_top_k.cpu())
            for blk in range(5):
                if leave and blk == 2:
                    before = snapshot()
                    for bad in (-1, 3):                                      # refused: non-zero, a message, nothing launched
                        assert llm.lib.hvx_llm_decode_leave(llm._h, s, C.byref(eng.args), bad) != 0
                        assert b'slot %d' % bad in llm.lib.hvx_last_error()
                    assert llm.lib.hvx_llm_decode_leave(llm._h, s, None, 1) != 0
                    assert torch.equal(snapshot()['ctl'], before['ctl'])
                    _lib.check(llm.lib.hvx_llm_decode_leave(llm._h, s, C.byref(eng.args), 1), 'hvx_llm_decode_leave')
                    info['before'], info['left'] = before, snapshot()
                steps(2 if leave and blk >= 2 else 3)
            info['end'] = snapshot()
            if leave:                                                        # the retired slot is joined again and decodes as ever
                again = request(1)
                eng._join(1, again, 5)
                eng._publish_limits()
                for blk in range(3):
                    steps(3)
                info['again'] = snapshot()
                again.noise.finalize(0)
        for r in rs:
            r.noise.finalize(0)
        return info
    alone, left = run(False), run(True)
    for info in (alone, left):
        st, out = info['end']['state'], info['end']['out']
        for slot in (0, 2):                                                  # bit for bit the oracle's ids, with and without the leave next door
            assert int(st[slot, 2]) == 1 and out[slot, :int(st[slot, 1])].tolist() == list(want[slot]), slot
    st = alone['end']['state']
    assert int(st[1, 7]) == 0 and alone['end']['out'][1, :int(st[1, 1])].tolist() == list(want[1])          # left alone, slot 1 finishes with the oracle's ids
    b, l, e = left['before'], left['left'], left['end']
    pos, n = int(b['state'][1, 0]), int(b['state'][1, 1])
    assert n == 2 * 8 * 3 < len(want[1]) and int(b['state'][1, 2]) == 0 and int(b['act'][1]) == 1           # 16 steps x 3 heads, still live
    for snap in (l, e):
        assert snap['state'][1].tolist() == [pos, n, 1, int(b['state'][1, 3]), int(b['state'][1, 4]), int(b['state'][1, 5]), 0, 1]
        assert snap['tok'][1].tolist() == [-1, -1, -1] and snap['ctrl'][:, 1].tolist() == [1, pos, 0, pos, -1] and int(snap['act'][1]) == 0
        assert torch.equal(snap['hist'][1], b['hist'][1]) and int(snap['cur'][1]) == int(b['cur'][1])       # ring and cursor untouched
        assert torch.equal(snap['heads'], b['heads']) and torch.equal(snap['top_k'], b['top_k'])
        assert snap['out'][1, :n].tolist() == list(want[1][:n])                                            # the ids decoded so far: a prefix of the full run
    assert int(b['state'][1, 5]) == 16
    # the leave touched nothing of the neighbours
    for slot in (0, 2):
        assert torch.equal(l['state'][slot], b['state'][slot]) and torch.equal(l['tok'][slot], b['tok'][slot]) and torch.equal(l['ctrl'][:, slot], b['ctrl'][:, slot])
    a = left['again']
    assert a['state'][1, 2] == 1 and int(a['state'][1, 7]) == 0 and a['out'][1, :int(a['state'][1, 1])].tolist() == list(want[1])


# ---- 6: the engine -----------------------------------------------------------------------------------------------------------------------------
def _grid_requests(cfg, cancel=None):
    """five requests: request 1 is the only 3-head one and by far the longest (400 ids, 134 steps: it outlives two rounds of the others, ~60 steps)"""
    gen = torch.Generator().manual_seed(91)
    reqs = []
    for i, n in enumerate((15, 100, 14, 16, 15)):
        reqs.append(dict(text=torch.randint(0, cfg.text_vocab, (n,), generator=gen, dtype=torch.int32), seed=500 + i, tag=i, max_token_text_ratio=RATIO,
                         min_token_text_ratio=RATIO, inference_head_num=3 if i == 1 else 2))
    if cancel is not None:
        reqs[1]['cancel'] = cancel
    return reqs


def test_engine_retires_a_cancelled_request_and_hands_its_slot_on(tiny_cfg, lm):
    from flowmirror_hydravox_amd.llm import Cancelled
    llm, cfg = lm[0], tiny_cfg.llm
    whole = {}
    for tag, ids, done in llm.generate_stream(iter(_grid_requests(cfg)), n_slots=3, stream_tokens=True, mixed_heads=True):
        if done:
            whole[tag] = ids
    st0 = dict(llm.last_stats)
    assert sorted(whole) == list(range(5)) and all(len(whole[i]) == RATIO * n for i, n in enumerate((15, 100, 14, 16, 15)))
    assert st0['cancelled'] == 0 and st0['requests'] == 5 and st0['head_runs'][-1][0] == 3              # left alone, the 3-head request is the last one live
    # the consumer cancels request 1 when its first increment arrives
    flag = threading.Event()
    parts, final = {}, {}
    for tag, ids, done in llm.generate_stream(iter(_grid_requests(cfg, flag)), n_slots=3, stream_tokens=True, mixed_heads=True):
        if done:
            assert tag not in final
            final[tag] = ids
        else:
            assert tag not in final
            parts.setdefault(tag, []).extend(ids)
            if tag == 1:
                flag.set()
    st = dict(llm.last_stats)
    assert isinstance(final[1], Cancelled) and final[1].tokens == parts[1]                               # the increments already yielded stay valid
    assert 0 < len(parts[1]) < len(whole[1]) and parts[1] == whole[1][:len(parts[1])]
    for i in (0, 2, 3, 4):
        assert final[i] == whole[i] == parts[i], i
    assert st['cancelled'] == 1 and st['requests'] == 4 and st['clean']
    assert st['head_runs'][0][0] == 3 and st['head_runs'][-1][0] == 2, st['head_runs']                   # heads_live is computed without the retired request
    assert st['steps'] < st0['steps']
    slot = dict((t, s) for t, s in st['joins'])[1]
    on_slot = [t for t, s in st['joins'] if s == slot]
    assert on_slot[0] == 1 and len(on_slot) >= 2 and len(st['joins']) == 5                                # the slot went to a waiting request
    # a request that arrives already cancelled never takes a slot; without stream_tokens the result is (tag, Cancelled)
    reqs = _grid_requests(cfg)[2:]
    gone = threading.Event()
    gone.set()
    reqs.insert(1, dict(reqs[0], tag='gone', cancel=gone))
    got = dict(llm.generate_stream(iter(reqs), n_slots=3, mixed_heads=True))
    st = llm.last_stats
    assert isinstance(got['gone'], Cancelled) and got['gone'].tokens == [] and 'gone' not in [t for t, _ in st['joins']] and len(st['joins']) == 3
    assert st['cancelled'] == 1 and all(got[i] == whole[i] for i in (2, 3, 4))


# ---- 7 / 8: the worker and the pipeline --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def pipe(tiny_cfg):
    from flowmirror_hydravox_amd.pipeline import HvxPipeline
    return HvxPipeline(tiny_cfg, llm_dtype=torch.float32, flow_dtype=torch.float32, max_batch=3, max_ctx=4096, max_t=1024, seed=7, init='fan_in',
                       inference_head_num=2)


def test_worker_serves_a_segmented_task_in_the_grid(tiny_cfg, pipe):
    """The example task (6 segments, seed 300) with one short task in front of it and two behind, through serve_queue(segment_fanout=True,
    segmented_text_chars=100, lm_slots=3): ONE epoch, no boundary, and the task's audio is the six segments served as plain `tts` tasks by the default
    worker (seeds segment_seeds(300, 6)) with the replayed gaps between them, sample for sample.  The same queue with the switch off: the long task
    closes the running epoch (1 boundary) and the short tasks sound the same.  (The short task in front is what makes the long one a BOUNDARY with the
    switch off: `epoch_boundaries` counts tasks that closed a running grid, and a long task at the head of the queue closes none.)"""
    from flowmirror_hydravox_amd.model_manager import segments_of
    from flowmirror_hydravox_amd.worker import segment_seeds, serve_queue
    from test_host_cpu import _QueueFrontend
    c = tiny_cfg

    class FE(_QueueFrontend):
        def _ids(self, text):
            return torch.tensor([[(ord(ch) * 7) % c.llm.text_vocab for ch in text]], dtype=torch.int32)

        def frontend_sft(self, text, spk_id):
            g = torch.Generator().manual_seed(len(spk_id))
            return dict(text=self._ids(text), text_len=torch.tensor([len(text)], dtype=torch.int32), llm_embedding=torch.zeros(0, 192),
                        flow_embedding=torch.randn(192, generator=g))
    mm = types.SimpleNamespace(frontend=FE(), configs={'sample_rate': c.sample_rate}, is_loaded=True, get_available_speakers=lambda: ['spk0', 'spk1'],
                               hvx_config=c, device=DEV, models=dict(llm=pipe.llm, flow=pipe.flow, hift=pipe.hift))
    ep = dict(top_p=0.8, top_k=25, win_size=10, tau_r=0.1, inference_head_num=2)
    segs = segments_of(TEXT)
    assert len(TEXT) == 111 and len(segs) == 6
    shorts = [dict(id='s%d' % i, task_type='tts', text=t, speaker_id='spk1', extra_params=dict(ep), seed=40 + i) for i, t in enumerate(('hello', 'one grid', 'lazy dogs'))]
    long_task = dict(id='long', task_type='tts', text=TEXT, speaker_id='spk0', extra_params=dict(ep), seed=300)

    def serve(tasks, **kw):
        q, results, toks = queue.Queue(), {}, {}
        for t in tasks:
            q.put(dict(t))
        q.put(None)
        stats = serve_queue(mm, q, results, worker_id=0, lm_slots=3, acoustic_batch=2, normalise=lambda s: s, token_log=toks, segmented_text_chars=100, **kw)
        return results, toks, stats
    mixed = [shorts[0], long_task, shorts[1], shorts[2]]
    random.seed(2024)
    r1, k1, s1 = serve(mixed, segment_fanout=True)
    random.seed(2024)
    gaps = [int(random.uniform(50, 150) * c.sample_rate / 1000) for _ in range(5)]
    plain = [dict(long_task, id='seg%d' % k, text=segs[k], seed=seed) for k, seed in enumerate(segment_seeds(300, 6))]
    r0, k0, s0 = serve(plain + shorts)
    assert not any('error' in r for r in list(r0.values()) + list(r1.values())), [r for r in list(r0.values()) + list(r1.values()) if 'error' in r]
    assert (s1['epochs'], s1['epoch_boundaries'], s1['fanned_out'], s1['cancelled']) == (1, 0, 1, 0)
    assert (s0['epochs'], s0['epoch_boundaries'], s0['fanned_out']) == (1, 0, 0)
    parts = []
    for k in range(6):
        if k:
            parts.append(torch.zeros(1, gaps[k - 1]))
        parts.append(r0['seg%d' % k]['output_audio'])
        assert len(k0['seg%d' % k]) > 0
    want = torch.cat(parts, dim=-1)
    got = r1['long']
    assert set(got) == set(r0['seg0']) and got['output_audio'].shape == want.shape and torch.equal(got['output_audio'], want)
    assert got['segments_info'] == {'total_segments': 6, 'segments': segs} and got['speaker_id'] == 'spk0' and got['duration'] == want.shape[-1] / c.sample_rate
    assert k1['long'] == [k0['seg%d' % k] for k in range(6)]
    for t in shorts:
        assert k1[t['id']] == k0[t['id']] and torch.equal(r1[t['id']]['output_audio'], r0[t['id']]['output_audio']), t['id']
    # the switch off
    r2, k2, s2 = serve(mixed)
    assert (s2['epochs'], s2['epoch_boundaries'], s2['fanned_out']) == (2, 1, 0)
    for t in shorts:
        assert k2[t['id']] == k0[t['id']] and torch.equal(r2[t['id']]['output_audio'], r0[t['id']]['output_audio']), t['id']
    assert 'long' in r2


def test_serve_stream_cancels_one_utterance(tiny_cfg, pipe):
    """serve(stream=True) over four utterances on three slots; the consumer sets one utterance's flag when its first piece arrives: that utterance comes
    back once as Cancelled (what it handed out before is a prefix of its pieces), the others' pieces are those of the uncancelled run, nothing is
    abandoned and the LM thread is gone.  Unstreamed, an utterance that arrives cancelled comes back as (utterance, Cancelled, [])."""
    from flowmirror_hydravox_amd.llm import Cancelled
    from flowmirror_hydravox_amd.pipeline import synthetic_utterance

    class Src:
        def __init__(self, items):
            self.it = iter(items)

        def poll(self, block):
            return next(self.it)

    def utts():
        us = [synthetic_utterance(tiny_cfg, 300 + i, n) for i, n in enumerate((8, 10, 12, 9))]
        for u in us:
            u.max_token_text_ratio = u.min_token_text_ratio = 15
        return us
    whole = {}
    for u, piece, info in pipe.serve(Src(utts()), lm_slots=3, stream=True):
        assert not isinstance(piece, BaseException), piece
        whole.setdefault(u.seed, []).append(piece)
    assert 'cancelled' not in pipe.last_continuous and all(len(v) >= 4 for v in whole.values())
    us = utts()
    us[2].cancel = threading.Event()
    got, back = {}, []
    for u, piece, info in pipe.serve(Src(us), lm_slots=3, stream=True):
        if isinstance(piece, BaseException):
            back.append((u.seed, piece, info))
            continue
        assert u.seed not in [s for s, _, _ in back]                            # nothing of it after its Cancelled
        got.setdefault(u.seed, []).append(piece)
        if u is us[2]:
            us[2].cancel.set()
    assert len(back) == 1 and back[0][0] == 302 and isinstance(back[0][1], Cancelled) and back[0][2] == {}
    for seed in (300, 301, 303):
        assert len(got[seed]) == len(whole[seed]) and all(torch.equal(a, b) for a, b in zip(got[seed], whole[seed])), seed
    assert 1 <= len(got[302]) < len(whole[302]) and all(torch.equal(a, b) for a, b in zip(got[302], whole[302]))
    lc = pipe.last_continuous
    assert lc['cancelled'] == 1 and lc['abandoned'] == [] and lc['llm']['cancelled'] == 1
    assert not any(t.name == 'hvx-lm' and t.is_alive() for t in threading.enumerate())
    # unstreamed
    us = utts()
    us[1].cancel = threading.Event()
    us[1].cancel.set()
    out = {u.seed: (w, t) for u, w, t in pipe.serve(Src(us), lm_slots=3)}
    assert isinstance(out[301][0], Cancelled) and out[301][1] == [] and pipe.last_continuous['cancelled'] == 1 and pipe.last_continuous['abandoned'] == []
    assert all(out[s][0].numel() == sum(p.numel() for p in whole[s]) for s in (300, 302, 303))
