"""Per-sequence head counts in one launch / one decode grid (sampler.hip: SampleArgs.seq_heads, hvx_ras_sample_mixed, hvx_llm_decode_steps_mixed,
hvx_llm_decode_join_mixed; hvx_llm.hip: heads_live; llm.py: _DecodeEngine(mixed_heads=True); worker.serve_queue(mixed_heads=True)).

Truth is the CPU oracle: oracle/sampler_ref.py head by head for the sampler, and oracle/llm_ref.py run once per request with that request's head
count and parameters for the decode grid (tests/golden/mixed_heads_grid.npz).  Everything here is an exact comparison of integer ids; the LM
runs in fp32 wherever ids are compared across grid shapes."""
import os
import sys
from functools import partial

import pytest
import torch

from conftest import load_golden, state_checksum

pytestmark = pytest.mark.gpu
DEV = 'cuda'

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
from mixed_heads_cases import HEAD_CAP, HEADS, N_SLOTS, N_TEXT, RATIO, SEEDS, WIN_CAP, grid_texts, sp as _sp  # noqa: E402


# ---- 1: the sampler ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('big', [False, True], ids=['V296', 'V6761'])
def test_sampler_per_sequence_head_counts_one_launch(big):
    """64 sequences x 5 head rows in ONE launch, k_s cycling 1..5, rows j >= k_s filled with NaN: ids for j < k_s and the cursors equal
    oracle/sampler_ref run head by head over the shared history snapshot, entries j >= k_s are -3.  Every sequence also has its own sampling
    parameters (those of its first row's case).  The rows are the cases of sampler_cases.make_case in order, without the i % 15 == 2 ones (stop
    ids pushed until max_trials is exhausted: 100 full-vocabulary races per head, covered by the single-head thousand-case test) — cycled
    where the vocabulary has fewer than 320 cases.  A second call with a NULL heads block equals hvx_ras_sample_seq on the same (NaN-free) inputs."""
    from flowmirror_hydravox_amd import ops
    from oracle import sampler_ref
    from sampler_cases import make_case, N_BIG, N_SMALL
    S, K = 64, 5
    pool = [i for i in (range(N_SMALL, N_SMALL + N_BIG) if big else range(N_SMALL)) if i % 15 != 2]
    rows = [[make_case(pool[(s * K + j) % len(pool)]) for j in range(K)] for s in range(S)]
    V, Vs = len(rows[0][0]['logp']), rows[0][0]['Vs']
    assert V == (6761 if big else 296)
    heads = [1 + s % K for s in range(S)]
    want_ids, want_cur = [], []
    for s in range(S):
        c = rows[s][0]
        noise = sampler_ref.NoiseStream(seed=c['seed'])
        min_len = len(c['hist']) + 1 if c['ignore_eos'] else 0
        ids = []
        for j in range(heads[s]):                                            # head by head, every head against the same snapshot
            try:
                ids.append(sampler_ref.sampling_ids(rows[s][j]['logp'], list(c['hist']), noise, Vs, (len(c['hist']) + j) < min_len, top_p=c['top_p'],
                                                    top_k=c['top_k'], win_size=c['win'], tau_r=c['tau']))
            except RuntimeError:
                ids.append(-1)
        want_ids.append(ids + [-3] * (K - heads[s]))
        want_cur.append(noise.cursor)
    ncap = (max(want_cur) + 2 * V + 1023) // 1024 * 1024
    H = max(1, max(len(rows[s][0]['hist']) for s in range(S)))
    hist = torch.zeros(S, H, dtype=torch.int32)
    for s in range(S):
        hist[s, :len(rows[s][0]['hist'])] = torch.tensor(rows[s][0]['hist'], dtype=torch.int32)
    hist_len = torch.tensor([len(rows[s][0]['hist']) for s in range(S)], dtype=torch.int32)
    ign = torch.tensor([int(rows[s][0]['ignore_eos']) for s in range(S)])
    min_len = torch.where(ign > 0, hist_len + 1, torch.zeros_like(hist_len)).to(torch.int32)
    clean = torch.stack([torch.stack([torch.from_numpy(rows[s][j]['logp']) for j in range(K)]) for s in range(S)])
    logp = clean.clone()
    for s in range(S):
        logp[s, heads[s]:] = float('nan')
    noise = torch.stack([torch.from_numpy(sampler_ref.NoiseStream(seed=rows[s][0]['seed']).take(ncap).copy()) for s in range(S)]).to(DEV)
    seq = dict(top_k=torch.tensor([rows[s][0]['top_k'] for s in range(S)], dtype=torch.int32),
               top_p=torch.tensor([rows[s][0]['top_p'] for s in range(S)], dtype=torch.float32),
               win_size=torch.tensor([rows[s][0]['win'] for s in range(S)], dtype=torch.int32),
               rep_thresh=torch.tensor([sampler_ref.rep_threshold(rows[s][0]['win'], rows[s][0]['tau']) for s in range(S)], dtype=torch.int32))
    args = (hist.to(DEV), hist_len.to(DEV), min_len.to(DEV), noise)
    cur = torch.zeros(S, dtype=torch.int64, device=DEV)
    ids = ops.ras_sample(logp.to(DEV), *args, cur, speech_tokens=Vs, seq_params=seq, seq_heads=torch.tensor(heads)).cpu().tolist()
    cur = cur.cpu().tolist()
    bad = [(s, heads[s], ids[s], want_ids[s], cur[s], want_cur[s]) for s in range(S) if ids[s] != want_ids[s] or cur[s] != want_cur[s]]
    assert not bad, (len(bad), bad[:5])
    assert sum(1 for s in range(S) if -1 in want_ids[s]) < S // 2          # (the comparison is about ids, not about exhausted trials)
    # NULL heads block == hvx_ras_sample_seq, ids and cursors
    c0, c1 = torch.zeros(S, dtype=torch.int64, device=DEV), torch.zeros(S, dtype=torch.int64, device=DEV)
    a = ops.ras_sample(clean.to(DEV), *args, c0, speech_tokens=Vs, seq_params=seq)
    b = ops.ras_sample(clean.to(DEV), *args, c1, speech_tokens=Vs, seq_params=seq, mixed_entry=True)
    assert torch.equal(a, b) and torch.equal(c0, c1) and int(a.min()) >= -1
    # up to its own head count a sequence draws what it draws with all five heads
    a = a.cpu().tolist()
    assert all(a[s][:heads[s]] == ids[s][:heads[s]] for s in range(S))
    with pytest.raises(ValueError):
        ops.ras_sample(clean.to(DEV), *args, c0, speech_tokens=Vs, seq_params=seq, seq_heads=torch.ones(S - 1))


# ---- 2 / 3 / 4: the decode grid ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def cfg():
    from flowmirror_hydravox_amd.config import cv3w_config
    return cv3w_config()


@pytest.fixture(scope='module')
def oracle_ids():
    """the oracle's ids of every request with its own head count and parameters (tests/golden/mixed_heads_grid.npz: minted by oracle/llm_ref.py,
    recomputed on the CPU by tests/test_mixed_heads_host.py) — loaded once, shared, never modified"""
    g = load_golden('mixed_heads_grid.npz')
    return tuple(tuple(int(t) for t in g['own_%d' % i]) for i in range(len(N_TEXT)))


@pytest.fixture(scope='module')
def llm(cfg):
    """one fp32 LM for the grid tests; every test sets `sampling` / `inference_head_num` before it decodes"""
    from flowmirror_hydravox_amd import weights as W
    from flowmirror_hydravox_amd.llm import HvxLLM
    g = load_golden('llm_cv3w.npz')
    sd = W.make_llm_state(cfg.llm, seed=int(g['weight_seed']), init='fan_in', with_lm_head=True)
    assert state_checksum(sd) == str(g['weight_sha'])
    return HvxLLM(cfg.llm, sd, dtype=torch.float32, max_batch=N_SLOTS, max_ctx=512)


def _defaults(llm, heads=HEAD_CAP, i=0):
    from flowmirror_hydravox_amd.sampling import ras_sampling
    llm.sampling = partial(ras_sampling, **_sp(i))
    llm.inference_head_num = heads


def _req(cfg, i, **kw):
    return dict(dict(text=grid_texts(cfg.llm)[i], seed=SEEDS[i], tag=i, max_token_text_ratio=RATIO, min_token_text_ratio=RATIO), **kw)


def _own(cfg, i, **kw):
    """request i as the fixture has it: its head count, and (odd requests) the second parameter set"""
    return _req(cfg, i, **dict(dict({'sampling': _sp(i)} if i % 2 else {}, inference_head_num=HEADS[i]), **kw))


def test_decode_grid_mixed_head_counts_and_slot_reuse(cfg, llm, oracle_ids):
    """The 8 requests (1, 2, 3, 5, 2, 5, 1, 4 heads, half of them with a second parameter set) through a 4-slot grid of 5 rows per sequence:
    every id list == the oracle's for that request == what the scalar engine gives serving the request alone with its head count on
    llm.inference_head_num and its parameters on llm.sampling; slots are taken over by requests with more and with fewer heads."""
    n = len(N_TEXT)
    _defaults(llm)
    got = dict(llm.generate_stream(iter([_own(cfg, i) for i in range(n)]), n_slots=N_SLOTS, mixed_heads=True, head_cap=HEAD_CAP, mixed_sampling=True,
                                   win_cap=WIN_CAP))
    st = llm.last_stats
    assert st['requests'] == n and st['mixed_heads'] and st['mixed_sampling'] and st['clean']
    assert st['head_cap'] == HEAD_CAP and st['rows'] == N_SLOTS * HEAD_CAP and st['head_k'] == HEAD_CAP
    assert sum(st['head_steps'].values()) == st['steps'] and set(st['head_steps']) <= set(range(1, HEAD_CAP + 1)) and HEAD_CAP in st['head_steps']
    owner, larger, smaller = {}, [], []
    for tag, slot in st['joins']:
        if slot in owner:
            (larger if HEADS[tag] > HEADS[owner[slot]] else smaller if HEADS[tag] < HEADS[owner[slot]] else []).append((slot, owner[slot], tag))
        owner[slot] = tag
    assert len(st['joins']) == n and larger and smaller, st['joins']
    for i in range(n):
        assert len(oracle_ids[i]) == N_TEXT[i] * RATIO >= 60
        assert got[i] == list(oracle_ids[i]), (i, 'mixed grid vs oracle', [k for k, (x, y) in enumerate(zip(got[i], oracle_ids[i])) if x != y][:3])
    # the scalar engine, one request at a time
    for i in range(n):
        _defaults(llm, HEADS[i], i)
        alone = dict(llm.generate_stream(iter([_req(cfg, i)]), n_slots=1))
        assert alone[i] == got[i], (i, 'scalar engine alone')
        assert not llm.last_stats['mixed_heads'] and llm.last_stats['head_k'] == HEADS[i]


def test_heads_live_follows_the_widest_request_in_flight(cfg, llm, oracle_ids):
    """Four requests at 2 heads under head_cap 5: every step is enqueued with heads_live = 2 and the ids are those of a head_cap = 2 grid (and
    request 4's, which the fixture has at 2 heads, the oracle's).  With a 5-head request in the middle of a 2-slot grid the steps run at 2, then
    5, then 2 again, and the ids still match the oracle."""
    _defaults(llm)
    reqs = [_req(cfg, i, inference_head_num=2) for i in (0, 1, 2, 4)]
    wide = dict(llm.generate_stream(iter(reqs), n_slots=4, mixed_heads=True, head_cap=HEAD_CAP))
    st = llm.last_stats
    assert list(st['head_steps']) == [2] and st['head_steps'][2] == st['steps'] and st['rows'] == 20 and not st['mixed_sampling']
    narrow = dict(llm.generate_stream(iter(reqs), n_slots=4, mixed_heads=True, head_cap=2))
    assert list(llm.last_stats['head_steps']) == [2] and llm.last_stats['rows'] == 8
    assert wide == narrow and wide[4] == list(oracle_ids[4])
    for i in (0, 1, 2, 4):
        assert len(wide[i]) == N_TEXT[i] * RATIO
    # requests 1 and 4 (2 heads) open the grid, request 3 (5 heads) follows, then 4 and 1 once more
    reqs = [_own(cfg, 1), _own(cfg, 4), _own(cfg, 3), _own(cfg, 4, tag='4b'), _own(cfg, 1, tag='1b')]
    got = dict(llm.generate_stream(iter(reqs), n_slots=2, mixed_heads=True, head_cap=HEAD_CAP, mixed_sampling=True, win_cap=WIN_CAP))
    st = llm.last_stats
    assert set(st['head_steps']) == {2, 5}
    assert [k for k, _ in st['head_runs']] == [2, 5, 2], st['head_runs']
    assert sum(n for _, n in st['head_runs']) == st['steps']
    for tag, i in ((1, 1), (4, 4), (3, 3), ('4b', 4), ('1b', 1)):
        assert got[tag] == list(oracle_ids[i]), tag


def test_refusals_leave_the_grid_running(cfg, llm, oracle_ids):
    """6 heads under head_cap 4 come back as a ValueError naming head_cap while the neighbours finish with the oracle's ids; a request carrying
    inference_head_num to a grid without the switch is refused; hvx_llm_decode_join_mixed with head count 0 and head_k + 1 returns non-zero with a
    message, launches nothing, and the neighbours' ids are what they are without it."""
    import ctypes as C
    from flowmirror_hydravox_amd import _lib
    from flowmirror_hydravox_amd.llm import _DecodeEngine, _Request
    from flowmirror_hydravox_amd.sampling import NoiseStream
    _defaults(llm, 2)
    reqs = [_own(cfg, 0), _own(cfg, 2, inference_head_num=6, tag='six'), _own(cfg, 1), _own(cfg, 7)]
    got = dict(llm.generate_stream(iter(reqs), n_slots=2, mixed_heads=True, head_cap=4, mixed_sampling=True, win_cap=WIN_CAP))
    assert isinstance(got['six'], ValueError) and 'head_cap=4' in str(got['six'])
    assert llm.last_stats['head_cap'] == 4 and llm.last_stats['rows'] == 8
    for i in (0, 1, 7):
        assert got[i] == list(oracle_ids[i]), i
    plain = dict(llm.generate_stream(iter([_req(cfg, 4, inference_head_num=2)]), n_slots=1))
    assert isinstance(plain[4], ValueError) and 'mixed_heads' in str(plain[4])
    with pytest.raises(ValueError):
        _DecodeEngine(llm, n_slots=1, max_out=8, max_prefix=8, head_cap=3)
    with pytest.raises(ValueError):
        _DecodeEngine(llm, n_slots=1, max_out=8, max_prefix=8, mixed_heads=True, head_cap=HEAD_CAP + 1)

    # the C entry point: requests 1 and 4 (2 heads each) decode in slots 0 and 2 of a 3-slot grid; between two blocks joins of slot 1 are refused
    def run(with_bad_join):
        eng = _DecodeEngine(llm, n_slots=3, max_out=128, max_prefix=64, mixed_sampling=True, win_cap=WIN_CAP, mixed_heads=True, head_cap=HEAD_CAP)
        rs = []
        for i, slot in ((1, 0), (4, 2)):
            text = grid_texts(cfg.llm)[i]
            r = _Request(llm._encode_prefix(text, None, None), len(text), N_TEXT[i] * RATIO, N_TEXT[i] * RATIO, NoiseStream(seed=SEEDS[i], chunk=8192))
            r.set_sampling(_sp(i))
            r.heads = HEADS[i]
            rs.append((slot, r))
        with torch.cuda.stream(eng.stream):
            for slot, r in rs:
                eng._join(slot, r, 0)
            eng._publish_limits()
            s = C.c_void_p(eng.stream.cuda_stream)
            assert eng.seq_heads.cpu().tolist() == [2, 5, 2]                  # (slot 1 was never joined: the LM's count)
            for blk in range(5):                                              # 5 x 8 steps x 2 heads >= 64 tokens
                if with_bad_join and blk == 2:
                    before = eng.ctl_dev.clone(), eng.seq_heads.clone(), eng.seq_top_k.clone(), eng.cur_dev.clone()
                    for k in (0, HEAD_CAP + 1):
                        rc = llm.lib.hvx_llm_decode_join_mixed(llm._h, s, C.byref(eng.args), C.byref(eng.seq), C.byref(eng.hd), 1, 7, 0, 4, 8, 25, 0.8, 10, 1, k)
                        assert rc != 0 and b'head count %d outside' % k in llm.lib.hvx_last_error()
                    after = eng.ctl_dev.clone(), eng.seq_heads.clone(), eng.seq_top_k.clone(), eng.cur_dev.clone()
                    assert all(torch.equal(x, y) for x, y in zip(before, after))          # nothing was launched: the slot's state is untouched
                    # heads_live outside [1, head_k], or below head_k without a heads block, is refused as well
                    assert llm.lib.hvx_llm_decode_steps_mixed(llm._h, s, C.byref(eng.args), C.byref(eng.seq), C.byref(eng.hd), HEAD_CAP + 1, 8) != 0
                    assert llm.lib.hvx_llm_decode_steps_mixed(llm._h, s, C.byref(eng.args), C.byref(eng.seq), C.byref(eng.hd), 0, 8) != 0
                    assert llm.lib.hvx_llm_decode_steps_mixed(llm._h, s, C.byref(eng.args), C.byref(eng.seq), None, 2, 8) != 0
                _lib.check(llm.lib.hvx_llm_decode_steps_mixed(llm._h, s, C.byref(eng.args), C.byref(eng.seq), C.byref(eng.hd), 2, 8), 'hvx_llm_decode_steps_mixed')
            eng.stream.synchronize()
            state = eng.ctl_dev[eng.o_state:eng.o_state + 24].view(3, 8).cpu()
            out = [eng.out_dev[slot, :int(state[slot, 1])].cpu().tolist() for slot, _ in rs]
        for _, r in rs:
            r.noise.finalize(0)
        assert int(state[1, 1]) == 0 and int(state[1, 2]) == 1                # slot 1 never ran
        return out
    _defaults(llm)
    clean, disturbed = run(False), run(True)
    assert clean == disturbed == [list(oracle_ids[1]), list(oracle_ids[4])]


# ---- 5: the queue worker ------------------------------------------------------------------------------------------------------------------------
def test_queue_worker_mixed_heads_keeps_another_head_count_on_the_grid(tiny_cfg, tmp_path):
    """The task list of the mixed-sampling worker test — twelve seeded tasks alternating between two parameter sets at 2 heads, and one in the middle
    with 3 heads — through worker.serve_queue on the tiny models (head_num 3): with mixed_sampling and mixed_heads the token ids and the
    waveforms per task id are those of the default worker bit for bit, and the whole queue is ONE epoch with no boundary (mixed_sampling alone:
    two boundaries, three epochs)."""
    import argparse
    import dataclasses
    import json
    import queue
    from flowmirror_hydravox_amd import weights as W
    from flowmirror_hydravox_amd.model_manager import HvxModelManager
    from flowmirror_hydravox_amd.worker import serve_queue
    from test_host_cpu import _QueueFrontend
    c = tiny_cfg
    assert c.llm.head_num == 3
    d = tmp_path / 'model'
    d.mkdir()
    torch.save(W.make_llm_state(c.llm, seed=5, init='fan_in'), d / 'llm.pt')
    torch.save(W.make_flow_state(c.flow, seed=6, init='fan_in'), d / 'flow.pt')
    torch.save(W.make_hift_state(c.hift, seed=7, init='fan_in'), d / 'hift.pt')
    (d / 'hvx_config.json').write_text(json.dumps({'llm': dataclasses.asdict(c.llm), 'flow': dataclasses.asdict(c.flow), 'hift': dataclasses.asdict(c.hift)}))

    class FE(_QueueFrontend):
        def _ids(self, text):
            return torch.tensor([[(ord(ch) * 7) % c.llm.text_vocab for ch in text]], dtype=torch.int32)

        def frontend_sft(self, text, spk_id):
            g = torch.Generator().manual_seed(len(spk_id))
            return dict(text=self._ids(text), text_len=torch.tensor([len(text)], dtype=torch.int32), llm_embedding=torch.zeros(0, 192),
                        flow_embedding=torch.randn(192, generator=g))
    sets = [dict(top_p=0.8, top_k=25, win_size=10, tau_r=0.1, inference_head_num=2), dict(top_p=0.95, top_k=4, win_size=6, tau_r=0.3, inference_head_num=2)]
    texts = ['hello world', 'a b', 'speech synthesis', 'one grid', 'the quick brown fox', 'xyz', 'jumps over', 'lazy dogs', 'nine', 'ten ten', 'eleven!', 'tail']
    tasks = [dict(id='t%d' % i, task_type='tts', text=t, speaker_id='spk%d' % (i % 2), extra_params=dict(sets[i % 2]), seed=300 + i) for i, t in enumerate(texts)]
    tasks.insert(6, dict(id='odd', task_type='tts', text='three heads', speaker_id='spk0', extra_params=dict(sets[0], inference_head_num=3), seed=299))

    def serve(**kw):
        mm = HvxModelManager(frontend_factory=lambda args, cfg: FE())
        mm.load_models(argparse.Namespace(config=None, model_dir=str(d), bf16=True, fp16=False, cpu=False))
        q, results, toks = queue.Queue(), {}, {}
        for t in tasks:
            q.put(dict(t))
        q.put(None)
        stats = serve_queue(mm, q, results, worker_id=0, lm_slots=3, acoustic_batch=2, normalise=lambda s: s, token_log=toks, **kw)
        return results, toks, stats
    r0, k0, s0 = serve()
    r1, k1, s1 = serve(mixed_sampling=True, mixed_heads=True)
    ids = {t['id'] for t in tasks}
    assert set(r0) == set(r1) == set(k0) == set(k1) == ids and not any('error' in r for r in list(r0.values()) + list(r1.values()))
    for i in sorted(ids):
        assert len(k0[i]) > 0 and k0[i] == k1[i], i
        assert r0[i]['output_audio'].shape == r1[i]['output_audio'].shape and torch.equal(r0[i]['output_audio'], r1[i]['output_audio']), i
    assert (s0['epoch_boundaries'], s0['epochs']) == (12, 13)
    assert (s1['epoch_boundaries'], s1['epochs']) == (0, 1) and s1['mixed_heads']
