"""Per-sequence sampling parameters in one launch / one decode grid (sampler.hip: SampleArgs.seq_*, hvx_ras_sample_seq,
hvx_llm_decode_steps_seq, hvx_llm_decode_join_seq; llm.py: _DecodeEngine(mixed_sampling=True); worker.serve_queue(mixed_sampling=True)).

Truth is the reference's own sampler (tests/golden/sampler_many.npz, minted by its sampling_ids) and, for the decode grid, the fp32 oracle
(oracle/llm_ref.py) run once per request with that request's parameters.  Everything here is an exact comparison of integer ids."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden, state_checksum

pytestmark = pytest.mark.gpu
DEV = 'cuda'

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
from mixed_sampling_cases import N_SLOTS, N_TEXT, RATIO, SEEDS, WIN_CAP, WINDOW_SENSITIVE, grid_texts, sp as _sp  # noqa: E402


# ---- 1 / 2: the sampler ---------------------------------------------------------------------------------------------------------------------
def test_sampler_thousand_cases_one_launch_per_vocabulary():
    """All 760 cases of sampler_many.npz at V = 296 in ONE launch and the 240 at V = 6761 in a second, every sequence with its own top_k / top_p /
    win_size / rep_thresh (5 x 5 x 4 x 4 values cycle through the set): ids and noise consumption equal the reference's for every case."""
    from flowmirror_hydravox_amd import ops
    from oracle import sampler_ref
    from sampler_cases import make_case, N_CASES
    g = load_golden('sampler_many.npz')
    cases = [make_case(i) for i in range(N_CASES)]
    by_v = {}
    for i, c in enumerate(cases):
        assert int.from_bytes(hashlib.sha256(c['logp'].tobytes()).digest()[:8], 'little', signed=True) == int(g['logp_sha'][i]), i
        by_v.setdefault((len(c['logp']), c['Vs']), []).append(i)
    assert sorted((v, len(idxs)) for (v, _), idxs in by_v.items()) == [(296, 760), (6761, 240)]
    bad, n_sets = [], 0
    for (V, Vs), idxs in by_v.items():
        S = len(idxs)
        n_sets += len({(cases[i]['top_k'], cases[i]['top_p'], cases[i]['win'], cases[i]['tau']) for i in idxs})
        ncap = (max(int(g['consumed'][i]) for i in idxs) + 2 * V + 1023) // 1024 * 1024
        H = max(1, max(len(cases[i]['hist']) for i in idxs))
        hist = torch.zeros(S, H, dtype=torch.int32)
        for j, i in enumerate(idxs):
            hist[j, :len(cases[i]['hist'])] = torch.tensor(cases[i]['hist'], dtype=torch.int32)
        hist_len = torch.tensor([len(cases[i]['hist']) for i in idxs], dtype=torch.int32)
        ign = torch.tensor([int(cases[i]['ignore_eos']) for i in idxs])
        min_len = torch.where(ign > 0, hist_len + 1, torch.zeros_like(hist_len)).to(torch.int32)
        logp = torch.stack([torch.from_numpy(cases[i]['logp']) for i in idxs]).view(S, 1, V)
        noise = torch.stack([torch.from_numpy(sampler_ref.NoiseStream(seed=cases[i]['seed']).take(ncap).copy()) for i in idxs])
        seq = dict(top_k=torch.tensor([cases[i]['top_k'] for i in idxs], dtype=torch.int32),
                   top_p=torch.tensor([cases[i]['top_p'] for i in idxs], dtype=torch.float32),
                   win_size=torch.tensor([cases[i]['win'] for i in idxs], dtype=torch.int32),
                   rep_thresh=torch.tensor([sampler_ref.rep_threshold(cases[i]['win'], cases[i]['tau']) for i in idxs], dtype=torch.int32))
        cur = torch.zeros(S, dtype=torch.int64).to(DEV)
        ids = ops.ras_sample(logp.to(DEV), hist.to(DEV), hist_len.to(DEV), min_len.to(DEV), noise.to(DEV), cur, speech_tokens=Vs,
                             seq_params=seq).cpu().view(-1).tolist()
        cur = cur.cpu().tolist()
        for j, i in enumerate(idxs):
            want_id, want_c = int(g['id'][i]), int(g['consumed'][i])
            if ids[j] != want_id or (want_id >= 0 and cur[j] != want_c):
                bad.append((i, ids[j], want_id, cur[j], want_c))
    assert n_sets > 100                                                  # (the launches really mixed parameter sets)
    assert not bad, (len(bad), bad[:10])


def test_seq_entry_with_null_block_is_hvx_ras_sample():
    """hvx_ras_sample_seq(args, NULL) returns the ids and cursors of hvx_ras_sample on sampler_small.npz, group by group"""
    from flowmirror_hydravox_amd import ops
    from oracle import sampler_ref
    g = load_golden('sampler_small.npz')
    n, V, ncap = len(g['id']), g['logp'].shape[1], 1 << 16
    keys = {}
    for i in range(n):
        keys.setdefault((int(g['top_k'][i]), float(g['top_p'][i]), int(g['win'][i]), float(g['tau'][i])), []).append(i)
    need = int(g['consumed'].max()) + 2 * V
    assert need <= ncap
    for (top_k, top_p, win, tau), idxs in keys.items():
        S = len(idxs)
        logp = torch.from_numpy(g['logp'][idxs]).view(S, 1, V).to(DEV)
        hist = torch.from_numpy(np.maximum(g['hist'][idxs], 0).astype(np.int32)).to(DEV)
        hl = torch.from_numpy(g['hist_len'][idxs].astype(np.int32))
        min_len = torch.where(torch.from_numpy(g['ignore_eos'][idxs]) > 0, hl + 1, torch.zeros_like(hl)).to(torch.int32).to(DEV)
        noise = torch.stack([torch.from_numpy(sampler_ref.NoiseStream(seed=int(g['seed'][i])).take(ncap).copy()) for i in idxs]).to(DEV)
        kw = dict(speech_tokens=int(g['Vs'][idxs[0]]), top_k=top_k, top_p=top_p, win_size=win, rep_thresh=sampler_ref.rep_threshold(win, tau))
        c0, c1 = torch.zeros(S, dtype=torch.int64, device=DEV), torch.zeros(S, dtype=torch.int64, device=DEV)
        a = ops.ras_sample(logp, hist, hl.to(DEV), min_len, noise, c0, **kw)
        b = ops.ras_sample(logp, hist, hl.to(DEV), min_len, noise, c1, seq_entry=True, **kw)
        assert torch.equal(a, b) and torch.equal(c0, c1), (top_k, top_p, win, tau)
        assert a.cpu().view(-1).tolist() == [int(g['id'][i]) for i in idxs]
    # the host refuses what the kernel could only clamp
    with pytest.raises(ValueError):
        ops.ras_sample(logp, hist, hl.to(DEV), min_len, noise, c0, speech_tokens=1,
                       seq_params=dict(top_k=torch.full((S,), 65), top_p=torch.ones(S), win_size=torch.ones(S), rep_thresh=torch.ones(S)))
    with pytest.raises(ValueError):
        ops.ras_sample(logp, hist, hl.to(DEV), min_len, noise, c0, speech_tokens=1, seq_params=dict(top_k=torch.ones(S), top_p=torch.ones(S)))


# ---- 3 / 4: the decode grid -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def cfg():
    from flowmirror_hydravox_amd.config import cv3w_config
    return cv3w_config()


@pytest.fixture(scope='module')
def llm_state(cfg):
    from flowmirror_hydravox_amd import weights as W
    g = load_golden('llm_cv3w.npz')
    sd = W.make_llm_state(cfg.llm, seed=int(g['weight_seed']), init='fan_in', with_lm_head=True)
    assert state_checksum(sd) == str(g['weight_sha'])
    return sd


@pytest.fixture(scope='module')
def oracle_ids():
    """the oracle's ids of every request with its own parameters (tests/golden/mixed_sampling_grid.npz: minted by oracle/llm_ref.py, recomputed on the
    CPU by tests/test_mixed_sampling_host.py) — loaded once, shared, never modified"""
    g = load_golden('mixed_sampling_grid.npz')
    return tuple(tuple(int(t) for t in g['own_%d' % i]) for i in range(len(N_TEXT)))


def _make_llm(cfg, sd, sampling, max_batch):
    from functools import partial
    from flowmirror_hydravox_amd.llm import HvxLLM
    from flowmirror_hydravox_amd.sampling import ras_sampling
    llm = HvxLLM(cfg.llm, sd, dtype=torch.float32, max_batch=max_batch, max_ctx=512, sampling=partial(ras_sampling, **sampling))
    llm.inference_head_num = 2
    return llm


def _req(cfg, i, **kw):
    return dict(dict(text=grid_texts(cfg.llm)[i], seed=SEEDS[i], tag=i, max_token_text_ratio=RATIO, min_token_text_ratio=RATIO), **kw)


def test_decode_grid_four_parameter_sets_and_slot_reuse(cfg, llm_state, oracle_ids):
    """8 requests with four parameter sets through a 5-slot mixed grid (win_cap 32): every id list == the oracle's for that request with its own
    parameters == what the scalar engine gives when it serves the request alone with the parameters on llm.sampling.  Every ring wraps at
    least three times and three slots are taken over by a request with another parameter set.  The window must matter for the comparison to
    show anything: for at least two requests the oracle's stream under window 32 differs from its stream under the request's own window."""
    n = len(N_TEXT)
    g = load_golden('mixed_sampling_grid.npz')
    for i in range(n):
        assert len(oracle_ids[i]) == N_TEXT[i] * RATIO >= 100 >= 3 * WIN_CAP
    differ = [i for i in WINDOW_SENSITIVE if tuple(int(t) for t in g['w32_%d' % i]) != oracle_ids[i]]
    assert len(differ) >= 2, differ
    llm = _make_llm(cfg, llm_state, _sp(0), N_SLOTS)
    got = dict(llm.generate_stream(iter([_req(cfg, i, sampling=_sp(i)) for i in range(n)]), n_slots=N_SLOTS, mixed_sampling=True, win_cap=WIN_CAP))
    st = llm.last_stats
    assert st['requests'] == n and st['mixed_sampling'] and st['clean']
    owner, reused = {}, []
    for tag, slot in st['joins']:
        if slot in owner and owner[slot] % 4 != tag % 4:
            reused.append((slot, owner[slot], tag))
        owner[slot] = tag
    assert len(st['joins']) == n and len(reused) >= 3, st['joins']
    for i in range(n):
        assert got[i] == list(oracle_ids[i]), (i, 'mixed grid vs oracle', [k for k, (x, y) in enumerate(zip(got[i], oracle_ids[i])) if x != y][:3])
    # today's engine, one request at a time, its parameters on llm.sampling
    from functools import partial
    from flowmirror_hydravox_amd.sampling import ras_sampling
    for i in range(n):
        llm.sampling = partial(ras_sampling, **_sp(i))
        alone = dict(llm.generate_stream(iter([_req(cfg, i)]), n_slots=1))
        assert alone[i] == got[i], (i, 'scalar engine alone')
        assert not llm.last_stats['mixed_sampling']


def test_refusals_leave_the_grid_running(cfg, llm_state, oracle_ids):
    """win_size 0 and win_size = win_cap + 1 come back with `error` set while the others finish with the oracle's ids; hvx_llm_decode_join_seq
    with top_k = 65 returns non-zero with a message, launches nothing, and the neighbours' ids are what they are without it."""
    import ctypes as C
    from flowmirror_hydravox_amd.llm import _DecodeEngine, _Request
    from flowmirror_hydravox_amd.sampling import NoiseStream
    llm = _make_llm(cfg, llm_state, _sp(0), 3)
    reqs = [_req(cfg, 0, sampling=_sp(0)), _req(cfg, 1, sampling=_sp(1, win_size=0), tag='zero'), _req(cfg, 4, sampling=_sp(0)),
            _req(cfg, 2, sampling=_sp(2, win_size=WIN_CAP + 1), tag='long'), _req(cfg, 5, sampling=_sp(5)), _req(cfg, 6, sampling=dict(top_k=65), tag='k65')]
    got = dict(llm.generate_stream(iter(reqs), n_slots=3, mixed_sampling=True, win_cap=WIN_CAP))
    assert isinstance(got['zero'], ValueError) and 'win_size=0' in str(got['zero'])
    assert isinstance(got['long'], ValueError) and 'win_cap=%d' % WIN_CAP in str(got['long'])
    assert isinstance(got['k65'], ValueError) and 'top_k' in str(got['k65'])
    for i in (0, 4, 5):
        assert got[i] == list(oracle_ids[i]), i
    # a request that carries parameters to a grid without the switch is refused too, not served with the model's
    plain = dict(llm.generate_stream(iter([_req(cfg, 0, sampling=_sp(1))]), n_slots=1))
    assert isinstance(plain[0], ValueError) and 'mixed_sampling' in str(plain[0])

    # the C entry point: requests 0 and 4 decode in slots 0 and 2 of a 3-slot grid; between two blocks a join of slot 1 with top_k = 65 is refused
    def run(with_bad_join):
        eng = _DecodeEngine(llm, n_slots=3, max_out=128, max_prefix=64, mixed_sampling=True, win_cap=WIN_CAP)
        rs = []
        for i, slot in ((0, 0), (4, 2)):
            text = grid_texts(cfg.llm)[i]
            r = _Request(llm._encode_prefix(text, None, None), len(text), N_TEXT[i] * RATIO, N_TEXT[i] * RATIO, NoiseStream(seed=SEEDS[i], chunk=8192))
            r.set_sampling(_sp(i))
            rs.append((slot, r))
        with torch.cuda.stream(eng.stream):
            for slot, r in rs:
                eng._join(slot, r, 0)
            eng._publish_limits()
            s = C.c_void_p(eng.stream.cuda_stream)
            for blk in range(14):                                         # 14 x 8 steps x 2 heads >= 100 tokens
                if with_bad_join and blk == 3:
                    before = eng.ctl_dev.clone(), eng.seq_top_k.clone(), eng.seq_win.clone(), eng.cur_dev.clone()
                    rc = llm.lib.hvx_llm_decode_join_seq(llm._h, s, C.byref(eng.args), C.byref(eng.seq), 1, 7, 0, 4, 8, 65, 0.8, 10, 1)
                    assert rc != 0 and b'top_k=65' in llm.lib.hvx_last_error()
                    after = eng.ctl_dev.clone(), eng.seq_top_k.clone(), eng.seq_win.clone(), eng.cur_dev.clone()
                    assert all(torch.equal(x, y) for x, y in zip(before, after))          # the slot's state is untouched
                    for bad in ((25, 0.0, 10, 1), (25, 0.8, 0, 1), (25, 0.8, WIN_CAP + 1, 1), (25, 0.8, 10, -1)):
                        assert llm.lib.hvx_llm_decode_join_seq(llm._h, s, C.byref(eng.args), C.byref(eng.seq), 1, 7, 0, 4, 8, *bad) != 0, bad
                _lib_check(llm.lib.hvx_llm_decode_steps_seq(llm._h, s, C.byref(eng.args), C.byref(eng.seq), 8))
            eng.stream.synchronize()
            state = eng.ctl_dev[eng.o_state:eng.o_state + 24].view(3, 8).cpu()
            out = [eng.out_dev[slot, :int(state[slot, 1])].cpu().tolist() for slot, _ in rs]
        for _, r in rs:
            r.noise.finalize(0)
        assert int(state[1, 1]) == 0 and int(state[1, 2]) == 1            # slot 1 never ran
        return out
    clean, disturbed = run(False), run(True)
    assert clean == disturbed == [list(oracle_ids[0]), list(oracle_ids[4])]


def _lib_check(rc):
    from flowmirror_hydravox_amd import _lib
    _lib.check(rc, 'hvx_llm_decode_steps_seq')


# ---- 5: the queue worker ----------------------------------------------------------------------------------------------------------------------
def test_queue_worker_mixed_sampling_keeps_alternating_requests_on_one_grid(tiny_cfg, tmp_path):
    """Twelve seeded tasks that alternate between two parameter sets, and one more in the middle with another inference_head_num, through
    worker.serve_queue on the tiny models: with mixed_sampling the token ids and the waveforms per task id are those of the default worker
    (bit for bit: the bound test_queue_worker_serves_the_continuous_engine uses between its two serving paths), and the run closes two running
    epochs — before and after the odd head count — where the default closes one at every task, twelve."""
    import argparse
    import dataclasses
    import json
    import queue
    from flowmirror_hydravox_amd import weights as W
    from flowmirror_hydravox_amd.model_manager import HvxModelManager
    from flowmirror_hydravox_amd.worker import serve_queue
    from test_host_cpu import _QueueFrontend
    c = tiny_cfg
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
    r1, k1, s1 = serve(mixed_sampling=True)
    ids = {t['id'] for t in tasks}
    assert set(r0) == set(r1) == set(k0) == set(k1) == ids and not any('error' in r for r in list(r0.values()) + list(r1.values()))
    for i in sorted(ids):
        assert len(k0[i]) > 0 and k0[i] == k1[i], i
        assert r0[i]['output_audio'].shape == r1[i]['output_audio'].shape and torch.equal(r0[i]['output_audio'], r1[i]['output_audio']), i
    assert len({tuple(k0['t0']), tuple(k0['t1'])}) == 2
    assert (s0['epoch_boundaries'], s0['epochs']) == (12, 13)
    assert (s1['epoch_boundaries'], s1['epochs']) == (2, 3)
