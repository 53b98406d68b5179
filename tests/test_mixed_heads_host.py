"""Host side of per-sequence head counts (no GPU): the oracle fixture of the decode-grid job, the queue worker's epoch rule with and without
`mixed_heads`, the effective-head rule, and the additive C ABI — hvx_seq_heads and the three `_mixed` entry points — in the header, the
library and the ctypes binding."""
import ctypes
import os
import queue
import re
import subprocess
import sys
import types

import numpy as np
import pytest

from test_host_cpu import _QueueFrontend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EP = dict(top_p=0.8, top_k=25, win_size=10, tau_r=0.1, inference_head_num=2)


def _mm(head_num=None):
    mm = types.SimpleNamespace(frontend=_QueueFrontend(), configs={'sample_rate': 24000}, is_loaded=True, get_available_speakers=lambda: ['s', 'tt'])
    if head_num is not None:
        mm.models = {'llm': types.SimpleNamespace(head_num=head_num, inference_head_num=2)}
    return mm


def _tts(i, **ep):
    return dict(id=i, task_type='tts', text='ab' + 'c' * i, speaker_id='s', extra_params=dict(EP, **ep))


def _drain(src):
    got = []
    while True:
        try:
            u = src.poll(False)
        except StopIteration:
            return got
        assert u is not None
        got.append(u)


def test_decode_grid_fixture_is_the_oracle_and_the_head_count_matters():
    """tests/golden/mixed_heads_grid.npz (what the GPU grid tests compare with) == oracle/llm_ref.py run now, request by request with its own head
    count and parameters; and for every request with fewer than 5 heads the stream at 5 heads — the grid's capacity — is another one."""
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    import mixed_heads_cases as M
    from conftest import load_golden, state_checksum
    from flowmirror_hydravox_amd import weights as W
    from flowmirror_hydravox_amd.config import cv3w_config
    g, fx = load_golden('llm_cv3w.npz'), load_golden('mixed_heads_grid.npz')
    cfg = cv3w_config().llm
    assert cfg.head_num == M.HEAD_CAP == 5 and M.HEADS == [1, 2, 3, 5, 2, 5, 1, 4] and len(M.N_TEXT) == 8
    sd = W.make_llm_state(cfg, seed=int(g['weight_seed']), init='fan_in', with_lm_head=True)
    assert state_checksum(sd) == str(g['weight_sha'])
    now = M.oracle_fixture(sd, cfg)
    assert sorted(now) == sorted(fx.files)
    for k in now:
        assert np.array_equal(now[k], fx[k]), k
    assert sum(1 for i in range(8) if M.sp(i) != M.sp(0)) == 4             # half of the requests carry the second parameter set
    for i, k in enumerate(M.HEADS):
        own, cap = fx['own_%d' % i], fx['cap_%d' % i]
        assert len(own) == len(cap) == M.N_TEXT[i] * M.RATIO >= 60, i
        assert np.array_equal(own, cap) == (k == M.HEAD_CAP), (i, k)


def test_mixed_heads_task_source_keeps_other_head_counts_in_the_epoch():
    """_TaskSource(mixed_heads=True): another inference_head_num in [1, head_cap] joins the running epoch and the utterance carries it; one above
    head_cap is carried to the next epoch, never overtaken; with mixed_sampling off a change of top_k still closes the epoch, with it on both
    kinds of change join."""
    from flowmirror_hydravox_amd.worker import _TaskSource
    mm, q, results = _mm(), queue.Queue(), {}
    tasks = [_tts(1), _tts(2, inference_head_num=3), _tts(3, inference_head_num=1), _tts(4, inference_head_num=0), _tts(5, inference_head_num=4),
             _tts(6, inference_head_num=5), _tts(7), _tts(8, top_k=5), _tts(9, top_k=5, inference_head_num=3), None]
    for t in tasks[1:]:
        q.put(t)
    src = _TaskSource(mm, q, results, tasks[0], lambda s: s, 0, mixed_heads=True, head_cap=4)
    assert src._joins(tasks[0])
    us = _drain(src)
    assert [u.tag['id'] for u in us] == [1, 2, 3, 4, 5]
    assert [u.inference_head_num for u in us] == [2, 3, 1, 0, 4]              # as the task gave it: the engine applies the reference's rule (0 -> 1)
    assert all(u.sampling is None for u in us)                                # (mixed_sampling is off: the LM's parameters)
    assert src.carry['id'] == 6 and not src.stop                              # 5 heads > head_cap 4: the next epoch's
    with pytest.raises(StopIteration):
        src.poll(True)
    # a grid of 5 rows per sequence holds it; the next boundary is the top_k change (the four sampling values are still the epoch's)
    src = _TaskSource(mm, q, results, src.carry, lambda s: s, 0, mixed_heads=True, head_cap=5)
    assert [u.tag['id'] for u in _drain(src)] == [6, 7] and src.carry['id'] == 8 and not src.stop
    # both switches: sampling and head count change inside the epoch
    src = _TaskSource(mm, q, results, src.carry, lambda s: s, 0, mixed_sampling=True, win_cap=64, mixed_heads=True, head_cap=5)
    us = _drain(src)
    assert [u.tag['id'] for u in us] == [8, 9] and us[1].inference_head_num == 3 and us[1].sampling['top_k'] == 5
    assert src.stop and src.carry is None
    assert results == {}
    # the model's head count bounds a request's before head_cap is looked at: 7 heads asked of a 3-head model are 3
    src = _TaskSource(_mm(head_num=3), queue.Queue(), {}, _tts(1), lambda s: s, 0, mixed_heads=True)
    assert src.head_cap == 3 and src._joins(_tts(2, inference_head_num=7)) and src._joins(_tts(3, inference_head_num=-1))
    src = _TaskSource(_mm(head_num=3), queue.Queue(), {}, _tts(1), lambda s: s, 0, mixed_heads=True, head_cap=2)
    assert not src._joins(_tts(2, inference_head_num=7)) and src._joins(_tts(3, inference_head_num=2))


def test_task_source_without_the_switch_closes_on_another_head_count():
    """off (the default, and mixed_sampling alone): another inference_head_num closes the epoch as before and the utterance carries none"""
    from flowmirror_hydravox_amd.worker import _TaskSource
    for kw in ({}, dict(mixed_sampling=True, win_cap=64)):
        mm, q, results = _mm(), queue.Queue(), {}
        q.put(_tts(2))
        q.put(_tts(3, inference_head_num=3))
        src = _TaskSource(mm, q, results, _tts(1), lambda s: s, 0, **kw)
        us = _drain(src)
        assert [u.tag['id'] for u in us] == [1, 2] and all(u.inference_head_num is None for u in us), kw
        assert src.carry['id'] == 3 and not src.stop, kw


def test_effective_head_rule():
    from flowmirror_hydravox_amd.llm import effective_heads
    from oracle import llm_ref
    cfg = types.SimpleNamespace(head_num=5)
    for n in (-3, 0, 1, 2, 5, 6, 100):
        assert effective_heads(n, 5) == llm_ref.effective_heads(cfg, n) == (1 if n <= 0 else min(n, 5)), n
    assert effective_heads(4, 3) == 3 and effective_heads(0, 3) == 1


def test_header_declares_and_ctypes_binds_the_mixed_entry_points(tmp_path):
    from flowmirror_hydravox_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'hvx.h')).read(), flags=re.S)
    for name in ('hvx_ras_sample_mixed', 'hvx_llm_decode_steps_mixed', 'hvx_llm_decode_join_mixed'):
        assert re.search(r'\bint\s+%s\s*\(' % name, src), name
        assert name in _lib.SYMBOLS, name
    assert [len(_lib.SYMBOLS[n][1]) for n in ('hvx_ras_sample_mixed', 'hvx_llm_decode_steps_mixed', 'hvx_llm_decode_join_mixed')] == [4, 7, 15]
    assert re.search(r'#define\s+HVX_ABI_VERSION\s+8\b', src)
    c = tmp_path / 's.c'
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hvx.h"\n'
                 'int main(){printf("%zu %zu\\n", sizeof(hvx_seq_heads), offsetof(hvx_seq_heads, head_k));return 0;}\n')
    exe = tmp_path / 's'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(_lib.SeqHeads), _lib.SeqHeads.head_k.offset]
    lib = _lib.load()                                          # binds every symbol of SYMBOLS, the three new ones included, or raises
    for name in ('hvx_ras_sample_mixed', 'hvx_llm_decode_steps_mixed', 'hvx_llm_decode_join_mixed'):
        assert getattr(lib, name) is not None
    assert lib.hvx_abi_version() == _lib.HVX_ABI_VERSION == 8
    # refusals that need no device: a heads block without its array, null arguments
    a, hd = _lib.SampleArgs(), _lib.SeqHeads()
    assert lib.hvx_ras_sample_mixed(ctypes.byref(a), None, ctypes.byref(hd), None) == -1 and b'heads block' in lib.hvx_last_error()
    assert lib.hvx_llm_decode_steps_mixed(None, None, None, None, None, 1, 1) == -1 and lib.hvx_last_error()
    d = _lib.DecodeArgs()
    d.head_k = 4
    hd.head_k = 16
    for k in (0, 5):
        assert lib.hvx_llm_decode_join_mixed(None, None, ctypes.byref(d), None, ctypes.byref(hd), 0, 0, 0, 0, 0, 25, 0.8, 10, 1, k) == -1
        assert b'head count %d outside [1,head_k=4]' % k in lib.hvx_last_error()
