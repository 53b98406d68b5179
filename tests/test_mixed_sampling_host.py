"""Host side of per-sequence sampling parameters (no GPU): the queue worker's epoch rule with and without `mixed_sampling`, and the additive
C ABI — hvx_seq_sampling and the three `_seq` entry points — in the header, the library and the ctypes binding."""
import ctypes
import os
import queue
import re
import subprocess
import types

import pytest

from test_host_cpu import _QueueFrontend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EP = dict(top_p=0.8, top_k=25, win_size=10, tau_r=0.1, inference_head_num=2)


def _mm():
    return types.SimpleNamespace(frontend=_QueueFrontend(), configs={'sample_rate': 24000}, is_loaded=True, get_available_speakers=lambda: ['s', 'tt'])


def _tts(i, **ep):
    t = dict(id=i, task_type='tts', text='ab' + 'c' * i, speaker_id='s')
    if ep is not None:
        t['extra_params'] = dict(EP, **ep)
    return t


def test_mixed_task_source_joins_parameter_changes_and_keeps_the_other_boundaries_in_order():
    """_TaskSource(mixed_sampling=True): a change of top_k / top_p / tau_r / win_size joins the running epoch and the utterance carries the task's
    own four values; another inference_head_num, win_size = 65 (> win_cap 64), a load_pt and the sentinel still close it — each is carried, never
    overtaken by what arrived behind it.  A task without extra_params joins with sampling=None (the epoch's defaults)."""
    from flowmirror_hydravox_amd.worker import _TaskSource
    mm, q, results = _mm(), queue.Queue(), {}
    plain = dict(id=6, task_type='tts', text='plain', speaker_id='s')
    tasks = [_tts(1), _tts(2, top_k=5), _tts(3, top_p=0.5), _tts(4, tau_r=0.5), _tts(5, win_size=64), plain,
             _tts(7, inference_head_num=3), _tts(8, inference_head_num=3, top_k=7), _tts(9, inference_head_num=3, win_size=65), _tts(10, inference_head_num=3),
             dict(id=11, task_type='load_pt', llm_pt='x', flow_pt='y'), _tts(12, win_size=0), _tts(13, top_k=65), _tts(14), None]
    for t in tasks[1:]:
        q.put(t)

    def source(first):
        return _TaskSource(mm, q, results, first, lambda s: s, 0, mixed_sampling=True, win_cap=64)

    def drain(src):
        got = []
        while True:
            try:
                u = src.poll(False)
            except StopIteration:
                return got
            assert u is not None
            got.append(u)
    src = source(tasks[0])
    us = drain(src)
    assert [u.tag['id'] for u in us] == [1, 2, 3, 4, 5, 6]
    assert us[0].sampling == dict(top_p=0.8, top_k=25, win_size=10, tau_r=0.1)
    assert us[1].sampling == dict(top_p=0.8, top_k=5, win_size=10, tau_r=0.1)
    assert us[2].sampling['top_p'] == 0.5 and us[3].sampling['tau_r'] == 0.5 and us[4].sampling['win_size'] == 64
    assert us[5].sampling is None                              # no extra_params: the epoch's defaults
    assert src.carry['id'] == 7 and not src.stop               # another head count: the grid's row count, an epoch boundary
    src = source(src.carry)
    us = drain(src)
    assert [u.tag['id'] for u in us] == [7, 8] and us[1].sampling['top_k'] == 7
    assert src.carry['id'] == 9 and not src.stop               # a window the 64-entry ring cannot hold
    with pytest.raises(StopIteration):                         # (closed stays closed)
        src.poll(True)
    # the worker serves task 9 on the scalar engine: an epoch of the default kind, which the next task (window 10) closes in turn
    src = _TaskSource(mm, q, results, src.carry, lambda s: s, 0)
    assert [u.tag['id'] for u in drain(src)] == [9] and src.carry['id'] == 10
    src = source(src.carry)
    assert [u.tag['id'] for u in drain(src)] == [10] and src.carry['id'] == 11 and not src.stop     # load_pt
    src = source(q.get())                                      # (the worker serves the load_pt itself, then opens the next epoch)
    assert src.head['id'] == 12 and not src._joins(src.head)   # win_size 0 (whole history) is no member of a mixed grid either
    src = _TaskSource(mm, q, results, src.head, lambda s: s, 0)
    assert [u.tag['id'] for u in drain(src)] == [12] and src.carry['id'] == 13
    assert not source(src.carry)._joins(src.carry)             # top_k = 65: refused by the mixed rule (and by sampling_params on the scalar path)
    src = source(tasks[13])
    q.get()                                                    # (task 14 was put as well: it is the head of this epoch)
    assert [u.tag['id'] for u in drain(src)] == [14]
    assert src.stop and src.carry is None                      # the sentinel
    assert results == {}


def test_default_task_source_still_closes_on_a_top_k_change():
    from flowmirror_hydravox_amd.worker import _TaskSource
    mm, q, results = _mm(), queue.Queue(), {}
    q.put(_tts(2, top_k=5))
    src = _TaskSource(mm, q, results, _tts(1), lambda s: s, 0)
    u = src.poll(False)
    assert u.tag['id'] == 1 and u.sampling is None             # the default epoch: llm.sampling is the model's, the utterance carries nothing
    with pytest.raises(StopIteration):
        src.poll(False)
    assert src.carry['id'] == 2 and not src.stop


def test_header_declares_and_ctypes_binds_the_seq_entry_points(tmp_path):
    from flowmirror_hydravox_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'hvx.h')).read(), flags=re.S)
    for name in ('hvx_ras_sample_seq', 'hvx_llm_decode_steps_seq', 'hvx_llm_decode_join_seq'):
        assert re.search(r'\bint\s+%s\s*\(' % name, src), name
        assert name in _lib.SYMBOLS, name
    assert len(_lib.SYMBOLS['hvx_llm_decode_join_seq'][1]) == 13 and len(_lib.SYMBOLS['hvx_llm_decode_steps_seq'][1]) == 5
    assert re.search(r'#define\s+HVX_ABI_VERSION\s+8\b', src)
    c = tmp_path / 's.c'
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hvx.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(hvx_seq_sampling), '
                 'offsetof(hvx_seq_sampling, top_k), offsetof(hvx_seq_sampling, top_p), offsetof(hvx_seq_sampling, win_size), '
                 'offsetof(hvx_seq_sampling, rep_thresh));return 0;}\n')
    exe = tmp_path / 's'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    S = _lib.SeqSampling
    assert got == [ctypes.sizeof(S), S.top_k.offset, S.top_p.offset, S.win_size.offset, S.rep_thresh.offset]
    lib = _lib.load()                                          # binds every symbol of SYMBOLS, the three new ones included, or raises
    assert lib.hvx_abi_version() == _lib.HVX_ABI_VERSION == 8
    # refusals that need no device: a sampling block with a missing array, a join without a block
    a, q = _lib.SampleArgs(), _lib.SeqSampling()
    q.top_k = 16
    assert lib.hvx_ras_sample_seq(ctypes.byref(a), ctypes.byref(q), None) == -1 and b'all four arrays' in lib.hvx_last_error()
    assert lib.hvx_llm_decode_join_seq(None, None, None, None, 0, 0, 0, 0, 0, 25, 0.8, 10, 1) == -1 and lib.hvx_last_error()


def test_decode_grid_fixture_is_the_oracle_and_the_window_matters():
    """tests/golden/mixed_sampling_grid.npz (what the GPU grid test compares with) == oracle/llm_ref.py run now, request by request with its own
    parameters; and for the requests in WINDOW_SENSITIVE the stream under window 32 — the ring capacity of that grid — is another one."""
    import sys
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    import mixed_sampling_cases as M
    from conftest import load_golden, state_checksum
    from flowmirror_hydravox_amd import weights as W
    from flowmirror_hydravox_amd.config import cv3w_config
    g, fx = load_golden('llm_cv3w.npz'), load_golden('mixed_sampling_grid.npz')
    cfg = cv3w_config().llm
    sd = W.make_llm_state(cfg, seed=int(g['weight_seed']), init='fan_in', with_lm_head=True)
    assert state_checksum(sd) == str(g['weight_sha'])
    now = M.oracle_fixture(sd, cfg)
    assert sorted(now) == sorted(fx.files)
    for k in now:
        assert np.array_equal(now[k], fx[k]), k
    assert len(M.WINDOW_SENSITIVE) >= 2
    for i in M.WINDOW_SENSITIVE:
        assert len(fx['own_%d' % i]) == len(fx['w32_%d' % i]) >= 100 and not np.array_equal(fx['own_%d' % i], fx['w32_%d' % i]), i
