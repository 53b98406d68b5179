#!/usr/bin/env python3
"""Throughput of the QUEUE WORKER (worker.serve_queue: the reference's task / result protocol served by the continuous-batching engine) at the
bench workload: N `tts` tasks of 512 text tokens pushed through a queue, HydraVox-CV3 bf16 LM + flow, fp32-contract vocoder, seeded random
weights; a stand-in frontend turns the task text into token ids (the real text / audio frontends are outside this build).

    python tools/bench_worker.py [--tasks 64] [--chars 512] [--lm-slots 64] [--acoustic-batch 4] [--one-by-one] [--alternate-sampling] [--mixed-sampling] [--alternate-heads] [--mixed-heads]
    python tools/bench_worker.py --long-text [--lm-slots 64] [--acoustic-batch 4]

--alternate-sampling: the tasks carry `extra_params` that alternate between two sampling parameter sets (same inference_head_num) — the worst
case for the worker's epochs: without --mixed-sampling every task closes the running decode grid.  --mixed-sampling serves the queue with
serve_queue(mixed_sampling=True): the parameters are per-sequence state of the grid and the tasks share it.
--alternate-heads: the tasks carry `extra_params` that alternate between two head counts (2 and 5, same sampling parameters); without
--mixed-heads every task closes the running grid, with it (serve_queue(mixed_heads=True)) they share one grid of head_num rows per sequence.
The A/B is four runs — off, on, off, on — each in its own process on the same box.
--long-text: another workload, both settings in THIS process: one `tts` task of 5001+ characters followed by eight 64-character tasks (text ids by
character, 5.5 speech tokens per character), served by serve_queue with segment_fanout off (the long task drains the grid and runs segment by
segment between two epochs) and on (its ~170 segments share the grid with everybody), same task seeds.  Prints, per setting, the seconds until the
long task's result, until the last short task's result, and epochs / epoch_boundaries.
"""
import argparse
import json
import os
import queue
import sys
import threading
import time
import types
from functools import partial

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument('--tasks', type=int, default=64)
ap.add_argument('--chars', type=int, default=512)
ap.add_argument('--lm-slots', type=int, default=64)
ap.add_argument('--acoustic-batch', type=int, default=4)
ap.add_argument('--one-by-one', action='store_true', help='the reference loop instead: worker_process_tts semantics, one task at a time')
ap.add_argument('--alternate-sampling', action='store_true', help='tasks alternate between two sampling parameter sets (extra_params)')
ap.add_argument('--mixed-sampling', action='store_true', help='serve_queue(mixed_sampling=True): requests with different sampling parameters share the grid')
ap.add_argument('--alternate-heads', action='store_true', help='tasks alternate between two head counts (extra_params.inference_head_num = 2 / 5)')
ap.add_argument('--mixed-heads', action='store_true', help='serve_queue(mixed_heads=True): requests with different head counts share the grid')
ap.add_argument('--long-text', action='store_true', help='one 5001+ character task and eight 64-character tasks, serve_queue(segment_fanout) off and on')
a = ap.parse_args()
if a.long_text:
    a.chars = 96                                         # sizes the models for the longest utterance of that workload: 64 characters, and the unsegmented warm-up text (under 70)
from flowmirror_hydravox_amd import cv3_config, weights as W  # noqa: E402
from flowmirror_hydravox_amd.flow import HvxFlow  # noqa: E402
from flowmirror_hydravox_amd.hift import HvxHift  # noqa: E402
from flowmirror_hydravox_amd.llm import HvxLLM  # noqa: E402
from flowmirror_hydravox_amd.model_manager import _synthesize  # noqa: E402
from flowmirror_hydravox_amd.sampling import ras_sampling  # noqa: E402
from flowmirror_hydravox_amd.worker import serve_queue  # noqa: E402

cfg = cv3_config()
ratio = 5.5
n_spk = int(a.chars * ratio)


class Frontend:
    def text_normalize(self, text, split=True, text_frontend=True):
        return [text] if split else text

    def frontend_sft(self, text, spk_id):
        if a.long_text:                                  # real texts: one id per character
            g = torch.Generator().manual_seed(len(text))
            return dict(text=torch.tensor([[(ord(c) * 7919) % 151643 for c in text]], dtype=torch.int32), text_len=torch.tensor([len(text)], dtype=torch.int32),
                        llm_embedding=torch.zeros(0, 192), flow_embedding=torch.randn(192, generator=g))
        g = torch.Generator().manual_seed(int(text))
        return dict(text=torch.randint(0, 151643, (1, a.chars), generator=g, dtype=torch.int32), text_len=torch.tensor([a.chars], dtype=torch.int32),
                    llm_embedding=torch.zeros(0, 192), flow_embedding=torch.randn(192, generator=g))


llm = HvxLLM(cfg.llm, W.make_llm_state(cfg.llm, seed=1986), dtype=torch.bfloat16, inference_head_num=2, max_batch=a.lm_slots,
             max_ctx=2 + a.chars + n_spk + 2 + 32, sampling=partial(ras_sampling, top_p=0.9, top_k=10, win_size=32, tau_r=0.2))
flow = HvxFlow(cfg.flow, W.make_flow_state(cfg.flow, seed=1987), dtype=torch.bfloat16, max_t=2 * n_spk + 64)
hift = HvxHift(cfg.hift, W.make_hift_state(cfg.hift, seed=1988))
mm = types.SimpleNamespace(models={'llm': llm, 'flow': flow, 'hift': hift}, device='cuda', configs={'sample_rate': 24000}, frontend=Frontend(),
                           hvx_config=cfg, load_pt=lambda *x: {'status': 'error', 'message': 'not in this probe'}, is_loaded=True,
                           get_available_speakers=lambda: [])        # (no speaker table: any speaker_id the tasks name is accepted)
# random weights never emit EOS sensibly: pin the length through the ratios, as bench.py does (the queue protocol has no such field: patch the defaults)
import flowmirror_hydravox_amd.pipeline as P  # noqa: E402
_serve = P.HvxPipeline.serve
P.HvxPipeline.serve = lambda self, src, **kw: _serve(self, src, max_token_text_ratio=ratio, min_token_text_ratio=ratio, **kw)


SETS = [dict(top_p=0.9, top_k=10, win_size=32, tau_r=0.2, inference_head_num=2), dict(top_p=0.8, top_k=25, win_size=10, tau_r=0.1, inference_head_num=2)]
counters = {}


def run(n, one_by_one):
    q, results = queue.Queue(), {}
    for i in range(n):
        t = dict(id=i, task_type='tts', text=str(i), speaker_id='s', seed=i)
        if a.alternate_sampling:
            t['extra_params'] = dict(SETS[i % 2])
        if a.alternate_heads:
            t['extra_params'] = dict(t.get('extra_params') or SETS[1], inference_head_num=(2, 5)[i % 2])
        q.put(t)
    q.put(None)
    torch.cuda.synchronize()
    t0 = time.time()
    if one_by_one:
        orig = llm.inference
        while True:
            t = q.get()
            if t is None:
                break
            llm.inference = lambda **kw: orig(seed=t['seed'], **dict(kw, max_token_text_ratio=ratio, min_token_text_ratio=ratio))
            if 'extra_params' in t:
                ep = t['extra_params']
                llm.sampling = partial(ras_sampling, top_p=ep['top_p'], top_k=ep['top_k'], win_size=ep['win_size'], tau_r=ep['tau_r'])
                llm.inference_head_num = ep['inference_head_num']
            out = _synthesize(mm, mm.frontend.frontend_sft(t['text'], t['speaker_id']), 1.0, zero_shot=False)
            results[t['id']] = {'output_audio': out, 'duration': out.shape[-1] / 24000}
        llm.inference = orig
    else:
        counters.update(serve_queue(mm, q, results, lm_slots=a.lm_slots, acoustic_batch=a.acoustic_batch, normalise=lambda s: s, mixed_sampling=a.mixed_sampling,
                                    mixed_heads=a.mixed_heads) or {})
    torch.cuda.synchronize()
    dt = time.time() - t0
    assert len(results) == n and all('output_audio' in r for r in results.values()), [r for r in results.values() if 'error' in r][:2]
    audio = sum(r['duration'] for r in results.values())
    return dt, audio


class _Timed(dict):
    """a result dict that notes when every key was written"""

    def __init__(self, t0):
        super().__init__()
        self.t0, self.at = t0, {}

    def __setitem__(self, k, v):
        self.at.setdefault(k, time.time() - self.t0)
        super().__setitem__(k, v)


def long_text(n_chars, n_short, fanout, chars=None):
    words = ['lorem', 'ipsum', 'dolor', 'sit', 'amet', 'consectetur', 'adipiscing', 'elit', 'sed', 'do']
    text, k = '', 0
    while len(text) < n_chars:                           # a sentence mark every three words: pieces of 15 .. 30 characters
        text += ' '.join(words[(k + j) % len(words)] for j in range(3)) + '.,;!?'[k % 5] + ' '
        k += 1
    q = queue.Queue()
    q.put(dict(id='long', task_type='tts', text=text, speaker_id='s', seed=1000))
    for i in range(n_short):
        q.put(dict(id='short%d' % i, task_type='tts', text=('short task number %d ' % i + 'x' * 64)[:64], speaker_id='s', seed=2000 + i))
    q.put(None)
    orig = llm.inference                                 # (the one-by-one path of the switch-off run calls llm.inference with the default ratios)
    llm.inference = lambda **kw: orig(**dict(kw, max_token_text_ratio=ratio, min_token_text_ratio=ratio))
    torch.cuda.synchronize()
    results = _Timed(time.time())
    try:
        st = serve_queue(mm, q, results, lm_slots=a.lm_slots, acoustic_batch=a.acoustic_batch, normalise=lambda s: s, segment_fanout=fanout, segmented_text_chars=chars)
    finally:
        llm.inference = orig
    torch.cuda.synchronize()
    assert all('output_audio' in results[k] for k in ['long'] + ['short%d' % i for i in range(n_short)]), [r for r in results.values() if 'error' in r][:2]
    return dict(segment_fanout=fanout, chars=len(text), segments=(results['long']['segments_info'] or {}).get('total_segments'), long_task_seconds=round(results.at['long'], 3),
                last_short_task_seconds=round(max(results.at['short%d' % i] for i in range(n_short)), 3), audio_seconds=round(sum(r['duration'] for r in results.values()), 2),
                epochs=st['epochs'], epoch_boundaries=st['epoch_boundaries'], fanned_out=st['fanned_out'])


if a.long_text:
    for fanout in (False, True):                         # warm-up of both paths (graphs, workspaces) on a small job of the same kind
        long_text(40, 2, fanout, chars=30)               # (40 .. 68 characters: off, one plain utterance on the one-by-one path; on, two or three segments)
    runs = [long_text(5001, 8, fanout) for fanout in (False, True)]
    print(json.dumps({'path': 'worker.serve_queue, one long tts task + 8 short ones', 'lm_slots': a.lm_slots, 'acoustic_batch': a.acoustic_batch, 'off': runs[0], 'on': runs[1]}))
    sys.exit(0)
run(min(a.tasks, 4), a.one_by_one)                       # warm-up (graphs, workspaces)
dt, audio = run(a.tasks, a.one_by_one)
print(json.dumps({'path': 'worker_process_tts (one task at a time, reference loop)' if a.one_by_one else 'worker.serve_queue (continuous engine)', 'tasks': a.tasks,
                  'chars': a.chars, 'seconds': round(dt, 2), 'requests_per_s': round(a.tasks / dt, 3), 'speech_tokens_per_s': round(a.tasks * n_spk / dt, 1),
                  'rtf': round(dt / audio, 6), 'lm_slots': a.lm_slots, 'acoustic_batch': a.acoustic_batch, 'alternate_sampling': a.alternate_sampling,
                  'mixed_sampling': a.mixed_sampling, 'alternate_heads': a.alternate_heads, 'mixed_heads': a.mixed_heads, 'epochs': counters.get('epochs'), 'epoch_boundaries': counters.get('epoch_boundaries')}))
