"""worker_process_tts — same task / result protocol as the reference's GPU worker (server/worker.py:25-102).

One process per GPU (`CUDA_VISIBLE_DEVICES = worker_id % num_workers_gpu`, :31), tasks popped from a
`multiprocessing.Manager().Queue()`, results written to a `Manager().dict()` keyed by task id; per-request knobs are applied
by mutating the llm object (`llm.sampling = partial(ras_sampling, top_p=, top_k=, win_size=, tau_r=)`,
`llm.inference_head_num`, :57-65); errors never propagate, they become `{"error": str(e)}` (:98-100); `None` is the shutdown
sentinel (:67-68).  The proprietary `fmtn` text normaliser is optional here (its wheel is absent from the reference tree).
"""
import argparse
import logging
import os
from functools import partial

logger = logging.getLogger('hvx.worker')


def _env_flag(name, default=False):
    raw = os.getenv(name)
    if raw is None:
        return default
    return raw.strip().lower() in {'1', 'true', 'yes', 'on'}


def _text_normaliser():
    """the reference worker's `fmtn` normaliser (server/worker.py:46-52, 72-88); identity when the proprietary wheel is absent"""
    try:
        from fmtn import create_default_tn
        return create_default_tn(verbose=True).process_text
    except Exception:
        return lambda s: s


def worker_process_tts(num_workers_gpu, task_queue, result_dict, worker_id, frontend_factory=None):
    os.environ['CUDA_VISIBLE_DEVICES'] = str(worker_id % num_workers_gpu)
    from .model_manager import HvxModelManager, text_to_speech, inference_zero_shot
    from .sampling import ras_sampling

    model_manager = HvxModelManager(frontend_factory=frontend_factory)
    args = argparse.Namespace(config=os.getenv('TTS_CONFIG'), model_dir=os.getenv('TTS_MODEL_DIR'), bf16=_env_flag('TTS_BF_16'),
                              fp16=_env_flag('TTS_FP_16'), cpu=_env_flag('TTS_CPU', False))
    model_manager.load_models(args)
    normalise = _text_normaliser()
    while True:
        task = task_queue.get()
        if task is None:
            break
        speed = 1.0
        if 'extra_params' in task:
            ep = task['extra_params']
            model_manager.models['llm'].sampling = partial(ras_sampling, top_p=ep['top_p'], top_k=ep['top_k'], win_size=ep['win_size'],
                                                           tau_r=ep['tau_r'])
            model_manager.models['llm'].inference_head_num = ep['inference_head_num']
            speed = float(ep.get('speed', 1.0))
        try:
            task_type = task['task_type']
            if task_type == 'zero_shot':
                out = inference_zero_shot(model_manager, normalise(task['tts_text']), normalise(task.get('prompt_text', '')),
                                          task['prompt_audio'], task['prompt_sample_rate'], speed=speed)
                sr = model_manager.configs['sample_rate']
                result = {'output_audio': out, 'sample_rate': sr, 'format': task.get('output_format', 'wav'), 'duration': out.shape[-1] / sr}
            elif task_type == 'tts':
                result = text_to_speech(model_manager, normalise(task['text']), task['speaker_id'], speed=speed)
            elif task_type == 'load_pt':
                result = model_manager.load_pt(task['llm_pt'], task['flow_pt'])
            else:
                result = {'error': 'unknown task_type %r' % (task_type,)}
        except Exception as e:
            logger.error('[TTS Worker-%d] Error: %s', worker_id, e)
            result = {'error': str(e)}
        result_dict[task['id']] = result


def _is_segmented(task, normalise, chars=None):
    """a `tts` task whose text takes the reference's segmented path (over 5000 characters, infer_speech_model.py:782-800): many short speaker-TTS
    calls concatenated — served one by one through text_to_speech, as an epoch boundary of the batched worker (or, with segment_fanout, as
    many utterances of the running grid: see _TaskSource).  chars: another threshold than model_manager.SEGMENTED_TEXT_CHARS."""
    from .model_manager import SEGMENTED_TEXT_CHARS
    if task.get('task_type') != 'tts':
        return False
    try:
        return len(normalise(task.get('text') or '')) > (SEGMENTED_TEXT_CHARS if chars is None else int(chars))
    except Exception:
        return False


def segment_seeds(seed, n):
    """the sampler seeds of the n segments of a fanned-out task: (seed + k) mod 2**31, or None for every segment of a task without a seed
    (each then draws its own, as a request without one does)"""
    return [None if seed is None else (int(seed) + k) % 2 ** 31 for k in range(n)]


CANCELLED_RESULT = {'error': 'cancelled', 'cancelled': True}


class _Fan:
    """One segmented `tts` task served as its segments (segment_fanout): the segments, the gaps between them (drawn when the task is expanded, in
    segment order — the draws inference_tts_with_segmentation makes), the `cancel` object all segments share, and what has come back so far."""

    def __init__(self, task, segments, gaps, seeds, cancel, speaker, sr):
        self.task, self.segments, self.gaps, self.seeds, self.cancel, self.speaker, self.sr = task, list(segments), list(gaps), list(seeds), cancel, speaker, sr
        self.n = len(self.segments)
        self.wavs = [None] * self.n
        self.tokens = [None] * self.n
        # streamed: pieces of segment k wait until segment k - 1 is final
        self.held = [[] for _ in range(self.n)]
        self.started = [False] * self.n
        self.final = [False] * self.n
        self.front = 0
        self.pieces = 0

    def _result(self, out):
        return {'output_audio': out, 'sample_rate': self.sr, 'format': 'wav', 'duration': out.shape[-1] / self.sr, 'speaker_id': self.speaker,
                'segments_info': {'total_segments': self.n, 'segments': list(self.segments)}}

    def _gap(self, k, like):
        import torch
        return torch.zeros(1, self.gaps[k - 1], dtype=like.dtype)

    def add(self, k, wav, toks):
        """the waveform of segment k; -> the task's result once every segment has one (text order, the zero gaps between them), else None"""
        import torch
        self.wavs[k], self.tokens[k] = wav.reshape(1, -1).cpu(), list(toks)
        if any(w is None for w in self.wavs):
            return None
        parts = []
        for j, w in enumerate(self.wavs):
            if j:
                parts.append(self._gap(j, w))
            parts.append(w)
        return self._result(torch.cat(parts, dim=-1))

    def failure(self, k, err):
        return {'error': 'TTS failed: segment %d failed: %s' % (k + 1, err)}

    def piece(self, k, wav, final, toks=None):
        """a piece of segment k (streamed) -> the messages that may leave now, in text order: [(audio (1, L), piece_index, final of the task)]"""
        import torch
        wav = wav.reshape(1, -1).cpu()
        if not self.started[k]:
            self.started[k] = True
            if k:
                wav = torch.cat([self._gap(k, wav), wav], dim=-1)      # the gap before a later segment rides on its first piece
        self.held[k].append(wav)
        if final:
            self.final[k], self.tokens[k] = True, list(toks or [])
        out = []
        while self.front < self.n:
            for w in self.held[self.front]:
                out.append([w, self.pieces, False])
                self.pieces += 1
            self.held[self.front] = []
            if not self.final[self.front]:
                break
            self.front += 1
        if out and self.front == self.n:
            out[-1][2] = True
        return [tuple(o) for o in out]


def _sampling_key(task):
    ep = task.get('extra_params') or {}
    return tuple(ep.get(k) for k in ('top_p', 'top_k', 'win_size', 'tau_r', 'inference_head_num'))


class _TaskSource:
    """The polling source HvxPipeline.serve reads (one EPOCH of the task queue): consecutive `tts` / `zero_shot` tasks with the same sampling
    parameters become utterances as they arrive and join the decode grid while earlier ones are still in flight.  The first task that cannot
    join — a `load_pt`, other sampling parameters (llm.sampling / inference_head_num are per-model state, server/worker.py:57-65), an unknown
    type, the shutdown sentinel — closes the epoch: it is kept in `carry` and served after everything accepted before it has finished, so
    arrival order around a hot swap is what the reference's one-by-one loop gives.
    mixed_sampling: top_p / top_k / win_size / tau_r are per-sequence state of the decode grid (HvxLLM.generate_stream(mixed_sampling=True)), so
    a task with other values joins the running epoch and its utterance carries them (`Utterance.sampling`; a task without extra_params
    carries None and takes the epoch's).  What still closes the epoch: another inference_head_num (it sets the grid's row count), a window
    that a ring of `win_cap` entries cannot hold (0 = whole history, or more than win_cap), a top_k outside [1, 64], and everything above.
    mixed_heads: inference_head_num is per-sequence state too (HvxLLM.generate_stream(mixed_heads=True)): a task whose effective head count
    (min(n, head_num), <= 0 -> 1) is in [1, head_cap] joins the running epoch and its utterance carries the task's value
    (`Utterance.inference_head_num`); one above head_cap is carried to the next epoch.  Without mixed_sampling the four sampling values must
    still be the epoch's.
    segment_fanout: a `tts` task over the segmented-text threshold that passes `_joins` is no epoch boundary: it is expanded into its segments
    (model_manager.segments_of), one utterance each, built as inference_tts builds a segment, with the task's speed, sampling and head count and the
    seeds segment_seeds gives; they are served in order before the queue is read further.  All carry the task (`tag`), their `segment` = (_Fan,
    index) and the fan's one `cancel`.  While segments wait, the front of the queue is still looked at for `cancel` tasks, up to the first other item: that
    one item is kept in `backlog` (shared with serve_queue, which reads it before the queue) and nothing more is read until it has been served.
    cancel tasks: {'task_type': 'cancel', 'id': c, 'target_id': x} never closes the epoch.  Every utterance carries a `cancel` event, registered in
    `cancels` under its task id until the task is answered (`answer`); a cancel task whose target is registered sets it, answers x with
    CANCELLED_RESULT and c with {'cancelled': True}; any other target gives {'cancelled': False}.  The registry is keyed by task id, as the result dict
    is: of two tasks with the SAME id in flight in one epoch only the first answer is written (before the registry the later one overwrote it); ids are
    the protocol's keys and are expected to be unique."""

    def __init__(self, mm, task_queue, result_dict, first, normalise, worker_id, mixed_sampling=False, win_cap=64, mixed_heads=False, head_cap=None,
                 segment_fanout=False, segmented_text_chars=None, backlog=None):
        from collections import deque
        self.mm, self.q, self.results, self.normalise, self.worker_id = mm, task_queue, result_dict, normalise, worker_id
        self.fanout, self.seg_chars = bool(segment_fanout), segmented_text_chars
        self.backlog = backlog if backlog is not None else deque()
        self.pending = deque()                 # (fan, segment index) of the task being expanded, in text order
        self.cancels = {}                      # task id -> the cancel event of a task that has no answer yet
        self.n_fanned = self.n_cancelled = 0
        self.mixed, self.win_cap = bool(mixed_sampling), int(win_cap)
        self.mixed_heads = bool(mixed_heads)
        self.key = _sampling_key(first)
        # the head count the epoch's grid is built with: the first task's, or (a first task without extra_params) what the model holds
        llm = (getattr(mm, 'models', None) or {}).get('llm')
        self.head_num = self.key[4] if first.get('extra_params') else getattr(llm, 'inference_head_num', None)
        # a mixed-heads grid: the model's head count bounds a request's (None: unknown here, the engine applies it) and head_cap is the grid's rows per sequence
        self.model_heads = getattr(llm, 'head_num', None)
        self.head_cap = int(head_cap) if head_cap is not None else self.model_heads
        self.head = first
        self.carry = None
        self.stop = False
        self.closed = False

    POLL_SECONDS = 0.1

    def _heads_fit(self, ep):
        """is the head count of these extra_params one a grid of head_cap rows per sequence holds?"""
        from .llm import effective_heads
        try:
            n = int(ep['inference_head_num'])
        except (KeyError, TypeError, ValueError):
            return False
        k = effective_heads(n, n if self.model_heads is None else self.model_heads)
        return self.head_cap is None or k <= self.head_cap

    def _joins(self, t):
        """does task t (tts / zero_shot, not segmented) belong to this epoch?"""
        if not self.mixed:
            if self.mixed_heads and t.get('extra_params') and _sampling_key(t)[:4] == self.key[:4]:
                return self._heads_fit(t['extra_params'])
            return _sampling_key(t) == self.key
        ep = t.get('extra_params')
        if not ep:
            return True                                # the epoch's defaults, whatever they are
        try:
            fits = 1 <= int(ep['win_size']) <= self.win_cap and 1 <= int(ep['top_k']) <= 64
        except (KeyError, TypeError, ValueError):
            return False                               # (an incomplete set: served on its own, where the one-by-one rules answer it)
        if self.mixed_heads:
            return fits and self._heads_fit(ep)
        return fits and ep.get('inference_head_num') is not None and ep.get('inference_head_num') == self.head_num

    def unpoll(self, u):
        """an utterance the engine fetched while it was being cancelled: its task opens the next epoch instead of failing with this one"""
        self.carry, self.closed = u.tag, True

    def answer(self, task_id, result):
        """write the one answer of a synthesis task; False (nothing written) when it has been answered already — by a cancel task, a failed sibling segment"""
        if self.cancels.pop(task_id, None) is None:
            return False
        self.results[task_id] = result
        return True

    def _cancel_task(self, c):
        ev = self.cancels.pop(c.get('target_id'), None)
        if ev is not None:
            self.results[c['target_id']] = dict(CANCELLED_RESULT)
            ev.set()                                   # (after the answer: whatever the target still delivers finds it answered)
            self.n_cancelled += 1
        self.results[c['id']] = {'cancelled': ev is not None}

    def _scan(self):
        """segments are waiting: cancel tasks at the front of the queue are honoured now.  The look-ahead is bounded: it stops at the first item that is no
        cancel task and keeps that ONE item in `backlog` (served next, before the queue) — the queue may be shared with other workers, which must not lose
        their tasks or their shutdown sentinels to a worker that is busy with a long expansion; nothing more is read while an item is held."""
        import queue as _queue
        while not self.backlog:
            try:
                t = self.q.get_nowait()
            except _queue.Empty:
                return
            if t is not None and t.get('task_type') == 'cancel':
                self._cancel_task(t)
            else:
                self.backlog.append(t)

    def _expand(self, t):
        """a segmented task becomes its segments (text_to_speech's checks first, as in _utterance)"""
        import random
        import threading
        from .model_manager import resolve_tts_request, segments_of
        try:
            text = self.normalise(t['text'])
            speaker = resolve_tts_request(self.mm, text, t.get('speaker_id'))
        except Exception as e:
            raise ValueError('TTS failed: %s' % e)
        segs = segments_of(text)
        sr = self.mm.configs['sample_rate']
        gaps = [int(random.uniform(50, 150) * sr / 1000) for _ in range(len(segs) - 1)]
        fan = _Fan(t, segs, gaps, segment_seeds(t.get('seed'), len(segs)), threading.Event(), speaker, sr)
        self.cancels[t['id']] = fan.cancel
        self.pending.extend((fan, k) for k in range(fan.n))
        self.n_fanned += 1

    def _segment(self, fan, k):
        from .pipeline import Utterance
        fe = self.mm.frontend
        mi = fe.frontend_sft(fe.text_normalize(fan.segments[k], split=True, text_frontend=True)[0], fan.speaker)
        u = Utterance(text=mi['text'].reshape(-1), seed=None, embedding=mi['flow_embedding'].reshape(-1))
        u.speaker_id = fan.speaker
        self._knobs(u, fan.task)
        u.seed, u.segment, u.cancel = fan.seeds[k], (fan, k), fan.cancel
        return u

    def _utterance(self, t):
        import threading
        from .pipeline import Utterance
        from .model_manager import resolve_tts_request
        fe, mm = self.mm.frontend, self.mm
        if t['task_type'] == 'tts':
            # the same checks and the same default speaker as the one-by-one path (model_manager.text_to_speech, infer_speech_model.py:743-780)
            try:
                text = self.normalise(t['text'])
                speaker = resolve_tts_request(mm, text, t.get('speaker_id'))
            except Exception as e:
                raise ValueError('TTS failed: %s' % e)
            mi = fe.frontend_sft(fe.text_normalize(text, split=True, text_frontend=True)[0], speaker)
            u = Utterance(text=mi['text'].reshape(-1), seed=None, embedding=mi['flow_embedding'].reshape(-1))
            u.speaker_id = speaker
        else:
            p_text = fe.text_normalize(self.normalise(t.get('prompt_text', '')), split=False, text_frontend=True)
            mi = fe.frontend_zero_shot(fe.text_normalize(self.normalise(t['tts_text']), split=True, text_frontend=True)[0], p_text,
                                       (t['prompt_audio'], t['prompt_sample_rate']), mm.configs['sample_rate'], zero_shot_spk_id='')
            u = Utterance(text=mi['text'].reshape(-1), seed=None, embedding=mi['flow_embedding'].reshape(-1),
                          prompt_text=mi['prompt_text'].reshape(-1), prompt_speech_token=mi['llm_prompt_speech_token'].reshape(-1),
                          prompt_feat=mi['prompt_speech_feat'].reshape(-1, mi['prompt_speech_feat'].shape[-1]),
                          flow_prompt_token=mi['flow_prompt_speech_token'].reshape(-1))
        self._knobs(u, t)
        u.cancel = self.cancels[t['id']] = threading.Event()
        return u

    def _knobs(self, u, t):
        """seed, speed, sampling, head count and tag of task t on utterance u"""
        u.seed = int(t['seed']) if t.get('seed') is not None else None       # (None: the LM draws one from the global generator)
        u.speed = float((t.get('extra_params') or {}).get('speed', 1.0))
        if u.speed <= 0:
            raise ValueError('Invalid speed: %s' % u.speed)
        if self.mixed and t.get('extra_params'):
            ep = t['extra_params']
            u.sampling = dict(top_p=ep['top_p'], top_k=ep['top_k'], win_size=ep['win_size'], tau_r=ep['tau_r'])
        if self.mixed_heads and t.get('extra_params'):
            u.inference_head_num = int(t['extra_params']['inference_head_num'])
        u.tag = t

    def poll(self, block):
        import queue as _queue
        while True:
            if self.closed:
                raise StopIteration
            if self.pending:
                self._scan()
                fan, k = self.pending.popleft()
                if fan.cancel.is_set():                # cancelled, or a sibling failed: what waits of it never joins
                    continue
                try:
                    return self._segment(fan, k)
                except Exception as e:                 # a frontend error of one segment fails the task, once
                    logger.error('[TTS Worker-%d] Error: %s', self.worker_id, e)
                    self.answer(fan.task['id'], fan.failure(k, e))
                    fan.cancel.set()
                    continue
            if self.head is not None:
                t, self.head = self.head, None
            elif self.backlog:
                t = self.backlog.popleft()
            else:
                try:
                    # bounded: the engine asks again (and looks at its cancellation flag) every time this returns None — a blocking get()
                    # would hold a cancelled engine, and the error replies of its requests, until the next task arrived
                    t = self.q.get(timeout=self.POLL_SECONDS) if block else self.q.get_nowait()
                except _queue.Empty:
                    return None
            if t is None:
                self.stop = self.closed = True
                raise StopIteration
            if t.get('task_type') == 'cancel':
                self._cancel_task(t)
                continue
            segmented = _is_segmented(t, self.normalise, self.seg_chars)
            if t.get('task_type') not in ('tts', 'zero_shot') or not self._joins(t) or (segmented and not self.fanout):
                self.carry, self.closed = t, True
                raise StopIteration
            try:
                if segmented:
                    self._expand(t)
                    continue
                return self._utterance(t)
            except Exception as e:                     # a frontend error fails that request only
                logger.error('[TTS Worker-%d] Error: %s', self.worker_id, e)
                self.results[t['id']] = {'error': str(e)}


def worker_process_tts_batched(num_workers_gpu, task_queue, result_dict, worker_id, frontend_factory=None, lm_slots=None, acoustic_batch=4,
                               mixed_sampling=False, mixed_heads=False, stream=False, segment_fanout=False, incremental_vocoder=False,
                               incremental_flow=False):
    """Same wire format as worker_process_tts, served by the continuous-batching engine (replaces the one-request-at-a-time
    loop of server/worker.py:54-102 and what server/router.py:144-156 feeds it): `tts` / `zero_shot` tasks join ONE decode grid as they arrive
    (HvxPipeline.serve -> HvxLLM.generate_stream: the LM weights are streamed once per step for every request in flight, a finished request's
    slot goes to the next waiting one), finished requests go to length-bucketed padded CFM solves and the vocoder beside the decode of the
    others, and every result is written to `result_dict` the moment its waveform is complete.  `load_pt` and a change of sampling parameters
    are epoch boundaries (FIFO: see _TaskSource).  What bench.py measures is this path.
    mixed_sampling=True: requests with different top_p / top_k / win_size / tau_r share the grid, each sampling with its own values; only
    another inference_head_num, a window over 64 (or 0) and the non-synthesis tasks remain epoch boundaries.
    mixed_heads=True: requests with different inference_head_num share the grid as well (rows per sequence: the model's head_num).
    stream=True: one result message per audio PIECE (see serve_queue).
    incremental_vocoder=True (with stream=True): the pieces come from a per-request vocoder stream instead of a pass over the whole mel cache (see serve_queue).
    incremental_flow=True (with stream=True): non-final pieces solve a window of the flow against per-request K / V caches instead of the whole prefix (see serve_queue).
    segment_fanout=True: a `tts` task over 5000 characters no longer drains the grid: its segments are utterances of the running epoch (see serve_queue)."""
    os.environ['CUDA_VISIBLE_DEVICES'] = str(worker_id % num_workers_gpu)
    from .model_manager import HvxModelManager
    from .pipeline import HvxPipeline
    from .sampling import ras_sampling

    mm = HvxModelManager(frontend_factory=frontend_factory)
    mm.load_models(argparse.Namespace(config=os.getenv('TTS_CONFIG'), model_dir=os.getenv('TTS_MODEL_DIR'), bf16=_env_flag('TTS_BF_16'),
                                      fp16=_env_flag('TTS_FP_16'), cpu=_env_flag('TTS_CPU', False)))
    serve_queue(mm, task_queue, result_dict, worker_id, lm_slots=lm_slots, acoustic_batch=acoustic_batch, mixed_sampling=mixed_sampling,
                mixed_heads=mixed_heads, **(dict(stream=True) if stream else {}), **(dict(segment_fanout=True) if segment_fanout else {}),
                **(dict(incremental_vocoder=True) if incremental_vocoder else {}), **(dict(incremental_flow=True) if incremental_flow else {}))


def serve_queue(mm, task_queue, result_dict, worker_id=0, lm_slots=None, acoustic_batch=4, normalise=None, mixed_sampling=False, win_cap=64, token_log=None,
                mixed_heads=False, head_cap=None, stream=False, segment_fanout=False, segmented_text_chars=None, incremental_vocoder=False, incremental_flow=False):
    """the loop of worker_process_tts_batched over an already loaded model manager (tests drive this directly).  Returns its counters:
    `epochs` (decode grids started) and `epoch_boundaries` (tasks that closed a running grid because they could not join it; the shutdown
    sentinel is not one).  token_log: a dict that receives task id -> speech-token ids of every synthesised request.
    mixed_heads / head_cap: see _TaskSource; llm.inference_head_num is still written at epoch start only (the first task's).
    stream=True: HvxPipeline.serve(stream=True) — every audio piece of a request is a result message of its own, written the moment the piece exists under
    the key stream_result_key(task id, piece_index): the keys of an unstreamed result (`output_audio` = this piece's samples, `duration` = this piece's) plus
    `piece_index` and `final`.  A request that fails is answered once, under its task id, as without the switch.
    incremental_vocoder=True: HvxPipeline.serve(stream=True, incremental_vocoder=True) — same messages, the vocoder works on a window per piece (hift.HiftStream);
    without stream=True it is refused with a ValueError before anything is served.
    incremental_flow=True: HvxPipeline.serve(stream=True, incremental_flow=True) — same messages, non-final pieces solve a window of the flow (flow.FlowStream); refused
    without stream=True in the same way; independent of incremental_vocoder.
    segment_fanout=True: a `tts` task over `segmented_text_chars` characters (None: model_manager.SEGMENTED_TEXT_CHARS) that can join an epoch is served as
    its segments in the decode grid (_TaskSource) instead of one by one between two epochs.  When the last segment has its waveform, ONE result is written
    under the task id: the keys of text_to_speech's segmented result, `output_audio` = the segments in text order with the zero gaps between them.  The first
    segment that fails answers the task once ('TTS failed: segment %d failed: ...', 1-based) and sets the shared `cancel`: siblings in flight are retired,
    waiting ones never join, what they still deliver is discarded.  token_log[task id] is the list of the segments' id lists.  With stream=True the pieces
    leave in text order (pieces of segment k are held until segment k - 1 is final), `piece_index` counts over the task, the gap before segment k >= 1 is
    prepended to its first piece, and `final` is true only on the last piece of the last segment, which carries `segments_info`.
    A task {'task_type': 'cancel', 'id': c, 'target_id': x} is honoured inside a running epoch without closing it (_TaskSource); outside one it is answered
    {'cancelled': False}.  Counters: `fanned_out` (tasks expanded) and `cancelled` (cancel tasks honoured)."""
    from collections import deque
    if incremental_vocoder and not stream:
        raise ValueError('incremental_vocoder needs stream=True: an unstreamed request is vocoded once')
    if incremental_flow and not stream:
        raise ValueError('incremental_flow needs stream=True: an unstreamed request is solved once')
    stats = dict(epochs=0, epoch_boundaries=0, mixed_sampling=bool(mixed_sampling), mixed_heads=bool(mixed_heads), fanned_out=0, cancelled=0)
    backlog = deque()                                  # the one task a source read past while segments were waiting (it was looking for cancel tasks): served before the queue
    fan_kw = dict(segment_fanout=bool(segment_fanout), segmented_text_chars=segmented_text_chars, backlog=backlog)
    from .llm import Cancelled
    from .pipeline import HvxPipeline
    from .sampling import ras_sampling
    normalise = normalise or _text_normaliser()
    pipe = HvxPipeline.from_models(mm.hvx_config, mm.models['llm'], mm.models['flow'], mm.models['hift'], acoustic_batch=acoustic_batch)
    lm_slots = lm_slots or mm.models['llm'].max_batch
    sr = mm.configs['sample_rate']
    carry = None
    while True:
        task, carry = (carry, None) if carry is not None else (backlog.popleft() if backlog else task_queue.get(), None)
        if task is None:
            break
        if task.get('task_type') not in ('tts', 'zero_shot') or (_is_segmented(task, normalise, segmented_text_chars) and not segment_fanout):
            try:
                if task.get('task_type') == 'load_pt':
                    result = mm.load_pt(task['llm_pt'], task['flow_pt'])
                elif task.get('task_type') == 'tts':               # segmented text: the one-by-one path, with this request's own knobs
                    from .model_manager import text_to_speech
                    result = text_to_speech(mm, normalise(task['text']), task.get('speaker_id'), speed=apply_extra_params(mm, task, ras_sampling))
                elif task.get('task_type') == 'cancel':            # no epoch is running: nothing is in flight
                    result = {'cancelled': False}
                else:
                    result = {'error': 'unknown task_type %r' % (task.get('task_type'),)}
            except Exception as e:
                logger.error('[TTS Worker-%d] Error: %s', worker_id, e)
                result = {'error': str(e)}
            result_dict[task['id']] = result
            continue
        src = _TaskSource(mm, task_queue, result_dict, task, normalise, worker_id, mixed_sampling=mixed_sampling, win_cap=win_cap,
                          **(dict(mixed_heads=True, head_cap=head_cap) if mixed_heads else {}), **fan_kw)
        if (mixed_sampling or mixed_heads) and not src._joins(task):
            # a request no mixed grid can hold (window 0 or over win_cap, more heads than head_cap): an epoch of its own on the scalar engine, as without the switch
            src = _TaskSource(mm, task_queue, result_dict, task, normalise, worker_id, **fan_kw)
        in_flight = {}
        stats['epochs'] += 1
        try:
            apply_extra_params(mm, task, ras_sampling)
            pipe.llm = mm.models['llm']
            kw = dict(mixed_sampling=True, win_cap=win_cap) if src.mixed else {}
            if src.mixed_heads:
                kw.update(mixed_heads=True, head_cap=head_cap)
            if stream:
                kw.update(stream=True)
            if incremental_vocoder:
                kw.update(incremental_vocoder=True)
            if incremental_flow:
                kw.update(incremental_flow=True)
            for u, wav, toks in pipe.serve(_Tracked(src, in_flight), lm_slots=lm_slots, acoustic_batch=acoustic_batch, acoustic_min_batch=1, **kw):
                t = u.tag
                if getattr(u, 'segment', None) is not None:     # a segment of a fanned-out task
                    fan, k = u.segment
                    if isinstance(wav, BaseException):
                        if t['id'] in src.cancels and not isinstance(wav, Cancelled):
                            logger.error('[TTS Worker-%d] Error: %s', worker_id, wav)
                            src.answer(t['id'], fan.failure(k, wav))
                            fan.cancel.set()
                            in_flight.pop(t['id'], None)
                        continue                                # (retired siblings, late errors: the task has its answer)
                    if t['id'] not in src.cancels:
                        continue                                # answered already (a failed sibling, a cancel task): late results are discarded
                    if stream:
                        info = toks
                        for out, index, last in fan.piece(k, wav, info['final'], info.get('tokens')):
                            msg = {'output_audio': out, 'sample_rate': sr, 'format': 'wav', 'duration': out.shape[-1] / sr, 'speaker_id': fan.speaker,
                                   'segments_info': fan._result(out)['segments_info'] if last else None, 'piece_index': index, 'final': last}
                            if last:
                                if src.cancels.pop(t['id'], None) is None:
                                    break
                                in_flight.pop(t['id'], None)
                                if token_log is not None:
                                    token_log[t['id']] = [list(x) for x in fan.tokens]
                            result_dict[stream_result_key(t['id'], index)] = msg
                        continue
                    result = fan.add(k, wav, toks)
                    if result is not None and src.answer(t['id'], result):
                        in_flight.pop(t['id'], None)
                        if token_log is not None:
                            token_log[t['id']] = [list(x) for x in fan.tokens]
                    continue
                if t['id'] not in src.cancels:                  # answered by a cancel task: whatever it still delivers is discarded
                    in_flight.pop(t['id'], None)
                    continue
                if stream and not isinstance(wav, BaseException):
                    info = toks                                 # (utterance, piece, info)
                    if info['final']:
                        if src.cancels.pop(t['id'], None) is None:
                            continue
                        in_flight.pop(t['id'], None)
                        if token_log is not None:
                            token_log[t['id']] = list(info['tokens'])
                    out = wav.reshape(1, -1).cpu()
                    msg = {'output_audio': out, 'sample_rate': sr, 'format': 'wav' if t['task_type'] == 'tts' else t.get('output_format', 'wav'),
                           'duration': out.shape[-1] / sr}
                    if t['task_type'] == 'tts':
                        msg.update(speaker_id=getattr(u, 'speaker_id', t.get('speaker_id')), segments_info=None)
                    msg.update(piece_index=info['index'], final=info['final'])
                    result_dict[stream_result_key(t['id'], info['index'])] = msg
                    continue
                in_flight.pop(t['id'], None)
                if token_log is not None and not isinstance(wav, BaseException):
                    token_log[t['id']] = list(toks)
                if isinstance(wav, Cancelled):
                    src.answer(t['id'], dict(CANCELLED_RESULT))
                elif isinstance(wav, BaseException):
                    logger.error('[TTS Worker-%d] Error: %s', worker_id, wav)
                    src.answer(t['id'], {'error': str(wav)})
                else:
                    out = wav.reshape(1, -1).cpu()
                    if t['task_type'] == 'tts':                 # the result keys of text_to_speech (infer_speech_model.py:802-812)
                        src.answer(t['id'], {'output_audio': out, 'sample_rate': sr, 'format': 'wav', 'duration': out.shape[-1] / sr,
                                             'speaker_id': getattr(u, 'speaker_id', t.get('speaker_id')), 'segments_info': None})
                    else:                                      # ... and of the worker's zero_shot branch (server/worker.py:76-83)
                        src.answer(t['id'], {'output_audio': out, 'sample_rate': sr, 'format': t.get('output_format', 'wav'), 'duration': out.shape[-1] / sr})
        except Exception as e:                         # an engine failure fails what was in flight, never the worker
            logger.error('[TTS Worker-%d] epoch error: %s', worker_id, e)
            for tid in list(in_flight):
                src.answer(tid, {'error': str(e)})
        stats['fanned_out'] += src.n_fanned
        stats['cancelled'] += src.n_cancelled
        carry = src.carry
        if carry is not None:
            stats['epoch_boundaries'] += 1
        if src.stop:
            break
    return stats


def stream_result_key(task_id, piece_index):
    """where serve_queue(stream=True) puts piece `piece_index` of a task's audio in the result dict"""
    return '%s:%d' % (task_id, piece_index)


class _Tracked:
    """notes which accepted tasks have no result yet (an engine failure must answer them)"""

    def __init__(self, src, in_flight):
        self.src, self.in_flight = src, in_flight

    def poll(self, block):
        u = self.src.poll(block)
        if u is not None:
            self.in_flight[u.tag['id']] = True
        return u

    def unpoll(self, u):
        if getattr(u, 'segment', None) is not None:
            return                                     # (one segment of a task: the task stays in flight and fails with the epoch, it is not served twice)
        self.in_flight.pop(u.tag['id'], None)
        self.src.cancels.pop(u.tag['id'], None)
        self.src.unpoll(u)


def apply_extra_params(mm, task, ras_sampling):
    """per-request knobs, exactly as server/worker.py:57-65 applies them; returns the speed"""
    ep = task.get('extra_params')
    if not ep:
        return 1.0
    mm.models['llm'].sampling = partial(ras_sampling, top_p=ep['top_p'], top_k=ep['top_k'], win_size=ep['win_size'], tau_r=ep['tau_r'])
    mm.models['llm'].inference_head_num = ep['inference_head_num']
    return float(ep.get('speed', 1.0))
