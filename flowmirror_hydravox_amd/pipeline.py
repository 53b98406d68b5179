"""End-to-end synthesis driver: llm.inference -> flow.inference -> hift.inference for a batch of utterances.

This is the loop of `inference_tts` / `inference_zero_shot` (server/model_utils/infer_speech_model.py:523-606, 612-690)
below the text frontend: speech tokens from the multi-head LM, mel from the flow decoder, waveform from the vocoder,
with the reference's own timing definitions (TPS = tokens / LLM wall, RTF = total wall / audio seconds, :563-565, :594-604).
The LLM decodes all utterances of the batch in lock-step; flow and HiFT run one utterance per call (each saturates the GPU).
"""
import threading
import time
from dataclasses import dataclass, field
from typing import List, Optional

import torch

from .config import HvxConfig
from .flow import HvxFlow
from .hift import HvxHift
from .llm import Cancelled, HvxLLM
from . import weights as W


@dataclass
class Utterance:
    text: torch.Tensor                         # int32 [N_text] text token ids
    seed: int                                  # per-utterance sampler seed (global utterance index in DP runs)
    embedding: torch.Tensor                    # f32 [192] speaker x-vector
    prompt_text: Optional[torch.Tensor] = None
    prompt_speech_token: Optional[torch.Tensor] = None      # int32 [Np]
    prompt_feat: Optional[torch.Tensor] = None              # f32 [2*Np][80]
    flow_prompt_token: Optional[torch.Tensor] = None        # int32 [Np']: the flow decoder's prompt tokens when they differ from the LM's (frontend_zero_shot)
    speed: float = 1.0                                      # mel resampled to T / speed frames before the vocoder (infer_speech_model.py:583-588)
    tag: object = None                                      # caller's handle (a queue task, ...), returned with the result
    max_token_text_ratio: Optional[float] = None            # per-utterance overrides of the call's length ratios
    min_token_text_ratio: Optional[float] = None
    sampling: object = None                                 # own top_p / top_k / win_size / tau_r (dict or partial) in a mixed-sampling grid; None: the LM's
    inference_head_num: Optional[int] = None                # own head count in a mixed-heads grid; None: the LM's
    cancel: object = None                                   # any object with is_set() (serve): once set, the utterance is retired and comes back as Cancelled


def _cancelled(u):
    c = getattr(u, 'cancel', None)
    return c is not None and c.is_set()


@dataclass
class SynthStats:
    tokens: int = 0
    audio_seconds: float = 0.0
    llm_seconds: float = 0.0
    flow_seconds: float = 0.0
    hift_seconds: float = 0.0
    total_seconds: float = 0.0
    per_utt_tokens: List[int] = field(default_factory=list)
    token_ids: List[List[int]] = field(default_factory=list)   # the speech-token ids of every utterance of the batch
    llm: dict = field(default_factory=dict)               # HvxLLM.last_stats of this batch (decode-step timing)

    @property
    def tps(self):
        return self.tokens / self.llm_seconds if self.llm_seconds > 0 else 0.0

    @property
    def rtf(self):
        return self.total_seconds / self.audio_seconds if self.audio_seconds > 0 else 0.0


def synthetic_utterance(cfg: HvxConfig, index: int, n_text: int, n_prompt_speech: int = 0, n_prompt_text: int = 0) -> Utterance:
    """text ids randint(0, 151643) seeded by the utterance index, randn(192) speaker embedding."""
    g = torch.Generator()
    g.manual_seed(index)
    hi = min(151643, cfg.llm.text_vocab)
    text = torch.randint(0, hi, (n_text,), generator=g, dtype=torch.int32)
    emb = torch.randn(cfg.flow.spk_embed_dim, generator=g)
    u = Utterance(text=text, seed=index, embedding=emb)
    if n_prompt_speech:
        u.prompt_speech_token = torch.randint(0, cfg.llm.speech_tokens, (n_prompt_speech,), generator=g, dtype=torch.int32)
        u.prompt_feat = torch.randn(2 * n_prompt_speech, cfg.flow.mel, generator=g)
        u.prompt_text = torch.randint(0, hi, (n_prompt_text,), generator=g, dtype=torch.int32)
    return u


def _flow_prompt(u):
    return u.prompt_speech_token if u.flow_prompt_token is None else u.flow_prompt_token


class _HostStream:
    """the acoustic "stream" of a pipeline over host stand-in models (from_models with objects on the CPU: the scheduling tests) — nothing to order or wait for"""
    device = torch.device('cpu')

    def synchronize(self):
        pass


def _on(stream):
    import contextlib
    return contextlib.nullcontext() if isinstance(stream, _HostStream) else torch.cuda.stream(stream)


class _StreamUtterance:
    """One utterance of `serve(stream=True)` between its first token and its last piece: what `streaming.StreamSession` keeps for a single request,
    as state the batched acoustic stage can work on — the mel cache plane (sized from the utterance's token budget; `fill` frames are valid), the chunk
    schedule, the prompt arguments of the flow, the jobs that are ready and `handed`, the samples already handed out."""

    def __init__(self, u, flow, hop, max_tokens, device, t_fetch, hift=None, incremental_flow=False):
        """hift: given with serve(incremental_vocoder=True) — the utterance owns a vocoder stream (hift.HiftStream) as long as its mel cache plane.
        incremental_flow: it owns a flow stream (flow.FlowStream: K / V^T caches and x-trajectory of its chunk-masked solves) for as long, sized for the prompt's
        frames plus the plane"""
        from .streaming import ChunkSchedule
        pt = _flow_prompt(u)
        self.u = u
        self.prompt_token = None if pt is None else pt.reshape(-1).to(device, torch.int32)
        self.prompt_feat = None if u.prompt_feat is None else u.prompt_feat.reshape(-1, flow.output_size).to(device, torch.float32)
        self.embedding = u.embedding.to(device)
        self.n_prompt = 0 if self.prompt_token is None else int(self.prompt_token.numel())
        self.prompt_frames = 0 if self.prompt_feat is None else int(self.prompt_feat.shape[0])
        self.sched = ChunkSchedule(self.n_prompt, hop, flow.pre_lookahead_len)
        self.cache = torch.empty(flow.output_size, max(1, int(max_tokens)) * flow.token_mel_ratio, dtype=torch.float32, device=device)
        self.fill = 0
        self.handed = 0
        self.vstream = None if hift is None else hift.stream(min(int(self.cache.shape[1]), hift.max_stream_frames))
        self.fstream = flow.stream(min(self.prompt_frames + int(self.cache.shape[1]), flow.max_t)) if incremental_flow else None
        self.jobs = []                   # (tokens in the piece, covered, final) not yet solved, in order
        self.pieces = 0
        self.tokens = None               # the utterance's full token list, once the LM has finished it
        self.t_fetch = t_fetch
        self.dead = False                # cancelled by its caller: nothing more of it is solved; it leaves when the LM hands it back

    def release(self):
        """the utterance leaves (final piece, cancelled, dropped, abandoned): its vocoder stream goes with its mel cache plane"""
        if self.vstream is not None:
            self.vstream.close()
            self.vstream = None
        if self.fstream is not None:
            self.fstream.release()
            self.fstream = None

    def window_rows(self, flow, n, covered):
        """rows the incremental flow solves for the non-final job (n, covered): flow.window_rule over the job's frames and the flow stream's fill"""
        from .flow import window_rule
        ratio = flow.token_mel_ratio
        return window_rule(self.prompt_frames + covered * ratio, ratio * (self.n_prompt + n - flow.pre_lookahead_len), flow.static_chunk_size, fill=self.fstream.fill)[1]

    def flow_inputs(self, flow, n, final):
        """mu, spk, cond of the flow over the prompt and the first n generated tokens (HvxFlow.inference's plumbing)"""
        tok = torch.tensor(self.sched.tokens[:n], dtype=torch.int32, device=self.cache.device)
        if self.prompt_token is not None:
            tok = torch.concat([self.prompt_token, tok])
        mu, spk = flow.encode(tok, self.embedding.reshape(-1), finalize=final)
        cond = torch.zeros(flow.output_size, mu.shape[-1], dtype=torch.float32, device=self.cache.device)
        if self.prompt_feat is not None:
            cond[:, :self.prompt_frames] = self.prompt_feat.t()
        return mu, spk, cond


class HvxPipeline:
    def __init__(self, cfg: HvxConfig, llm_sd=None, flow_sd=None, hift_sd=None, llm_dtype=torch.bfloat16, flow_dtype=torch.bfloat16,
                 device='cuda', max_batch=8, max_ctx=4096, max_t=None, seed=1986, init='normal02', hift_tables=None, sampling=None,
                 inference_head_num=2, hift_exact_fp32=False):
        self.cfg = cfg
        llm_sd = llm_sd if llm_sd is not None else W.make_llm_state(cfg.llm, seed=seed, init=init)
        self._llm_kw = dict(dtype=llm_dtype, device=device, max_batch=max_batch, max_ctx=max_ctx)
        self.llm = HvxLLM(cfg.llm, llm_sd, sampling=sampling, inference_head_num=inference_head_num, **self._llm_kw)
        self._llms = [self.llm]
        del llm_sd
        flow_sd = flow_sd if flow_sd is not None else W.make_flow_state(cfg.flow, seed=seed + 1, init=init)
        self._flow_kw = dict(dtype=flow_dtype, device=device, max_t=max_t)
        self.flow = HvxFlow(cfg.flow, flow_sd, **self._flow_kw)
        del flow_sd
        hift_sd = hift_sd if hift_sd is not None else W.make_hift_state(cfg.hift, seed=seed + 2, init=init)
        self._hift_kw = dict(device=device, tables=hift_tables, exact_fp32=hift_exact_fp32)      # (exact_fp32: the reference's own fp32 vocoder arithmetic, hift.py)
        self.hift = HvxHift(cfg.hift, hift_sd, **self._hift_kw)
        self._acoustic = [(self.flow, self.hift)]
        # utterances of similar length that share one padded CFM solve (hvx_cfm_solve_batch): the DiT GEMMs and the attention reach their
        # large-grid rates from about 4 utterances (x CFG 2) per launch
        self.acoustic_batch = 4
        self.device = torch.device(device)

    @classmethod
    def from_models(cls, cfg: HvxConfig, llm, flow, hift, acoustic_batch=4):
        """a pipeline over model objects that already exist (the queue worker's `model_manager.models`): same engine, nothing re-loaded"""
        p = cls.__new__(cls)
        p.cfg, p.llm, p.flow, p.hift = cfg, llm, flow, hift
        p._llms, p._acoustic = [llm], [(flow, hift)]
        p._llm_kw = p._flow_kw = p._hift_kw = None
        p.acoustic_batch = acoustic_batch
        p.device = torch.device(llm.device)
        return p

    # ---- stages -----------------------------------------------------------------------------------------------------------------
    def _speech_tokens(self, utts, max_token_text_ratio, min_token_text_ratio, llm=None):
        return (llm or self.llm).generate_batch([u.text for u in utts],
                                       prompt_texts=[u.prompt_text for u in utts] if any(u.prompt_text is not None for u in utts) else None,
                                       prompt_speech_tokens=[u.prompt_speech_token for u in utts] if any(u.prompt_speech_token is not None for u in utts) else None,
                                       seeds=[u.seed for u in utts], max_token_text_ratio=max_token_text_ratio,
                                       min_token_text_ratio=min_token_text_ratio)

    def _mels(self, utts, toks, flow=None):
        dev = self.device
        flow = flow or self.flow
        mels = []
        for u, t in zip(utts, toks):
            if not t:
                mels.append(None)
                continue
            token = torch.tensor(t, dtype=torch.int32, device=dev)[None]
            kw = {}
            if _flow_prompt(u) is not None:
                kw = dict(prompt_token=_flow_prompt(u).to(dev)[None], prompt_token_len=torch.tensor([len(_flow_prompt(u))]),
                          prompt_feat=u.prompt_feat.to(dev)[None], prompt_feat_len=torch.tensor([u.prompt_feat.shape[0]]))
            mel, _ = flow.inference(token=token, token_len=torch.tensor([token.shape[1]], dtype=torch.int32), embedding=u.embedding[None].to(dev),
                                         finalize=True, **kw)
            mels.append(mel)
        return mels

    def _mels_batched(self, utts, toks, flow=None, max_pad=0.15, max_batch=None):
        """the same mels as _mels, solved in length buckets: utterances whose frame counts lie within `max_pad` of the longest of their
        bucket (at most `max_batch` of them) share one padded solve (hvx_cfm_solve_batch)"""
        flow = flow or self.flow
        dev = self.device
        mels = [None] * len(utts)
        def frames(i):
            return len(toks[i]) + (0 if _flow_prompt(utts[i]) is None else len(_flow_prompt(utts[i])))
        order = sorted((i for i in range(len(utts)) if toks[i]), key=lambda i: -frames(i))
        while order:
            top = frames(order[0])
            bucket = [i for i in order if frames(i) >= (1.0 - max_pad) * top][:max_batch]
            order = [i for i in order if i not in bucket]
            out = flow.inference_batch([torch.tensor(toks[i], dtype=torch.int32, device=dev) for i in bucket], [utts[i].embedding.to(dev) for i in bucket],
                                       prompt_tokens=[None if _flow_prompt(utts[i]) is None else _flow_prompt(utts[i]).to(dev) for i in bucket],
                                       prompt_feats=[None if utts[i].prompt_feat is None else utts[i].prompt_feat.to(dev) for i in bucket])
            for i, m in zip(bucket, out):
                mels[i] = m
        return mels

    def _waves(self, mels, hift=None, speeds=None):
        wavs = []
        hift = hift or self.hift
        for k, mel in enumerate(mels):
            if mel is None:
                wavs.append(torch.zeros(0, device=self.device))
                continue
            if speeds is not None and speeds[k] != 1.0:
                from .ops import resample_linear
                mel = resample_linear(mel, max(1, int(mel.shape[2] / speeds[k])))
            wav, _ = hift.inference(speech_feat=mel)
            wavs.append(wav[0])
        return wavs

    @torch.inference_mode()
    def synthesize(self, utts: List[Utterance], max_token_text_ratio=20, min_token_text_ratio=2):
        """-> (list of waveforms f32 [samples] on the device, SynthStats); the three stages run back to back"""
        st = SynthStats()
        torch.cuda.synchronize()
        t0 = time.time()
        toks = self._speech_tokens(utts, max_token_text_ratio, min_token_text_ratio)
        torch.cuda.synchronize()
        t1 = time.time()
        st.llm_seconds = t1 - t0
        st.llm = dict(self.llm.last_stats)
        st.per_utt_tokens = [len(t) for t in toks]
        st.token_ids = [list(t) for t in toks]
        st.tokens = sum(st.per_utt_tokens)
        mels = self._mels_batched(utts, toks, max_batch=self.acoustic_batch) if self.acoustic_batch > 1 else self._mels(utts, toks)
        torch.cuda.synchronize()
        t2 = time.time()
        st.flow_seconds = t2 - t1
        wavs = self._waves(mels)
        torch.cuda.synchronize()
        t3 = time.time()
        st.hift_seconds = t3 - t2
        st.total_seconds = t3 - t0
        st.audio_seconds = sum(w.numel() for w in wavs) / float(self.cfg.sample_rate)
        return wavs, st

    # ---- software pipeline over batches ------------------------------------------------------------------------------------------
    def _acoustic_chain(self, k):
        """k-th acoustic chain: (flow, vocoder) handles with their own workspaces over the same packed weights, and a stream"""
        while len(self._acoustic) <= k:
            if self._flow_kw is None:
                raise ValueError('a pipeline built with from_models() owns one acoustic chain (it does not know how its models were constructed)')
            flow = HvxFlow(self.cfg.flow, None, **self._flow_kw)
            flow.load_packed(self.flow._weights)
            hift = HvxHift(self.cfg.hift, None, **self._hift_kw)
            hift.load_packed(self.hift._weights)
            self._acoustic.append((flow, hift))
        while len(self._bg_streams) <= k:
            self._bg_streams.append(torch.cuda.Stream(device=self.device, priority=0))
        return self._acoustic[k] + (self._bg_streams[k],)

    def _acoustic_worker(self, utts, toks, st, k=0):
        """flow + vocoder of one batch on a background stream (runs in a worker thread; returns when the waveforms are complete)"""
        flow, hift, stream = self._acoustic_chain(k)
        torch.cuda.set_device(stream.device)                       # the current device is per thread
        with torch.inference_mode(), torch.cuda.stream(stream):
            t0 = time.time()
            mels = self._mels(utts, toks, flow)
            t1 = time.time()                       # enqueue time only: the stream is not drained between the stages
            wavs = self._waves(mels, hift)
            stream.synchronize()
            t2 = time.time()
        st.flow_seconds, st.hift_seconds = t1 - t0, t2 - t1
        st.audio_seconds = sum(w.numel() for w in wavs) / float(self.cfg.sample_rate)
        return wavs

    def _lm_chain(self, k):
        """k-th LM decode chain: a further native handle (own KV cache, workspace, stream, graphs) over the SAME packed weight tensors"""
        while len(self._llms) <= k:
            if self._llm_kw is None:
                raise ValueError('a pipeline built with from_models() owns one LM chain (it does not know how its models were constructed)')
            clone = HvxLLM(self.cfg.llm, None, **self._llm_kw)
            clone.load_packed(self.llm._weights)
            self._llms.append(clone)
        llm = self._llms[k]
        llm.sampling, llm.inference_head_num = self.llm.sampling, self.llm.inference_head_num       # per-request knobs live on self.llm
        return llm

    def _lm_worker(self, k, utts, max_token_text_ratio, min_token_text_ratio):
        torch.cuda.set_device(self._bg_stream.device)              # the current device is per thread
        with torch.inference_mode():
            st = SynthStats()
            llm = self._lm_chain(k)
            t0 = time.time()
            toks = self._speech_tokens(utts, max_token_text_ratio, min_token_text_ratio, llm=llm)
            st.llm_seconds = time.time() - t0
            st.llm = dict(llm.last_stats)
            st.per_utt_tokens = [len(t) for t in toks]
            st.token_ids = [list(t) for t in toks]
            st.tokens = sum(st.per_utt_tokens)
            return toks, st, t0

    def _acoustic_after(self, utts, lm_future, k=0):
        toks, st, t0 = lm_future.result()
        wavs = self._acoustic_worker(utts, toks, st, k)
        st.total_seconds = time.time() - t0
        return wavs, st

    @torch.inference_mode()
    def synthesize_continuous(self, utts, lm_slots=16, max_token_text_ratio=20, min_token_text_ratio=2, acoustic_batch=None, acoustic_min_batch=1, pace=None):
        """Generator over (index, waveform, tokens) in completion order — continuous batching end to end over a finite
        list of utterances; see `serve` (the same engine over an open-ended source).  Results equal synthesize(): every utterance carries
        its own sampler seed.  `self.last_continuous` holds the stage accounting of the run."""
        utts = list(utts)
        maxr = max_token_text_ratio if isinstance(max_token_text_ratio, (list, tuple)) else [max_token_text_ratio] * len(utts)
        minr = min_token_text_ratio if isinstance(min_token_text_ratio, (list, tuple)) else [min_token_text_ratio] * len(utts)
        for i, u in enumerate(utts):
            u.max_token_text_ratio, u.min_token_text_ratio = maxr[i], minr[i]
        max_out = max([int(len(u.text) * maxr[i]) for i, u in enumerate(utts)] + [1])
        max_prefix = max([2 + len(u.text) + (0 if u.prompt_text is None else len(u.prompt_text)) +
                          (0 if u.prompt_speech_token is None else len(u.prompt_speech_token)) for u in utts] + [1])
        index = {id(u): i for i, u in enumerate(utts)}

        class _List:
            def __init__(self):
                self.it = iter(utts)

            def poll(self, block):
                return next(self.it)
        for u, wav, toks in self.serve(_List(), lm_slots=lm_slots, acoustic_batch=acoustic_batch, acoustic_min_batch=acoustic_min_batch,
                                       max_out=max_out, max_prefix=max_prefix, pace=pace):
            if isinstance(wav, BaseException):
                raise wav
            yield index[id(u)], wav, toks

    @torch.inference_mode()
    def serve(self, source, lm_slots=16, acoustic_batch=None, acoustic_min_batch=1, max_out=None, max_prefix=None,
              max_token_text_ratio=20, min_token_text_ratio=2, pace=None, mixed_sampling=False, win_cap=None, mixed_heads=False, head_cap=None,
              stream=False, sync_every=None, event_log=None, incremental_vocoder=False, incremental_flow=False):
        """The continuous engine over an open-ended SOURCE of utterances: `source.poll(block)` returns the next `Utterance`, or None when
        nothing is waiting (it is asked to block only while the decode grid is idle), and raises StopIteration when closed.  Generator over
        (utterance, waveform | exception, tokens) in completion order.
        The LM decodes up to `lm_slots` utterances in ONE grid (HvxLLM.generate_stream: the weights are streamed once per step for all of
        them, a finished utterance's slot goes to the next waiting one), driven by a worker thread on the high-priority decode stream; every
        finished utterance goes straight to the flow decoder and the vocoder, which run here on a second stream beside the decode of the
        utterances still in flight, in padded solves of up to `acoustic_batch` utterances of similar length.  `acoustic_min_batch` > 1 trades
        latency for throughput: the acoustic stage then waits until that many finished utterances are queued (or the LM is idle / done).
        A request that cannot run (context budget) comes back as (utterance, exception, []) without disturbing the others.  If the consumer
        stops iterating, the LM thread is cancelled: it stops taking requests and abandons the decode of those in flight; every utterance that was
        fetched from the source and got no result is listed in `self.last_continuous['abandoned']`.  Source protocol: `poll(block)` as above and,
        optionally, `unpoll(utterance)` — an utterance fetched in the instant of a cancellation is handed back through it (the queue worker's
        sources implement it and re-serve the request); without `unpoll` it joins the abandoned list.
        `pace` = (first, every_steps, more): admission pacing of the decode grid (see _DecodeEngine.run).
        `mixed_sampling`: utterances may carry their own `sampling` and decode side by side with others' (HvxLLM.generate_stream; `win_cap` is
        the longest repetition window the grid holds).  Off, an utterance that carries `sampling` comes back with an error.
        `mixed_heads`: the same for `inference_head_num` (`head_cap`: rows per sequence of the grid, default the model's head_num).
        `stream`: audio leaves in PIECES while the utterances are still decoding — the reference's chunked synthesis (streaming.stream_tts) for every
        utterance of the grid at once.  The generator then yields (utterance, piece, info) for every piece of every utterance in the order the pieces
        become ready, interleaved across utterances; info = {'index': piece number from 0, 'final': bool} and, on the final piece, 'tokens': the
        utterance's token list.  Pieces of one utterance come in order and concatenate to its audio.  The LM hands over the ids of every slot after each
        host round trip (generate_stream(stream_tokens=True)), a `ChunkSchedule` per utterance says when a chunk is ready, and the ready chunks of different
        utterances — up to `acoustic_batch`, in the length buckets of the unstreamed path — share one chunk-masked solve over their token prefixes
        (HvxFlow.solve_stream_batch) that appends the new frames to each utterance's mel cache; the vocoder runs per utterance over its cache.  An
        utterance with speed != 1.0 comes back as (utterance, AssertionError, {}): the reference refuses it too.  `acoustic_min_batch` does not apply.
        The mel cache of an utterance holds `max_out` tokens when that is given, otherwise the utterance's own token budget (its text length x its
        `max_token_text_ratio`, or this call's).  self.last_continuous gains `pieces`, `chunk_solves`, `first_piece_seconds` ((n, seconds from the
        utterance's fetch to its first piece) of the latest 4096 utterances, n = fetch order) and `pieces_out` (pieces already handed out, per entry of
        `abandoned`).  `event_log`: a list (or anything with append) that receives the engine's log as it happens — ('tokens', n, count) / ('done', n)
        from the LM thread, ('piece', n, index, final) from this one; nothing is logged without it (a server's serve() call may live for days).
        `incremental_vocoder` (with `stream`; ValueError without): every utterance owns a vocoder stream (hift.HiftStream) sized like its mel cache plane and a
        piece is vocoded from a window of the cache — left context + new frames + look-ahead — instead of the whole cache; pieces, order, `index` and `final`
        are those of the switch-off path.  The stream is released with the plane (final piece, cancel, drop, abandoned).  `last_continuous['vocoder_frames']`:
        mel frames the vocoder decoded over the call, with the switch on or off.
        `incremental_flow` (with `stream`; ValueError without; independent of `incremental_vocoder`): every utterance owns a flow stream (flow.FlowStream) and a non-final
        chunk job solves only the rows from the last chunk boundary at or below the frames already handed out, against the cached keys and values of the rows below
        (HvxFlow.solve_incremental_batch); such jobs are bucketed by window length instead of prefix length.  Final jobs (full mask) are whole-prefix solves, as with the
        switch off.  The stream is released with the plane.  `last_continuous['flow_rows']`: rows the flow solved over the call, window or prefix, with the switch on or off.
        `sync_every`: decode steps per host round trip of the grid (default 8); smaller: tokens — and so pieces — surface at a finer cadence, for more
        round trips.
        Cancelling ONE utterance: `Utterance.cancel` (any object with is_set()) goes to the decode engine with the request (HvxLLM.generate_stream).  Unstreamed, a
        cancelled utterance comes back once as (utterance, Cancelled, ids so far) — also when it is cancelled between its last token and its solve.  Streamed, its
        chunk jobs not yet solved are dropped, its mel cache and state are released and it comes back once as (utterance, Cancelled, {}); pieces already handed
        out are not recalled.  `self.last_continuous['cancelled']` counts them (the key is there when some utterance of the run carried `cancel`); they are not `abandoned`."""
        acoustic_batch = acoustic_batch or self.acoustic_batch
        acoustic_min_batch = max(1, min(int(acoustic_min_batch), acoustic_batch))
        piecewise = bool(stream)                           # (`stream` names the acoustic stage's device stream below)
        if incremental_vocoder and not piecewise:
            raise ValueError('incremental_vocoder needs stream=True: an unstreamed utterance is vocoded once')
        if incremental_flow and not piecewise:
            raise ValueError('incremental_flow needs stream=True: an unstreamed utterance is solved once')
        import queue
        import threading
        if getattr(self, '_bg_stream', None) is None:
            lm_cus = int(getattr(self, 'lm_cus', 0) or 0)
            if self.device.type != 'cuda':
                self._bg_stream = _HostStream()
            elif lm_cus > 0:
                # CU partition (docs/history/DESIGN_rounds1-4.md §5.0): the decode engine on CUs [0, lm_cus), the acoustic stage on the rest — both ranges spread over all
                # 8 XCDs.  Must be set before the first decode engine of self.llm is built (the engine keeps its stream).
                from . import _lib
                n_cu = _lib.load().hvx_device_ok()
                self.llm.cu_range = (0, lm_cus)
                self._bg_stream = _lib.cu_range_stream(lm_cus, n_cu - lm_cus, device=self.device)
            elif int(getattr(self, 'acoustic_cus', 0) or 0) > 0:
                # the acoustic stage on the LAST `acoustic_cus` compute units only, the decode engine unconfined: its short launches always find
                # the reserved CUs free instead of waiting for a 200-900 us workgroup of the acoustic stage to retire
                from . import _lib
                n_cu = _lib.load().hvx_device_ok()
                self._bg_stream = _lib.cu_range_stream(n_cu - int(self.acoustic_cus), int(self.acoustic_cus), device=self.device)
            else:
                # (lm_cus_only: the decode engine alone is confined — to CUs [0, lm_cus_only) — and the acoustic stage may use every CU)
                if int(getattr(self, 'lm_cus_only', 0) or 0) > 0:
                    self.llm.cu_range = (0, int(self.lm_cus_only))
                self._bg_stream = torch.cuda.Stream(device=self.device, priority=0)
            self._bg_streams = [self._bg_stream]
            self._bg_pools = []
        flow, hift, stream = self._acoustic_chain(0)
        if self.device.type == 'cuda':
            torch.cuda.synchronize(self.device)           # (everything the handles were built from is complete before other streams use it)
        # bounded, but wide enough that a whole grid can finish at once without the decode engine waiting on this queue (it stalls inside its
        # `yield` while the LM thread is blocked in put): only a consumer that has fallen a full grid behind holds the LM back
        q_len = 2 * int(lm_slots) + 2 * acoustic_batch
        if piecewise:
            # ... which, streamed, also takes room for the token items: every slot puts one per block of `sync_every` steps (at least one id each), so
            # a whole grid's worth of them is lm_slots * max_out / sync_every; the items are short id lists
            q_len += int(lm_slots) * (-(-int(max_out or getattr(self.llm, 'max_ctx', 4096)) // int(sync_every or 8)))
        q = queue.Queue(maxsize=q_len)
        cancel = threading.Event()
        lm_info = {}
        seen = {}                                          # running id -> utterance in flight; an entry goes when its result is handed out
        n_seen = [0]
        abandoned = []                                     # fetched from a source without `unpoll` while the engine was being cancelled
        from collections import deque
        fetched = {}                                       # stream: running id -> (time of its fetch, tokens its mel cache must hold), until its session exists
        live = {}                                          # stream: running id -> _StreamUtterance, until its final piece has left
        acct = dict(pieces=0, chunk_solves=0, first=deque(maxlen=4096), acoustic=0.0, audio=0.0, tokens=0, cancelled=0, with_cancel=False, vocoder_frames=0,
                    incremental=bool(incremental_vocoder), incremental_flow=bool(incremental_flow), flow_rows=0)

        class _Requests:
            @staticmethod
            def poll(block):
                # The source is asked to block only while the decode grid is idle, and a well-behaved source blocks for a bounded time (returning
                # None): `cancel` is looked at again on every call, so a consumer that stopped — or an acoustic-stage failure — ends the LM thread
                # within that bound instead of when the next request happens to arrive.
                if cancel.is_set():
                    raise StopIteration
                while True:
                    u = source.poll(block)
                    if u is None:
                        return None
                    if cancel.is_set():                    # fetched while the engine was being cancelled: hand it back rather than fail it
                        if hasattr(source, 'unpoll'):
                            source.unpoll(u)
                        else:                              # (a source without `unpoll`: it is reported with the abandoned ones, never silently lost)
                            abandoned.append(u)
                        raise StopIteration
                    tag = n_seen[0]
                    n_seen[0] += 1
                    if getattr(u, 'cancel', None) is not None:
                        acct['with_cancel'] = True
                    seen[tag] = u
                    if piecewise and u.speed != 1.0:          # (cosyvoice/cli/model.py:425) answered at once, it never takes a slot
                        if not put((tag, AssertionError('speed change only support non-stream inference mode'), True)):
                            raise StopIteration
                        continue
                    break
                if piecewise:
                    budget = max_out if max_out is not None else int(len(u.text) * (max_token_text_ratio if u.max_token_text_ratio is None else u.max_token_text_ratio))
                    fetched[tag] = (time.time(), max(int(budget), 1))
                return dict(text=u.text, prompt_text=u.prompt_text, prompt_speech_token=u.prompt_speech_token, seed=u.seed, tag=tag, sampling=u.sampling,
                            inference_head_num=u.inference_head_num, **(dict(cancel=u.cancel) if getattr(u, 'cancel', None) is not None else {}),
                            max_token_text_ratio=max_token_text_ratio if u.max_token_text_ratio is None else u.max_token_text_ratio,
                            min_token_text_ratio=min_token_text_ratio if u.min_token_text_ratio is None else u.min_token_text_ratio)

        def put(item):
            while not cancel.is_set():
                try:
                    q.put(item, timeout=0.05)
                    return True
                except queue.Full:
                    pass
            return False

        def lm_thread():
            try:
                if self.device.type == 'cuda':
                    torch.cuda.set_device(stream.device)           # the current device is per thread
                with torch.inference_mode():
                    t0 = time.time()
                    gen = self.llm.generate_stream(_Requests(), n_slots=lm_slots, max_out=max_out, max_prefix=max_prefix, pace=pace,
                                                   **(dict(mixed_sampling=True, win_cap=win_cap) if mixed_sampling else {}),
                                                   **(dict(mixed_heads=True, head_cap=head_cap) if mixed_heads else {}),
                                                   **(dict(stream_tokens=True) if piecewise else {}), **(dict(sync_every=sync_every) if sync_every else {}))
                    try:
                        for item in gen:
                            if piecewise and event_log is not None:
                                event_log.append(('done', item[0]) if item[2] else ('tokens', item[0], len(item[1])))
                            if not put(item):
                                break
                    finally:
                        gen.close()
                    lm_info.update(seconds=time.time() - t0, stats=dict(self.llm.last_stats))
                put(None)
            except BaseException as e:                              # surfaces in the consuming thread
                put(e)

        th = threading.Thread(target=lm_thread, name='hvx-lm', daemon=True)
        t_begin = time.time()
        th.start()
        acoustic = audio = 0.0
        tokens = 0
        try:
            if piecewise:
                yield from self._stream_consumer(q, seen, fetched, live, flow, hift, stream, acoustic_batch, acct, event_log)
            while not piecewise:
                item = q.get()
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise item
                # whatever else has finished meanwhile joins this acoustic batch (up to `acoustic_batch` utterances, solved in length buckets)
                group, tail, ended = [item], None, False
                while len(group) < acoustic_batch:
                    try:
                        nxt = q.get() if len(group) < acoustic_min_batch else q.get_nowait()     # (a throughput job waits for its minimum batch or the end)
                    except queue.Empty:
                        break
                    if nxt is None or isinstance(nxt, BaseException):
                        tail, ended = nxt, True                    # (the sentinel / error is handled after this batch)
                        break
                    group.append(nxt)
                # (cancelled between its last token and its solve: it never reaches the acoustic stage)
                group = [(i, Cancelled(t) if not isinstance(t, BaseException) and _cancelled(seen[i]) else t) for i, t in group]
                bad = [(i, t) for i, t in group if isinstance(t, BaseException) or not t]
                group = [(i, t) for i, t in group if not isinstance(t, BaseException) and t]
                for i, t in bad:
                    if isinstance(t, Cancelled):
                        acct['cancelled'] += 1
                        yield seen.pop(i), t, list(t.tokens)
                        continue
                    yield seen.pop(i), (t if isinstance(t, BaseException) else torch.zeros(0, device=self.device)), []
                if group:
                    us = [seen[i] for i, _ in group]
                    t0 = time.time()
                    with _on(stream):
                        wavs = self._waves(self._mels_batched(us, [t for _, t in group], flow, max_batch=acoustic_batch), hift, speeds=[u.speed for u in us])
                        stream.synchronize()
                    acoustic += time.time() - t0
                    for (i, toks), wav in zip(group, wavs):
                        audio += wav.numel() / float(self.cfg.sample_rate)
                        tokens += len(toks)
                        yield seen.pop(i), wav, toks
                if ended:
                    if isinstance(tail, BaseException):
                        raise tail
                    break
        finally:
            cancel.set()
            while th.is_alive():                                   # (keep the queue moving so that a blocked put sees the cancellation)
                try:
                    q.get_nowait()
                except queue.Empty:
                    pass
                th.join(timeout=0.05)
            self.last_continuous = dict(tokens=tokens, audio_seconds=audio, acoustic_seconds=acoustic, total_seconds=time.time() - t_begin,
                                        llm_seconds=lm_info.get('seconds', 0.0), llm=lm_info.get('stats', {}), lm_slots=lm_slots,
                                        abandoned=abandoned + list(seen.values()))
            if acct['with_cancel']:                                # (a run in which no utterance carried `cancel` reports what it always reported)
                self.last_continuous['cancelled'] = acct['cancelled']
            if piecewise:
                for se in live.values():                            # (utterances the run leaves behind: abandoned, or cut off by an error)
                    se.release()
                self.last_continuous.update(tokens=acct['tokens'], audio_seconds=acct['audio'], acoustic_seconds=acct['acoustic'], pieces=acct['pieces'],
                                            chunk_solves=acct['chunk_solves'], first_piece_seconds=list(acct['first']), vocoder_frames=acct['vocoder_frames'], flow_rows=acct['flow_rows'],
                                            pieces_out=[0] * len(abandoned) + [live[k].pieces if k in live else 0 for k in seen])

    def _stream_consumer(self, q, seen, fetched, live, flow, hift, stream, acoustic_batch, acct, event_log, max_pad=0.15):
        """the acoustic stage of serve(stream=True): generator over (utterance, piece | exception, info).  Queue items are generate_stream(stream_tokens=True)'s:
        (n, new ids, False) and (n, token list | exception, True), None when the LM is done.  `live`: n -> _StreamUtterance (serve reads it when it ends)."""
        import queue
        hop = flow.static_chunk_size // flow.token_mel_ratio        # "must matching training static_chunk_size" (cosyvoice/cli/model.py:395-396)
        ratio = flow.token_mel_ratio
        order = []                                                 # n of every job that is ready, oldest first
        ended = False

        def session(n):
            if n not in live:
                t_fetch, budget = fetched.pop(n)
                with _on(stream):                                  # (its copies to the device are ordered with the solves that read them)
                    live[n] = _StreamUtterance(seen[n], flow, hop, budget, self.device, t_fetch, hift=hift if acct['incremental'] else None,
                                               **(dict(incremental_flow=True) if acct['incremental_flow'] else {}))
            return live[n]

        def drop(n):
            """utterance n leaves without (further) pieces: its session, its bookkeeping and whatever of it was scheduled"""
            se = live.pop(n, None)
            if se is not None:
                se.release()
            fetched.pop(n, None)
            order[:] = [m for m in order if m != n]

        def log(*ev):
            if event_log is not None:
                event_log.append(ev)
        while True:
            # ---- everything the LM has handed over so far; wait only when no chunk is ready
            while not ended:
                try:
                    item = q.get_nowait() if order else q.get()
                except queue.Empty:
                    break
                if item is None:
                    ended = True
                    break
                if isinstance(item, BaseException):
                    raise item
                n, ids, done = item
                if n in live and live[n].dead:                     # retired here already: the LM's last word on it is all that is waited for
                    if done:
                        drop(n)
                        acct['cancelled'] += 1
                        yield seen.pop(n), ids if isinstance(ids, Cancelled) else Cancelled(ids if not isinstance(ids, BaseException) else ()), {}
                elif not done:
                    se = session(n)
                    for k, covered in se.sched.feed(ids):
                        se.jobs.append((k, covered, False))
                        order.append(n)
                elif isinstance(ids, BaseException):
                    drop(n)
                    acct['cancelled'] += isinstance(ids, Cancelled)
                    yield seen.pop(n), ids, {}
                elif not ids:                                      # nothing was generated: one empty, final piece
                    drop(n)
                    log('piece', n, 0, True)
                    acct['pieces'] += 1
                    yield seen.pop(n), torch.zeros(0, device=self.device), dict(index=0, final=True, tokens=[])
                else:
                    se = session(n)
                    for k, covered in se.sched.feed(ids[len(se.sched.tokens):]):      # (every id has come as an increment already; an LM that sends none is served too)
                        se.jobs.append((k, covered, False))
                        order.append(n)
                    k, covered = se.sched.finish()
                    se.tokens = list(ids)
                    se.jobs.append((k, covered, True))
                    order.append(n)
            # ---- utterances cancelled by their caller: their jobs go; one the LM has finished leaves here, the others when the LM hands them back
            for n, se in list(live.items()):
                if se.dead or not _cancelled(se.u):
                    continue
                se.dead, se.jobs = True, []
                order[:] = [m for m in order if m != n]
                if se.tokens is not None:
                    drop(n)
                    acct['cancelled'] += 1
                    yield seen.pop(n), Cancelled(se.tokens), {}
            if not order:
                if ended:
                    return
                continue
            # ---- one job each of up to `acoustic_batch` utterances, oldest first (the jobs of ONE utterance follow each other: each appends to its cache)
            picked, rest = [], []
            for n in order:
                if len(picked) < acoustic_batch and n not in picked:
                    picked.append(n)
                else:
                    rest.append(n)
            order = rest
            jobs = {n: live[n].jobs.pop(0) for n in picked}
            t0 = time.time()
            out = []
            with _on(stream):
                for final in (False, True):                        # a final job runs with the full mask: its own solves
                    windowed = acct['incremental_flow'] and not final       # non-final jobs solve windows: bucketed by window length instead of prefix length
                    size = (lambda n: live[n].window_rows(flow, jobs[n][0], jobs[n][1])) if windowed else (lambda n: live[n].n_prompt + jobs[n][0])
                    todo = sorted((n for n in picked if jobs[n][2] == final), key=lambda n: -size(n))
                    while todo:
                        top = size(todo[0])
                        bucket = [n for n in todo if size(n) >= (1.0 - max_pad) * top]
                        todo = [n for n in todo if n not in bucket]
                        ins = [live[n].flow_inputs(flow, jobs[n][0], final) for n in bucket]
                        if windowed:
                            acct['flow_rows'] += sum(size(n) for n in bucket)
                            fresh = flow.solve_incremental_batch([live[n].fstream for n in bucket], [i[0] for i in ins], [i[1] for i in ins], [i[2] for i in ins],
                                                                 [live[n].prompt_frames + jobs[n][1] * ratio for n in bucket], [live[n].cache for n in bucket],
                                                                 [live[n].fill for n in bucket])
                        else:
                            acct['flow_rows'] += sum(int(i[0].shape[-1]) for i in ins)
                            fresh = flow.solve_stream_batch([i[0] for i in ins], [i[1] for i in ins], [i[2] for i in ins],
                                                            [live[n].prompt_frames + jobs[n][1] * ratio for n in bucket], [live[n].cache for n in bucket],
                                                            [live[n].fill for n in bucket], streaming=not final)
                        acct['chunk_solves'] += 1
                        for n, f in zip(bucket, fresh):
                            se = live[n]
                            se.fill += f
                            if se.vstream is not None:
                                before = se.vstream.frames_vocoded
                                piece = se.vstream.piece(se.cache, se.fill, final)[0]
                                acct['vocoder_frames'] += se.vstream.frames_vocoded - before
                            else:
                                wav, _ = hift.inference(speech_feat=se.cache[None, :, :se.fill], finalize=final)
                                piece = wav[0, se.handed:]
                                acct['vocoder_frames'] += se.fill
                            se.handed += piece.numel()
                            out.append((n, piece, final))
                stream.synchronize()
            acct['acoustic'] += time.time() - t0
            for n, piece, final in sorted(out, key=lambda o: picked.index(o[0])):
                se = live[n]
                info = dict(index=se.pieces, final=final)
                if se.pieces == 0:
                    acct['first'].append((n, time.time() - se.t_fetch))
                se.pieces += 1
                acct['pieces'] += 1
                acct['audio'] += piece.numel() / float(self.cfg.sample_rate)
                log('piece', n, info['index'], final)
                if final:
                    info['tokens'] = se.tokens
                    acct['tokens'] += len(se.tokens)
                    se.release()
                    del live[n]
                    u = seen.pop(n)
                else:
                    u = seen[n]
                yield u, piece, info

    @torch.inference_mode()
    def synthesize_pipelined(self, batches, max_token_text_ratio=20, min_token_text_ratio=2, lm_chains=3, acoustic_chains=1):
        """Generator over (waveforms, SynthStats) of successive batches, in order, with the stages of neighbouring batches overlapped.
        The multi-head LM decode is a chain of ~160 short dependent launches per step that leaves most of the GPU idle, so (a) the flow
        decoder and the vocoder of batch i (MFMA-bound) run on a second, lower-priority stream driven by a worker thread while later
        batches decode, and (b) `lm_chains` batches decode at the same time, each on its own native handle (KV cache, workspace, stream,
        graphs) over the same weight tensors and driven by its own host thread: two chains fill each other's launch gaps and together
        emit 1.63x the tokens of one (tools/two_chain_probe.py); with three the acoustic stage is the bottleneck of the bench workload.
        `acoustic_chains` > 1 runs flow + vocoder of several batches at once, each chain with its own handles, workspaces and stream (both
        stages are throughput-bound, so this buys little; it is supported and bit-identical to the serial path — the wrong waveforms it
        returned now and then in round 2 were packed-fp32 VALU instructions disturbed by another queue's MFMA stream, see build.py).
        At most max(lm_chains, acoustic_chains) + 1 batches are in flight.  Results are identical
        to synthesize(): every utterance carries its own sampler seed and no stage depends on another batch.  In the stats llm_seconds
        is the decode wall time of the batch and flow_seconds + hift_seconds the wall time of its acoustic stages, all while overlapped."""
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor
        if getattr(self, '_bg_stream', None) is None:
            self._bg_stream = torch.cuda.Stream(device=self.device, priority=0)
            self._bg_streams = [self._bg_stream]
            self._bg_pools = []
        lm_chains, acoustic_chains = max(1, int(lm_chains)), max(1, int(acoustic_chains))
        while len(self._bg_pools) < acoustic_chains:
            self._bg_pools.append(ThreadPoolExecutor(max_workers=1, thread_name_prefix='hvx-acoustic%d' % len(self._bg_pools)))
        for k in range(acoustic_chains):
            self._acoustic_chain(k)
        pools = getattr(self, '_lm_pools', [])
        while len(pools) < lm_chains:                     # one single-thread pool per chain: a handle is never used by two threads
            pools.append(ThreadPoolExecutor(max_workers=1, thread_name_prefix='hvx-lm%d' % len(pools)))
        self._lm_pools = pools
        for k in range(lm_chains):
            self._lm_chain(k)                             # build the handles on this thread, before the clock of the first job
        # the handles' tables and workspaces were produced by torch ops on THIS thread's stream; the worker threads use them on other
        # streams: without this barrier a worker can read a noise / rotary table that is still being written (seen as a rare wrong waveform)
        torch.cuda.synchronize(self.device)
        window = deque()
        for idx, utts in enumerate(batches):
            k = idx % lm_chains
            lm_f = pools[k].submit(self._lm_worker, k, utts, max_token_text_ratio, min_token_text_ratio)
            ka = idx % acoustic_chains
            window.append(self._bg_pools[ka].submit(self._acoustic_after, utts, lm_f, ka))      # FIFO per chain, results taken in batch order
            while len(window) > max(lm_chains, acoustic_chains):
                yield window.popleft().result()
        while window:
            yield window.popleft().result()
