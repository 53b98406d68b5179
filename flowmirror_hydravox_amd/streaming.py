"""Chunked (streaming) synthesis on top of the three HIP models — SURVEY.md §8(f) N3.

Host-side mirror of `CosyVoice3Model.token2wav` and the `stream=True` branch of `CosyVoice2Model.tts`
(server/model_utils/cosyvoice/cli/model.py:405-430, 316-352): speech tokens arrive from the LM one at a time, every
`token_hop_len` of them (plus `pre_lookahead_len` of look-ahead) the whole prefix is pushed through the flow with the static
chunk mask (`streaming=True`, dit.py:163-164) and `finalize=False`, the new mel frames are appended to the session's mel cache,
HiFT runs over the cached mel with `finalize=False` and only the samples past `speech_offset` are handed out.  All arithmetic is in
libhvx (flow.py / hift.py); this file is bookkeeping only, so it is covered on CPU with stand-in models as well as on the GPU.
"""
import math

import torch


class StreamSession:
    """One utterance being synthesised chunk by chunk.  What the reference keeps in `hift_cache_dict[uuid] = {'mel', 'speech_offset'}`
    (cli/model.py:405-430) lives here as two facts about the session: the mel frames produced so far and how many samples have already
    been handed to the caller.  Every push = flow over the token prefix -> keep only the frames past the prefix already covered ->
    vocode ALL frames so far -> return the samples not yet handed out."""

    def __init__(self, flow, hift, prompt_token, prompt_feat, embedding, device=None, incremental_vocoder=False, max_frames=None, incremental_flow=False):
        """incremental_vocoder: the session owns a vocoder stream (`hift.stream(max_frames)`, hift.HiftStream) and every push vocodes a window of the
        cached mel — left context + new frames + look-ahead — instead of all of it; the samples are those of the whole-cache pass.  max_frames:
        the longest utterance the stream holds (default: what the vocoder's fixed noise table covers, `hift.max_stream_frames`).  The stream is
        released with the final push (or close()).
        incremental_flow: the session owns a flow stream (`flow.stream(max_frames)`, flow.FlowStream — here max_frames counts the prompt's frames too and defaults to
        the flow's max_t) and every non-final push solves only the rows from the last chunk boundary at or below the frames already handed out, against the cached keys
        and values of the rows below (HvxFlow.solve_incremental_batch); the final push — full mask — stays a whole-prefix solve.  `flow_rows` counts the rows solved,
        with the switch on or off."""
        self.flow, self.hift = flow, hift
        self._fstream = flow.stream(int(max_frames) if max_frames is not None else flow.max_t) if incremental_flow else None
        self.flow_rows = 0
        self._vstream = hift.stream(int(max_frames) if max_frames is not None else hift.max_stream_frames) if incremental_vocoder else None
        self.device = device if device is not None else getattr(flow, 'device', 'cpu')
        self.embedding = embedding.to(self.device)
        prompt_token, prompt_feat = prompt_token.to(self.device), prompt_feat.to(self.device)
        # the prompt never changes during an utterance: its flow arguments are fixed here
        self._prompt = {}
        if prompt_token.shape[1] > 0:
            self._prompt = dict(prompt_token=prompt_token, prompt_token_len=torch.tensor([prompt_token.shape[1]], dtype=torch.int32),
                                prompt_feat=prompt_feat, prompt_feat_len=torch.tensor([prompt_feat.shape[1]], dtype=torch.int32))
        self._frames = None            # (1, mel, n) every mel frame of the utterance so far
        self._handed = 0               # samples already returned

    def _fresh_frames(self, token, covered, stream, finalize):
        """mel frames of the tokens past the first `covered` ones (the flow re-runs over the whole prefix, as the reference does)"""
        ratio = self.flow.token_mel_ratio
        n_prompt = self._prompt['prompt_token'].shape[1] if self._prompt else 0
        if self._fstream is not None and stream and not finalize:
            tok = token.to(self.device, dtype=torch.int32).reshape(-1)
            prompt_frames = 0
            if self._prompt:
                tok = torch.concat([self._prompt['prompt_token'].reshape(-1).to(torch.int32), tok])
                prompt_frames = int(self._prompt['prompt_feat'].shape[1])
            mu, spk = self.flow.encode(tok, self.embedding.reshape(-1), finalize=False)
            T = int(mu.shape[-1])
            cond = torch.zeros(mu.shape[0], T, dtype=torch.float32, device=mu.device)
            if prompt_frames:
                cond[:, :prompt_frames] = self._prompt['prompt_feat'][0].to(mu.device, torch.float32).t()
            done = prompt_frames + covered * ratio
            plane = torch.empty(mu.shape[0], T - done, dtype=torch.float32, device=mu.device)
            before = self._fstream.rows_solved
            self.flow.solve_incremental_batch([self._fstream], [mu], [spk], [cond], [done], [plane], [0])
            self.flow_rows += self._fstream.rows_solved - before
            return plane.unsqueeze(0)
        mel, _ = self.flow.inference(token=token.to(self.device, dtype=torch.int32), token_len=torch.tensor([token.shape[1]], dtype=torch.int32),
                                     embedding=self.embedding, streaming=stream, finalize=finalize, **self._prompt)
        self.flow_rows += ratio * (n_prompt + int(token.shape[1]) - (0 if finalize else self.flow.pre_lookahead_len))
        return mel[:, :, covered * ratio:]

    def _unheard(self, wav):
        out = wav[:, self._handed:]
        self._handed += out.shape[1]
        return out

    def push(self, token, covered, stream=False, finalize=False, speed=1.0):
        """token (1, n): all speech tokens generated so far (plus the look-ahead when not final); `covered`: how many of them earlier
        pushes already turned into frames -> the new samples (1, L)."""
        fresh = self._fresh_frames(token, covered, stream, finalize)
        self._frames = fresh if self._frames is None else torch.concat([self._frames, fresh], dim=2)
        mel = self._frames
        if speed != 1.0:
            if covered != 0 or not finalize:
                raise AssertionError('speed change only support non-stream inference mode')      # cli/model.py:425
            from .ops import resample_linear                                                      # F.interpolate(mode='linear') in libhvx
            mel = resample_linear(mel, int(mel.shape[2] / speed))
        if self._vstream is not None and speed == 1.0:
            out = self._vstream.piece(mel, mel.shape[2], finalize)
            self._handed += out.shape[1]
            if finalize:
                self.close()
            return out
        wav, _ = self.hift.inference(speech_feat=mel, finalize=finalize)
        if finalize and self._fstream is not None:          # (the flow stream goes with the utterance's last piece)
            self._fstream.release()
            self._fstream = None
        return self._unheard(wav)

    def close(self):
        """release the vocoder and flow streams (the final push does it; a session that is abandoned earlier calls this)"""
        if self._vstream is not None:
            self._vstream.close()
            self._vstream = None
        if self._fstream is not None:
            self._fstream.release()
            self._fstream = None

    # the reference's name and argument order (cli/model.py:405)
    def token2wav(self, token, token_offset, stream=False, finalize=False, speed=1.0):
        return self.push(token, token_offset, stream=stream, finalize=finalize, speed=speed)


class ChunkSchedule:
    """The chunk schedule of the reference's `tts(stream=True)` (cli/model.py:329-352) as host state of one utterance: which token prefixes go through the
    flow, and how many of their tokens earlier passes already covered.  A job is `(n_tokens_in_piece, covered)`: the flow runs over the first
    `n_tokens_in_piece` generated tokens (the last `pre_lookahead_len` of them are look-ahead only) and the frames past `covered` tokens are new.
    The first hop is padded so that prompt + hop is a whole number of `token_hop_len` chunks (`prompt_token_pad`), a job is ready as soon as
    hop + look-ahead unseen tokens are buffered, and `finish()` gives the last job: every token, full mask, `finalize=True`."""

    def __init__(self, n_prompt_tokens, token_hop_len, pre_lookahead_len):
        self.hop_len, self.look = int(token_hop_len), int(pre_lookahead_len)
        self.prompt_token_pad = int(math.ceil(n_prompt_tokens / self.hop_len) * self.hop_len - n_prompt_tokens)
        self.tokens = []
        self.covered = 0                 # the reference's token_offset
        self.finished = False

    def _hop(self):
        return self.hop_len + self.prompt_token_pad if self.covered == 0 else self.hop_len

    def feed(self, ids):
        """more generated ids (any number, also none) -> the jobs that became ready, in order"""
        assert not self.finished
        jobs = []
        for t in ids:
            self.tokens.append(int(t))
            hop = self._hop()                                    # (looked at after every token, as the reference's loop does: at most one job per token)
            if len(self.tokens) - self.covered >= hop + self.look:
                jobs.append((self.covered + hop + self.look, self.covered))
                self.covered += hop
        return jobs

    def finish(self):
        """the LM has stopped: the job of the final pass (whatever remains, full attention mask, finalize=True)"""
        self.finished = True
        return len(self.tokens), self.covered


def stream_tts(token_source, flow, hift, prompt_token, prompt_feat, embedding, token_hop_len=25, stream=True, speed=1.0, incremental_vocoder=False,
               incremental_flow=False):
    """Generator of waveform pieces (1, L) float32 from an iterable of speech-token ids (e.g. `HvxLLM.inference(...)`).

    The chunk schedule is the reference's (cli/model.py:329-352), kept in `ChunkSchedule`: the first hop is padded so that prompt + hop is a whole number
    of `token_hop_len` chunks (`prompt_token_pad`), a chunk is synthesised as soon as `hop + pre_lookahead_len` unseen tokens are
    buffered, and whatever remains when the LM stops goes through once more with `finalize=True`.  `token_hop_len` must be
    `static_chunk_size / token_mel_ratio` ("must matching training static_chunk_size", cli/model.py:395-396).
    incremental_vocoder: every piece is vocoded from a window of the mel cache and the session's vocoder stream (StreamSession); same pieces.  It
    needs stream=True (ValueError otherwise: an unstreamed utterance is vocoded once).
    incremental_flow: every non-final piece's flow solves a window against the session's flow stream (StreamSession) instead of the whole prefix.  Independent of
    incremental_vocoder; needs stream=True too (ValueError otherwise: an unstreamed utterance is solved once).
    """
    if incremental_vocoder and not stream:
        raise ValueError('incremental_vocoder needs stream=True: an unstreamed utterance is vocoded once')
    if incremental_flow and not stream:
        raise ValueError('incremental_flow needs stream=True: an unstreamed utterance is solved once')
    sess = StreamSession(flow, hift, prompt_token, prompt_feat, embedding, incremental_vocoder=incremental_vocoder, incremental_flow=incremental_flow)
    try:
        yield from _stream_tts(sess, token_source, flow, prompt_token, token_hop_len, stream, speed)
    finally:
        sess.close()                                 # (a consumer that stops early leaves no vocoder stream behind)


def _stream_tts(sess, token_source, flow, prompt_token, token_hop_len, stream, speed):
    if not stream:
        tokens = [int(t) for t in token_source]
        yield sess.token2wav(torch.tensor(tokens, dtype=torch.int32).unsqueeze(0), 0, stream=False, finalize=True, speed=speed)
        return
    sched = ChunkSchedule(prompt_token.shape[1], token_hop_len, flow.pre_lookahead_len)
    for t in token_source:
        for n, covered in sched.feed([t]):
            yield sess.token2wav(torch.tensor(sched.tokens[:n], dtype=torch.int32).unsqueeze(0), covered, stream=True, finalize=False)
    # the reference's last call leaves `stream` at its default False (cli/model.py:355-361): the final pass uses the full attention mask
    n, covered = sched.finish()
    yield sess.token2wav(torch.tensor(sched.tokens[:n], dtype=torch.int32).unsqueeze(0), covered, stream=False, finalize=True)
