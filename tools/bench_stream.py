#!/usr/bin/env python3
"""Streaming synthesis timing: one utterance, tokens from HvxLLM.inference fed to streaming.stream_tts.
Prints time to first audio and the arrival time / length of every piece; full-size CosyVoice3 dimensions, seeded random weights.

    python tools/bench_stream.py [--chars 128] [--heads 2]
    python tools/bench_stream.py --serve 8 --slots 8 [--chars 128]     # N concurrent streamed requests through HvxPipeline.serve(stream=True): first-audio
                                                                       # time and piece inter-arrival per request, and the tokens/s of the same requests
                                                                       # with stream=False (what streaming costs under load)
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def serve_bench(a):
    from functools import partial
    from flowmirror_hydravox_amd import cv3_config, tiny_config
    from flowmirror_hydravox_amd.pipeline import HvxPipeline, synthetic_utterance
    from flowmirror_hydravox_amd.sampling import ras_sampling
    cfg = tiny_config() if a.tiny else cv3_config()
    ratio = 5.5
    n_spk = int(a.chars * ratio)
    pipe = HvxPipeline(cfg, max_batch=a.slots, max_ctx=2 + a.chars + 20 + a.prompt + n_spk + 64, max_t=2 * (n_spk + a.prompt) + 64, seed=1986,
                       sampling=partial(ras_sampling, top_p=0.9, top_k=10, win_size=32, tau_r=0.2), inference_head_num=a.heads)
    utts = [synthetic_utterance(cfg, i, a.chars, n_prompt_speech=a.prompt, n_prompt_text=20) for i in range(a.serve)]
    for u in utts:
        u.max_token_text_ratio = u.min_token_text_ratio = ratio

    class Src:
        def __init__(self):
            self.it = iter(utts)

        def poll(self, block):
            return next(self.it)
    kw = dict(lm_slots=a.slots, max_out=n_spk, max_prefix=2 + a.chars + 20 + a.prompt, **(dict(sync_every=a.sync_every) if a.sync_every else {}))
    for rep in range(2):                                        # first pass warms up (graph capture, workspaces)
        torch.cuda.synchronize()
        t0 = time.time()
        arr = {}
        for u, piece, info in pipe.serve(Src(), stream=True, **kw):
            if isinstance(piece, BaseException):
                raise piece
            piece = piece.cpu()
            arr.setdefault(u.seed, []).append((time.time() - t0, piece.numel() / cfg.sample_rate))
        t_stream = time.time() - t0
        lc = dict(pipe.last_continuous)
        torch.cuda.synchronize()
        t0 = time.time()
        for u, wav, toks in pipe.serve(Src(), **kw):
            if isinstance(wav, BaseException):
                raise wav
            wav.cpu()
        t_plain = time.time() - t0
        plain = dict(pipe.last_continuous)
        if rep == 0:
            continue
        first = sorted(v[0][0] for v in arr.values())
        gaps = sorted(b[0] - a_[0] for v in arr.values() for a_, b in zip(v, v[1:]))
        late = sum(1 for v in arr.values() for i in range(1, len(v)) if v[i][0] > v[0][0] + sum(x[1] for x in v[:i]))
        print('serve: %d requests of %d tokens in %d slots, %d pieces in %d chunk solves' % (a.serve, n_spk, a.slots, lc['pieces'], lc['chunk_solves']))
        print('  first audio after: min %.3f  median %.3f  max %.3f s   (from the fetch, per request: %s)'
              % (first[0], first[len(first) // 2], first[-1], ' '.join('%.3f' % s for _, s in sorted(lc['first_piece_seconds']))))
        if gaps:
            print('  piece inter-arrival: median %.3f  max %.3f s; pieces that arrive after the audio before them finished playing: %d' % (gaps[len(gaps) // 2], gaps[-1], late))
        print('  streamed:   %d tokens in %.3f s = %.0f tokens/s (all audio delivered)' % (lc['tokens'], t_stream, lc['tokens'] / t_stream))
        print('  unstreamed: %d tokens in %.3f s = %.0f tokens/s (all audio delivered); streamed / unstreamed = %.3f'
              % (plain['tokens'], t_plain, plain['tokens'] / t_plain, (lc['tokens'] / t_stream) / (plain['tokens'] / t_plain)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chars', type=int, default=128)
    ap.add_argument('--heads', type=int, default=2)
    ap.add_argument('--prompt', type=int, default=75, help='prompt speech tokens (3 s)')
    ap.add_argument('--tiny', action='store_true')
    ap.add_argument('--serve', type=int, default=0, help='N concurrent requests through the continuous-batching server, streamed and unstreamed')
    ap.add_argument('--slots', type=int, default=8, help='decode-grid slots of --serve')
    ap.add_argument('--sync-every', type=int, default=None, help='decode steps per host round trip of --serve (default 8)')
    a = ap.parse_args()
    if a.serve:
        return serve_bench(a)
    from functools import partial
    from flowmirror_hydravox_amd import cv3_config, tiny_config
    from flowmirror_hydravox_amd.pipeline import HvxPipeline, synthetic_utterance
    from flowmirror_hydravox_amd.sampling import ras_sampling
    from flowmirror_hydravox_amd.streaming import stream_tts
    cfg = tiny_config() if a.tiny else cv3_config()
    ratio = 5.5
    n_spk = int(a.chars * ratio)
    pipe = HvxPipeline(cfg, max_batch=1, max_ctx=2 + a.chars + 20 + a.prompt + n_spk + 64, max_t=2 * (n_spk + a.prompt) + 64, seed=1986,
                       sampling=partial(ras_sampling, top_p=0.9, top_k=10, win_size=32, tau_r=0.2), inference_head_num=a.heads)
    u = synthetic_utterance(cfg, 0, a.chars, n_prompt_speech=a.prompt, n_prompt_text=20)

    def tokens():
        return pipe.llm.inference(text=u.text[None], text_len=torch.tensor([a.chars], dtype=torch.int32), prompt_text=u.prompt_text[None],
                                  prompt_text_len=torch.tensor([20], dtype=torch.int32), prompt_speech_token=u.prompt_speech_token[None],
                                  prompt_speech_token_len=torch.tensor([a.prompt], dtype=torch.int32), embedding=u.embedding[None],
                                  max_token_text_ratio=ratio, min_token_text_ratio=ratio, seed=0)

    for rep in range(2):                                        # first pass warms up (graph capture, workspaces)
        for stream in (True, False):
            torch.cuda.synchronize()
            t0 = time.time()
            arr = []
            for wav in stream_tts(tokens(), pipe.flow, pipe.hift, u.prompt_speech_token[None], u.prompt_feat[None], u.embedding[None],
                                  token_hop_len=cfg.flow.static_chunk_size // cfg.flow.token_mel_ratio, stream=stream):
                wav = wav.cpu()
                arr.append((time.time() - t0, wav.shape[1] / cfg.sample_rate))
            if rep == 0:
                continue
            audio = sum(x[1] for x in arr)
            print('%s: %d pieces, first audio after %.3f s (%.2f s of audio), all %.2f s of audio after %.3f s (RTF %.4f)'
                  % ('stream   ' if stream else 'one piece', len(arr), arr[0][0], arr[0][1], audio, arr[-1][0], arr[-1][0] / audio))
            if stream:
                print('  piece arrival [s]: ' + ' '.join('%.2f' % x[0] for x in arr))
                late = [i for i in range(1, len(arr)) if arr[i][0] > arr[0][0] + sum(x[1] for x in arr[:i])]
                print('  pieces that would arrive after the audio before them finished playing: %d' % len(late))


if __name__ == '__main__':
    main()
