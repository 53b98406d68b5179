#!/usr/bin/env python3
"""Streaming synthesis timing: one utterance, tokens from HvxLLM.inference fed to streaming.stream_tts.
Prints time to first audio and the arrival time / length of every piece; full-size CosyVoice3 dimensions, seeded random weights.

    python tools/bench_stream.py [--chars 128] [--heads 2]
    python tools/bench_stream.py --serve 8 --slots 8 [--chars 128]     # N concurrent streamed requests through HvxPipeline.serve(stream=True): first-audio
                                                                       # time and piece inter-arrival per request, and the tokens/s of the same requests
                                                                       # with stream=False (what streaming costs under load)
    python tools/bench_stream.py --incremental-vocoder [--serve 8 --slots 8]   # the vocoder on a window per piece (hift.HiftStream) against the whole-cache pass, both
                                                                       # settings in this process: per-piece arrival times, acoustic seconds, vocoder_frames
    python tools/bench_stream.py --incremental-flow [--serve 8 --slots 8]      # the flow on a window per non-final piece against cached K / V (flow.FlowStream) against the
                                                                       # whole-prefix solve, both settings in this process: device time per piece, acoustic seconds,
                                                                       # flow_rows (profiles/flow_stream_ab.log)
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
    if a.incremental_vocoder or a.incremental_flow:
        return serve_ab(a, cfg, pipe, Src, kw, n_spk, 'incremental_flow' if a.incremental_flow else 'incremental_vocoder')
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


def serve_ab(a, cfg, pipe, Src, kw, n_spk, switch='incremental_vocoder'):
    """serve(stream=True) with `switch` off and on, same requests, one process: arrival time of every piece, acoustic seconds, vocoder_frames, flow_rows"""
    res = {}
    for rep in range(2):                                        # first pass warms up (graph capture, workspaces)
        for on in (False, True):
            torch.cuda.synchronize()
            t0 = time.time()
            arr = {}
            for u, piece, info in pipe.serve(Src(), stream=True, **{switch: on}, **kw):
                if isinstance(piece, BaseException):
                    raise piece
                piece = piece.cpu()
                arr.setdefault(u.seed, []).append(time.time() - t0)
            res[on] = (arr, time.time() - t0, dict(pipe.last_continuous))
    print('serve A/B: %d requests of %d tokens in %d slots; %s off | on' % (a.serve, n_spk, a.slots, switch))
    for on in (False, True):
        arr, t, lc = res[on]
        print('  %s: %d pieces, %.3f s wall, acoustic %.3f s, vocoder_frames %d, flow_rows %d, audio %.2f s, %.0f tokens/s'
              % ('on ' if on else 'off', lc['pieces'], t, lc['acoustic_seconds'], lc['vocoder_frames'], lc['flow_rows'], lc['audio_seconds'], lc['tokens'] / t))
    for seed in sorted(res[False][0]):
        print('  request %d piece arrival [s] off: %s' % (seed, ' '.join('%.3f' % x for x in res[False][0][seed])))
        print('  request %d piece arrival [s] on : %s' % (seed, ' '.join('%.3f' % x for x in res[True][0][seed])))
    print('  acoustic seconds on / off = %.3f; vocoder_frames on / off = %.3f; flow_rows on / off = %.3f'
          % (res[True][2]['acoustic_seconds'] / res[False][2]['acoustic_seconds'], res[True][2]['vocoder_frames'] / float(res[False][2]['vocoder_frames']),
             res[True][2]['flow_rows'] / float(res[False][2]['flow_rows'])))


def flow_ab(a, cfg, pipe):
    """the flow alone over one utterance's chunk jobs (prompt + hops of `static_chunk_size` frames, the final full-mask job left out: it is the same solve in both
    settings): device time per piece, whole-prefix solve against FlowStream (random mu: the arithmetic does not depend on the values)"""
    flow, hop = pipe.flow, cfg.flow.static_chunk_size
    prompt = -(-2 * a.prompt // hop) * hop                      # the schedule pads prompt + first hop to whole chunks
    n = prompt + 2 * int(a.chars * 5.5) // hop * hop
    g = torch.Generator().manual_seed(0)
    mu, cond, spk = torch.randn(80, n, generator=g).to('cuda'), torch.zeros(80, n, device='cuda'), torch.randn(80, generator=g).to('cuda')
    jobs = [(T, max(T - hop, prompt) if T > prompt + hop else prompt) for T in range(prompt + hop, n + 1, hop)]
    out = {}
    for on in (False, True):
        for rep in range(2):
            st = flow.stream(n) if on else None
            plane = torch.empty(80, n, device='cuda')
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(jobs) + 1)]
            ev[0].record()
            fill = 0
            for i, (T, cov) in enumerate(jobs):
                if on:
                    fill += flow.solve_incremental_batch([st], [mu[:, :T]], [spk], [cond[:, :T]], [cov], [plane], [fill])[0]
                else:
                    fill += flow.solve_stream_batch([mu[:, :T]], [spk], [cond[:, :T]], [cov], [plane], [fill], streaming=True)[0]
                ev[i + 1].record()
            torch.cuda.synchronize()
            out[on] = ([ev[i].elapsed_time(ev[i + 1]) for i in range(len(jobs))], st.rows_solved if on else sum(T for T, _ in jobs))
            if on:
                st.release()
    print('flow alone: %d frames (%d of them prompt) in %d non-final pieces of %d' % (n, prompt, len(jobs), hop))
    for on in (False, True):
        ms, rows = out[on]
        print('  %s: %.2f ms in all, rows solved %d; per piece [ms]: %s' % ('on ' if on else 'off', sum(ms), rows, ' '.join('%.2f' % x for x in ms)))
    print('  time on / off = %.3f; last piece on / off = %.3f' % (sum(out[True][0]) / sum(out[False][0]), out[True][0][-1] / out[False][0][-1]))


def vocoder_ab(a, cfg, pipe):
    """the vocoder alone over one utterance's worth of mel frames delivered in pieces of `static_chunk_size` frames: device time per piece, whole-cache pass
    against HiftStream (random mel: the arithmetic does not depend on the values)"""
    hop = cfg.flow.static_chunk_size
    n = 2 * int(a.chars * 5.5)
    mel = torch.randn(1, 80, n, generator=torch.Generator().manual_seed(0)).to('cuda')
    fills = [(f, False) for f in range(hop, n, hop)] + [(n, True)]
    out = {}
    for on in (False, True):
        for rep in range(2):
            st = pipe.hift.stream(n) if on else None
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(fills) + 1)]
            ev[0].record()
            for i, (f, fin) in enumerate(fills):
                if on:
                    st.piece(mel, f, fin)
                else:
                    pipe.hift.inference(speech_feat=mel[:, :, :f], finalize=fin)
                ev[i + 1].record()
            torch.cuda.synchronize()
            out[on] = ([ev[i].elapsed_time(ev[i + 1]) for i in range(len(fills))], st.frames_vocoded if on else sum(f for f, _ in fills))
            if on:
                st.close()
    print('vocoder alone: %d frames in %d pieces of %d' % (n, len(fills), hop))
    for on in (False, True):
        ms, frames = out[on]
        print('  %s: %.2f ms in all, frames decoded %d; per piece [ms]: %s' % ('on ' if on else 'off', sum(ms), frames, ' '.join('%.2f' % x for x in ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chars', type=int, default=128)
    ap.add_argument('--heads', type=int, default=2)
    ap.add_argument('--prompt', type=int, default=75, help='prompt speech tokens (3 s)')
    ap.add_argument('--tiny', action='store_true')
    ap.add_argument('--serve', type=int, default=0, help='N concurrent requests through the continuous-batching server, streamed and unstreamed')
    ap.add_argument('--slots', type=int, default=8, help='decode-grid slots of --serve')
    ap.add_argument('--sync-every', type=int, default=None, help='decode steps per host round trip of --serve (default 8)')
    ap.add_argument('--incremental-vocoder', action='store_true', help='A/B of the windowed vocoder (hift.HiftStream) against the whole-cache pass, in one process')
    ap.add_argument('--incremental-flow', action='store_true', help='A/B of the windowed flow (flow.FlowStream) against the whole-prefix solve, in one process')
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

    if a.incremental_vocoder:
        vocoder_ab(a, cfg, pipe)
    if a.incremental_flow:
        flow_ab(a, cfg, pipe)
    for rep in range(2):                                        # first pass warms up (graph capture, workspaces)
        for stream, inc in ((True, False), (True, True), (False, False)) if (a.incremental_vocoder or a.incremental_flow) else ((True, False), (False, False)):
            torch.cuda.synchronize()
            t0 = time.time()
            arr = []
            for wav in stream_tts(tokens(), pipe.flow, pipe.hift, u.prompt_speech_token[None], u.prompt_feat[None], u.embedding[None],
                                  token_hop_len=cfg.flow.static_chunk_size // cfg.flow.token_mel_ratio, stream=stream,
                                  **({'incremental_flow' if a.incremental_flow else 'incremental_vocoder': True} if inc else {})):
                wav = wav.cpu()
                arr.append((time.time() - t0, wav.shape[1] / cfg.sample_rate))
            if rep == 0:
                continue
            audio = sum(x[1] for x in arr)
            print('%s: %d pieces, first audio after %.3f s (%.2f s of audio), all %.2f s of audio after %.3f s (RTF %.4f)'
                  % (('stream+inc' if inc else 'stream   ') if stream else 'one piece', len(arr), arr[0][0], arr[0][1], audio, arr[-1][0], arr[-1][0] / audio))
            if stream:
                print('  piece arrival [s]: ' + ' '.join('%.2f' % x[0] for x in arr))
                late = [i for i in range(1, len(arr)) if arr[i][0] > arr[0][0] + sum(x[1] for x in arr[:i])]
                print('  pieces that would arrive after the audio before them finished playing: %d' % len(late))


if __name__ == '__main__':
    main()
