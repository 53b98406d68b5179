"""The decode-grid job of tests/test_gpu_mixed_sampling.py: 8 requests with four sampling parameter sets, and the fp32 oracle's id stream of
every one of them (tests/golden/mixed_sampling_grid.npz).  `python tests/golden/mixed_sampling_cases.py` mints the fixture with oracle/llm_ref.py
(our own CPU restatement; no reference code runs here); tests/test_mixed_sampling_host.py recomputes it on the CPU and compares.

  own_<i>   ids of request i under its own parameters
  w32_<i>   ids of request i with win_size replaced by 32 (the grid's ring capacity), for the requests in WINDOW_SENSITIVE: they differ from
            own_<i>, i.e. a sampler that counted repetitions over the whole ring instead of the request's window would be caught."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
# (top_k, top_p, win_size, tau_r), dealt round-robin to the requests
PARAM_SETS = [(25, 0.8, 10, 0.1), (1, 1.0, 4, 0.05), (50, 0.99, 32, 0.2), (5, 0.5, 24, 0.5)]
WIN_CAP = 32
N_SLOTS = 5
# text tokens per request at ratio 4 (min = max: the length is exact, stop ids are ignored up to it).  Requests 0 and 4 (slots 0 and 4, set 0) finish
# first and together, request 1 (slot 1, set 1) a few blocks later, requests 2 and 3 keep their slots until everything else has joined: requests
# 5 / 6 / 7 (sets 1 / 2 / 3) take over slots whose previous occupant had set 0 / 0 / 1.  Every request produces >= 100 tokens: the shortest ring
# (4 entries) wraps 25 times, the longest (32) three times.
N_TEXT = [25, 33, 45, 46, 25, 26, 27, 28]
RATIO = 4
# seeds picked with the oracle so that the window matters for at least two requests (it does for WINDOW_SENSITIVE: the seed of request 4 was the
# fourth one tried, the others the first)
SEEDS = [9100, 9101, 9102, 9103, 9504, 9105, 9106, 9107]
WINDOW_SENSITIVE = (0, 1, 4)


def sp(i, **over):
    top_k, top_p, win, tau = PARAM_SETS[i % len(PARAM_SETS)]
    return dict(dict(top_k=top_k, top_p=top_p, win_size=win, tau_r=tau), **over)


def grid_texts(c):
    gen = torch.Generator().manual_seed(2024)
    return [torch.randint(0, c.text_vocab, (n,), generator=gen, dtype=torch.int32) for n in N_TEXT]


def oracle_stream(sd, c, text, seed, sampling):
    from oracle import llm_ref, sampler_ref
    return list(llm_ref.llm_inference(sd, c, text, sampler_ref.NoiseStream(seed=seed), inference_head_num=2, sampling=sampling,
                                      max_token_text_ratio=RATIO, min_token_text_ratio=RATIO, use_kv_cache=True))


def oracle_fixture(sd, c):
    texts = grid_texts(c)
    out = {'own_%d' % i: np.array(oracle_stream(sd, c, texts[i], SEEDS[i], sp(i)), dtype=np.int32) for i in range(len(N_TEXT))}
    out.update({'w32_%d' % i: np.array(oracle_stream(sd, c, texts[i], SEEDS[i], sp(i, win_size=WIN_CAP)), dtype=np.int32) for i in WINDOW_SENSITIVE})
    return out


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from flowmirror_hydravox_amd import weights as W
    from flowmirror_hydravox_amd.config import cv3w_config
    g = np.load(os.path.join(HERE, 'llm_cv3w.npz'), allow_pickle=False)
    cfg = cv3w_config().llm
    sd = W.make_llm_state(cfg, seed=int(g['weight_seed']), init='fan_in', with_lm_head=True)
    fx = oracle_fixture(sd, cfg)
    np.savez_compressed(os.path.join(HERE, 'mixed_sampling_grid.npz'), **fx)
    print({k: len(v) for k, v in fx.items()})
