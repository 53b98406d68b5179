"""The decode-grid job of tests/test_gpu_mixed_heads.py: 8 requests with six different head counts on the 5-head cv3w model, and the fp32 oracle's
id stream of every one of them (tests/golden/mixed_heads_grid.npz).  `python tests/golden/mixed_heads_cases.py` mints the fixture with
oracle/llm_ref.py (our own CPU restatement; no reference code runs here); tests/test_mixed_heads_host.py recomputes it on the CPU and compares.

  own_<i>   ids of request i with inference_head_num = HEADS[i] and its own sampling parameters
  cap_<i>   ids of the same request with inference_head_num = HEAD_CAP (5): they differ from own_<i> for every request with fewer heads, i.e. a
            sampler that ignored the per-sequence count and ran every head of the grid would be caught."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
HEAD_CAP = 5
N_SLOTS = 4
HEADS = [1, 2, 3, 5, 2, 5, 1, 4]
# (top_k, top_p, win_size, tau_r): SET_A is what the LM holds (requests with an even index carry no parameters), the odd ones carry SET_B
SET_A = (25, 0.8, 10, 0.1)
SET_B = (8, 0.95, 6, 0.3)
WIN_CAP = 16
# text tokens per request at ratio 4 (min = max: the length is exact, stop ids are ignored up to it): 60..72 tokens each.  In a 4-slot grid the
# first occupants need 60 / 30 / 23 / 12 steps: request 3 (5 heads) finishes first and request 4 (2 heads) takes its slot — a smaller count —,
# request 2 (3 heads) next and request 5 (5 heads) takes that one — a larger count.
N_TEXT = [15, 15, 17, 15, 16, 15, 18, 16]
RATIO = 4
SEEDS = [9200, 9201, 9202, 9203, 9204, 9205, 9206, 9207]          # the first ones tried


def sp(i):
    top_k, top_p, win, tau = SET_B if i % 2 else SET_A
    return dict(top_k=top_k, top_p=top_p, win_size=win, tau_r=tau)


def grid_texts(c):
    gen = torch.Generator().manual_seed(2025)
    return [torch.randint(0, c.text_vocab, (n,), generator=gen, dtype=torch.int32) for n in N_TEXT]


def oracle_stream(sd, c, text, seed, sampling, heads):
    from oracle import llm_ref, sampler_ref
    return list(llm_ref.llm_inference(sd, c, text, sampler_ref.NoiseStream(seed=seed), inference_head_num=heads, sampling=sampling,
                                      max_token_text_ratio=RATIO, min_token_text_ratio=RATIO, use_kv_cache=True))


def oracle_fixture(sd, c):
    texts = grid_texts(c)
    out = {}
    for i in range(len(N_TEXT)):
        out['own_%d' % i] = np.array(oracle_stream(sd, c, texts[i], SEEDS[i], sp(i), HEADS[i]), dtype=np.int32)
        out['cap_%d' % i] = out['own_%d' % i] if HEADS[i] == HEAD_CAP else np.array(oracle_stream(sd, c, texts[i], SEEDS[i], sp(i), HEAD_CAP), dtype=np.int32)
    return out


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from flowmirror_hydravox_amd import weights as W
    from flowmirror_hydravox_amd.config import cv3w_config
    g = np.load(os.path.join(HERE, 'llm_cv3w.npz'), allow_pickle=False)
    cfg = cv3w_config().llm
    assert cfg.head_num == HEAD_CAP
    sd = W.make_llm_state(cfg, seed=int(g['weight_seed']), init='fan_in', with_lm_head=True)
    fx = oracle_fixture(sd, cfg)
    np.savez_compressed(os.path.join(HERE, 'mixed_heads_grid.npz'), **fx)
    print({k: len(v) for k, v in fx.items()})
