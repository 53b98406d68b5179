#!/usr/bin/env python3
"""Which roundings keep the flow decoder from the 1e-3 mel contract, and what does an fp16 mode that meets it look like?  CPU study on the 22-block fixture case
(tests/golden/flow_cv3d.npz, e1: T = 192, chunk mask): the oracle (oracle/flow_ref.py) with one family of operands rounded at a time, everything else fp32 —
`_lin` rounds each Linear by its weight's name, `_r` / `_sdpa_emu` round q / k / v and the attention's probabilities and output, the position-embedding
convolution is replaced by one that rounds its operands.  Output: max|d| / max|ref| of the estimator against the fp32 reference.  The last block of rows is
the design of HvxFlow(dtype=torch.float16) (csrc/hvx_flow.hip, DT_F16; tests/test_flow_fp16_host.py pins it).

    python tools/flow_fp16_study.py          # ~1 s per case
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from flowmirror_hydravox_amd import weights as W  # noqa: E402
from flowmirror_hydravox_amd.config import cv3d_config  # noqa: E402
from oracle import flow_ref  # noqa: E402
from test_oracle_golden import cv3w_flow_inputs  # noqa: E402

g = np.load(os.path.join(ROOT, 'tests', 'golden', 'flow_cv3d.npz'))
c = cv3d_config().flow
sd = W.make_flow_state(c, seed=int(g['weight_seed']), init='fan_in')
tag = 'e1'
x, mask, mu, spk, cond = cv3w_flow_inputs(int(g[tag + '_seed']), int(g[tag + '_T']), g[tag + '_lens'].tolist())
t = torch.from_numpy(g[tag + '_t'])
ref = g[tag + '_out']
names = {id(v): k for k, v in sd.items()}
ROUND = {'f32': lambda v: v, 'bf16': flow_ref.bf16r, 'f16': lambda v: v.to(torch.float16).float()}


def family(weight):
    n = names.get(id(weight), '?')
    if 'attn.to_out' in n:
        return 'out'                                     # the attention's out-projection
    if 'attn.to_' in n or 'ff.ff.' in n:
        return 'blk'                                     # QKV, FF1, FF2 of a block
    return 'small'                                       # time MLP, adaLN modulation, input / output projection


def run(blk='f32', out='f32', att='f32', conv='f32', small='f32', stream16=False):
    """operand rounding per family: f32 (none), bf16 or f16; stream16: the residual stream stored as fp16"""
    def lin(a, w, b=None, emu=False, f16=False):
        r = ROUND[{'out': out, 'blk': blk, 'small': small}[family(w)]]
        return F.linear(r(a), r(w), b)

    ra = ROUND[att]

    def sdpa(q, k, v, am):
        s = torch.matmul(q, k.transpose(-1, -2)) / (q.shape[-1] ** 0.5)
        s = s.masked_fill(~am, float('-inf'))
        e = ra(torch.exp(s - s.amax(dim=-1, keepdim=True)))
        return ra(torch.matmul(e, v) / e.sum(dim=-1, keepdim=True))

    def conv_pos(h, sd_, cfg, pre, emu=False):
        rc = ROUND[conv]
        k = cfg.conv_kernel
        h = h.permute(0, 2, 1)
        for name in ('conv1.0.', 'conv2.0.'):
            h = F.mish(F.conv1d(rc(F.pad(h, (k - 1, 0))), rc(sd_[pre + name + 'weight']), sd_[pre + name + 'bias'], groups=cfg.conv_groups))
        return h.permute(0, 2, 1)

    saved = (flow_ref._lin, flow_ref._sdpa_emu, flow_ref._r, flow_ref.causal_conv_pos_embed)
    try:
        flow_ref._lin, flow_ref._sdpa_emu, flow_ref.causal_conv_pos_embed = lin, sdpa, conv_pos
        flow_ref._r = lambda v, emu: ra(v)               # (after the patch above, q / k / v are the only callers)
        with torch.no_grad():
            o = flow_ref.dit_forward(x, mask, mu, t, spk, cond, sd, c, streaming=bool(g[tag + '_streaming']), emu=True, resid16=stream16) * mask
    finally:
        flow_ref._lin, flow_ref._sdpa_emu, flow_ref._r, flow_ref.causal_conv_pos_embed = saved
    return float(np.abs(o.numpy() - ref).max() / np.abs(ref).max())


FP16_MODE = dict(blk='f16', out='f16', att='f16', conv='f16', small='f32')
CASES = [
    ('rounded alone: block QKV / FF1 / FF2 operands in fp16', dict(blk='f16')),
    ('rounded alone: attention out-projection operands in bf16 (product)', dict(out='bf16')),
    ('rounded alone: ... in fp16', dict(out='f16')),
    ('rounded alone: q / k / v / P / attention output in bf16 (product)', dict(att='bf16')),
    ('rounded alone: ... in fp16', dict(att='f16')),
    ('rounded alone: residual stream stored in fp16 (product)', dict(stream16=True)),
    ('rounded alone: conv position embedding operands in bf16 (product)', dict(conv='bf16')),
    ('rounded alone: ... in fp16', dict(conv='f16')),
    ('product as built today (bf16 handle defaults)', dict(blk='f16', out='bf16', att='bf16', conv='bf16', small='f32', stream16=True)),
    ('ALL OF THE ABOVE IN FP16, fp32 stream, fp32 small Linears (the fp16 mode)', FP16_MODE),
    ('  same with the fp16 stream', dict(FP16_MODE, stream16=True)),
    ('  same with the small Linears in fp16', dict(FP16_MODE, small='f16')),
    ('  same with the small Linears in bf16', dict(FP16_MODE, small='bf16')),
]

if __name__ == '__main__':
    print('22 DiT blocks, dim 1024, T = %d (flow_cv3d.npz %s): estimator max|d| / max|ref| against the fp32 reference; contract 1e-3' % (int(g[tag + '_T']), tag))
    for label, kw in CASES:
        print('%-80s %.1e' % (label, run(**kw)), flush=True)
