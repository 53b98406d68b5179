"""The flow's fp16 mode (HvxFlow(dtype=torch.float16), hvx_flow_config.dtype == 2) on the host: dtype plumbing, refusals, the packed-weight tell, the
HvxModelManager opt-in, and the design decision itself — the mode's arithmetic emulated on the CPU oracle lands within 5e-4 of the fp32 reference on the
22-block fixture (tests/golden/flow_cv3d.npz), half the 1e-3 contract.  tests/test_gpu_flow_fp16.py holds the kernels to the same emulation."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, state_checksum
from test_oracle_golden import cv3w_flow_inputs


def _r16(v):
    return v.to(torch.float16).float()


def fp16_mode_dit(x, mask, mu, t, spk, cond, sd, cfg, streaming=False):
    """oracle.flow_ref.dit_forward with the fp16 mode's rounding points (csrc/hvx_flow.hip, DT_F16): every operand of the block Linears (QKV, out-projection,
    FF1, FF2) and of the position-embedding convolutions in fp16, q / k / v and the attention's probabilities and output in fp16, the residual stream and the
    small Linears (time MLP, adaLN modulation, input / output projection) in fp32."""
    from oracle import flow_ref

    def lin(a, w, b=None, emu=False, f16=False):
        return F.linear(_r16(a), _r16(w), b) if emu else F.linear(a, w, b)

    def sdpa(q, k, v, am):
        s = torch.matmul(q, k.transpose(-1, -2)) / (q.shape[-1] ** 0.5)
        s = s.masked_fill(~am, float('-inf'))
        e = _r16(torch.exp(s - s.amax(dim=-1, keepdim=True)))
        return _r16(torch.matmul(e, v) / e.sum(dim=-1, keepdim=True))

    saved = (flow_ref._lin, flow_ref._sdpa_emu, flow_ref._r)
    try:
        flow_ref._lin = lin
        flow_ref._sdpa_emu = sdpa
        flow_ref._r = lambda v, emu: _r16(v) if emu else v
        return flow_ref.dit_forward(x, mask, mu, t, spk, cond, sd, cfg, streaming=streaming, emu=True, resid16=False, lin16=True, small32=True)
    finally:
        flow_ref._lin, flow_ref._sdpa_emu, flow_ref._r = saved


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))


def test_dtype_code_and_refusals():
    from flowmirror_hydravox_amd import _lib
    from flowmirror_hydravox_amd.config import FlowConfig, tiny_config
    from flowmirror_hydravox_amd.flow import HvxFlow, fp16_mode_supported
    from flowmirror_hydravox_amd.llm import HvxLLM
    assert _lib.dtype_code(torch.float16) == _lib.F16 == 2
    assert (_lib.dtype_code(torch.float32), _lib.dtype_code(torch.bfloat16)) == (_lib.F32, _lib.BF16) == (0, 1)
    with pytest.raises(_lib.HvxError, match='unsupported dtype'):
        _lib.dtype_code(torch.float64)
    with pytest.raises(_lib.HvxError, match='bf16 or fp32'):
        HvxLLM(tiny_config().llm, None, dtype=torch.float16)
    with pytest.raises(_lib.HvxError, match='fp32, bf16 or fp16'):
        HvxFlow(FlowConfig(), None, dtype=torch.float64)
    assert fp16_mode_supported(FlowConfig())
    for kw in ('half_stream', 'f16_linears', 'f32_small'):
        with pytest.raises(ValueError, match='belong to the bf16 mode'):
            HvxFlow(FlowConfig(), None, dtype=torch.float16, **{kw: True})
    small = tiny_config().flow
    assert not fp16_mode_supported(small)
    with pytest.raises(_lib.HvxError, match='fp16 flow mode needs'):
        HvxFlow(small, None, dtype=torch.float16)


def test_an_fp16_pack_is_told_from_a_bf16_pack_with_fp16_linears():
    """weights[] of each mode (include/hvx.h): the fp16 pack has fp16 block Linears like a bf16 pack with f16_linears, but its attention out-projection is fp16 too —
    and its small Linears and pre-lookahead convolutions are fp32"""
    from flowmirror_hydravox_amd import weights as W
    from flowmirror_hydravox_amd.config import FlowConfig
    from flowmirror_hydravox_amd.flow import pack_flow_state, packed_flow_dtype
    c = FlowConfig(dim=256, depth=2, heads=4, conv_groups=4, pre_lookahead_channels=64, noise_frames=64)
    sd = W.make_flow_state(c, seed=3, init='fan_in')
    f16 = pack_flow_state(c, sd, torch.float16, 'cpu', 64)
    b16 = pack_flow_state(c, sd, torch.bfloat16, 'cpu', 64, f16_linears=True, f32_small=True)
    f32 = pack_flow_state(c, sd, torch.float32, 'cpu', 64)
    assert len(f16) == len(b16) == len(f32) == 19 + 10 * c.depth + 4
    assert (packed_flow_dtype(f16, c.depth), packed_flow_dtype(b16, c.depth), packed_flow_dtype(f32, c.depth)) == (torch.float16, torch.bfloat16, torch.float32)
    half = [15, 17] + [19 + 10 * i + j for i in range(c.depth) for j in (2, 4, 6, 8)]
    single = [5, 7, 9, 11, 13] + [19 + 10 * i for i in range(c.depth)] + [19 + 10 * c.depth, 19 + 10 * c.depth + 2]
    assert all(f16[i].dtype == torch.float16 for i in half), [(i, f16[i].dtype) for i in half]
    assert all(f16[i].dtype == torch.float32 for i in single), [(i, f16[i].dtype) for i in single]
    assert b16[21].dtype == torch.float16 and b16[23].dtype == torch.bfloat16            # the same QKV dtype, another out-projection dtype
    assert all(torch.equal(a.float(), b.float()) for a, b in zip(f16, f32) if a.dtype == torch.float32)


def test_model_manager_fp16_flow_opt_in(monkeypatch):
    from flowmirror_hydravox_amd.model_manager import HvxModelManager
    monkeypatch.delenv('HVX_FLOW_FP16', raising=False)
    assert HvxModelManager().flow_fp16 is False                                          # default: the bf16 production mode
    assert HvxModelManager(flow_fp16=True).flow_fp16 is True
    monkeypatch.setenv('HVX_FLOW_FP16', '1')
    assert HvxModelManager().flow_fp16 is True
    assert HvxModelManager(flow_fp16=False).flow_fp16 is False                           # the constructor argument wins over the host default


def test_emulated_fp16_mode_meets_the_contract_on_the_22_block_fixture():
    """the design decision, pinned on the host: the fp16 mode's rounding points (fp16_mode_dit) within 5e-4 of the fp32 reference on both fixture cases
    (e0: T = 256, padded second row; e1: T = 192, chunk mask) — the product's bf16 mode sits at ~2e-3 on the same cases"""
    from flowmirror_hydravox_amd import weights as W
    from flowmirror_hydravox_amd.config import cv3d_config
    g = load_golden('flow_cv3d.npz')
    c = cv3d_config().flow
    sd = W.make_flow_state(c, seed=int(g['weight_seed']), init='fan_in')
    assert state_checksum(sd) == str(g['weight_sha'])
    for tag in ('e0', 'e1'):
        T, lens, streaming = int(g[tag + '_T']), g[tag + '_lens'].tolist(), bool(g[tag + '_streaming'])
        x, mask, mu, spk, cond = cv3w_flow_inputs(int(g[tag + '_seed']), T, lens)
        with torch.no_grad():
            out = (fp16_mode_dit(x, mask, mu, torch.from_numpy(g[tag + '_t']), spk, cond, sd, c, streaming=streaming) * mask).numpy()
        e = _rel(out, g[tag + '_out'])
        print('emulated fp16 mode, %s: %.2e of the fp32 reference' % (tag, e))
        assert e < 5e-4, (tag, e)
