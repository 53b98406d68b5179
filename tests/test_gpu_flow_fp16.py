"""The flow's fp16 mode (HvxFlow(dtype=torch.float16)) on MI355X, held to the CONTRACT — mel / estimator within 1e-3 of the reference's fp32 run, on
max|d| / max|ref| and on relative L2 — at the benchmarked shapes (tests/golden/flow_full_*.npz), at full depth on the small fixture (flow_cv3d.npz, also against
the mode's emulation: tests/test_flow_fp16_host.py), end to end on configs[0] (single_cv3.npz), and kernel by kernel: the fp16 attention tile against float64
on the rotated tile's stress cases, the fp16 position-embedding convolution against a float64 grouped causal convolution."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, state_checksum
from test_flow_fp16_host import fp16_mode_dit
from test_oracle_golden import cv3w_flow_inputs

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CONTRACT = 1e-3


def _scale_rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12))


def _l2_rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _contract(tag, got, ref):
    e = (_scale_rel(got, ref), _l2_rel(got, ref))
    print('%s: max|d|/max|ref| %.2e, relative L2 %.2e  [contract %.0e]' % (tag, e[0], e[1], CONTRACT))
    assert e[0] < CONTRACT and e[1] < CONTRACT, (tag, e)
    return e


@pytest.fixture(scope='module')
def full_sd():
    from flowmirror_hydravox_amd import cv3_config
    from flowmirror_hydravox_amd import weights as W
    c = cv3_config().flow
    sd = W.make_flow_state(c, seed=1987, init='fan_in')
    return c, sd, state_checksum(sd)


@pytest.fixture(scope='module')
def full_flow(full_sd):
    from flowmirror_hydravox_amd.flow import HvxFlow
    c, sd, _ = full_sd
    flow = HvxFlow(c, sd, dtype=torch.float16, max_t=5632 + 64)
    assert flow.fp16 and not flow.bf16 and not (flow.half_stream or flow.f16_linears or flow.f32_small)
    return flow


def test_fp16_dit_22_blocks_5632_frames_vs_reference(full_sd, full_flow):
    c, sd, sha = full_sd
    g = load_golden('flow_full_est.npz')
    assert sha == str(g['weight_sha'])
    T, lens = int(g['T']), g['lens'].tolist()
    x, mask, mu, spk, cond = cv3w_flow_inputs(int(g['seed']), T, lens)
    est = (full_flow.estimator(x, mask, mu, torch.from_numpy(g['t']), spk, cond).cpu() * mask).numpy()
    assert np.isfinite(est).all()
    for i, n in enumerate(lens):
        _contract('fp16 DiT 22 blocks, T = %d, row %d (%d frames)' % (T, i, n), est[i, :, :n], g['out'][i, :, :n])
    assert np.abs(est[1, :, lens[1]:]).max() == 0.0


def test_fp16_cfm_solve_5632_frames_alone_and_in_a_padded_batch(full_sd, full_flow):
    c, sd, sha = full_sd
    g = load_golden('flow_full_solve.npz')
    assert sha == str(g['weight_sha'])
    token, emb = torch.from_numpy(g['token']), torch.from_numpy(g['emb'])
    mel, _ = full_flow.inference(token=token.to(DEV), token_len=torch.tensor([token.shape[1]], dtype=torch.int32), embedding=emb.to(DEV), finalize=True)
    mel = mel.cpu().numpy()
    assert mel.shape == g['mel'].shape and np.isfinite(mel).all()
    _contract('fp16 10-step CFG solve, 2816 tokens -> 5632 frames', mel, g['mel'])
    gen = torch.Generator().manual_seed(5)
    others = [torch.randint(0, c.vocab, (n,), generator=gen, dtype=torch.int32).to(DEV) for n in (2816, 2500, 2050)]
    embs = [emb[0].to(DEV)] + [torch.randn(c.spk_embed_dim, generator=gen).to(DEV) for _ in others]
    mels = full_flow.inference_batch([token[0].to(torch.int32).to(DEV)] + others, embs)
    _contract('   the same utterance as entry 0 of a padded batch of 4', mels[0].cpu().numpy(), g['mel'])


def test_fp16_cfm_solve_with_a_prompt_vs_reference(full_sd, full_flow):
    c, sd, sha = full_sd
    g = load_golden('flow_full_prompt.npz')
    assert sha == str(g['weight_sha'])
    token, ptoken, pfeat, emb = (torch.from_numpy(g[k]) for k in ('token', 'ptoken', 'pfeat', 'emb'))
    mel, _ = full_flow.inference(token=token.to(DEV), token_len=torch.tensor([token.shape[1]], dtype=torch.int32), embedding=emb.to(DEV), finalize=True,
                                 prompt_token=ptoken.to(DEV), prompt_token_len=torch.tensor([ptoken.shape[1]], dtype=torch.int32),
                                 prompt_feat=pfeat.to(DEV), prompt_feat_len=torch.tensor([pfeat.shape[1]], dtype=torch.int32))
    mel = mel.cpu().numpy()
    assert mel.shape == g['mel'].shape and np.isfinite(mel).all()
    _contract('fp16 10-step CFG solve with a prompt, 1408 + 75 tokens', mel, g['mel'])


def test_fp16_packed_weights_round_trip(full_sd, full_flow, tmp_path):
    """save_packed / load_packed of an fp16 handle give the same arithmetic; the pack is refused by a bf16 handle (cache metadata and weights[] tell)"""
    from flowmirror_hydravox_amd import checkpoint
    from flowmirror_hydravox_amd.flow import HvxFlow
    c, sd, _ = full_sd
    path = str(tmp_path / 'flow.fp16.hvxpack')
    checkpoint.save_packed(full_flow, path, source='s')
    assert checkpoint.read_packed_meta(path)['dtype'] == 'torch.float16'
    x, mask, mu, spk, cond = cv3w_flow_inputs(7, 320, [320, 250])
    t = torch.tensor([0.3, 0.3])
    want = full_flow.estimator(x, mask, mu, t, spk, cond).cpu()
    again = HvxFlow(c, None, dtype=torch.float16, max_t=5632 + 64)
    checkpoint.load_packed(again, path, source='s')
    assert torch.equal(again.estimator(x, mask, mu, t, spk, cond).cpu(), want)
    bf = HvxFlow(c, None, dtype=torch.bfloat16, max_t=5632 + 64)
    with pytest.raises(ValueError):
        checkpoint.load_packed(bf, path)
    with pytest.raises(ValueError, match='fp16|float16'):
        bf.load_packed(full_flow._weights)


# ---- 22 blocks, CV3 widths, small fixture ----------------------------------------------------------------------------------------------------------
def test_fp16_flow_22_blocks_vs_reference_and_emulation():
    """estimator at T = 256 with a padded second row and at T = 192 with the static chunk mask (streaming) against the reference (contract) and against the
    mode's emulation (tighter: 6e-4 — the kernels round where the design says), and the 10-step mel with a prompt"""
    from flowmirror_hydravox_amd import weights as W
    from flowmirror_hydravox_amd.config import cv3d_config
    from flowmirror_hydravox_amd.flow import HvxFlow
    g = load_golden('flow_cv3d.npz')
    c = cv3d_config().flow
    sd = W.make_flow_state(c, seed=int(g['weight_seed']), init='fan_in')
    assert state_checksum(sd) == str(g['weight_sha'])
    flow = HvxFlow(c, sd, dtype=torch.float16, max_t=512)
    for tag in ('e0', 'e1'):
        T, lens, streaming = int(g[tag + '_T']), g[tag + '_lens'].tolist(), bool(g[tag + '_streaming'])
        x, mask, mu, spk, cond = cv3w_flow_inputs(int(g[tag + '_seed']), T, lens)
        t = torch.from_numpy(g[tag + '_t'])
        est = (flow.estimator(x, mask, mu, t, spk, cond, streaming=streaming).cpu() * mask).numpy()
        _contract('fp16 22 blocks, %s estimator (streaming=%s) vs the reference' % (tag, streaming), est, g[tag + '_out'])
        with torch.no_grad():
            emu = (fp16_mode_dit(x, mask, mu, t, spk, cond, sd, c, streaming=streaming) * mask).numpy()
        e_emu = _scale_rel(est, emu)
        print('   vs the fp16-mode emulation: %.2e (bound 6e-4)' % e_emu)
        assert e_emu < 6e-4, (tag, e_emu)
    token, ptoken, pfeat, emb = (torch.from_numpy(g[k]) for k in ('token', 'ptoken', 'pfeat', 'emb'))
    mel, _ = flow.inference(token=token.to(DEV), token_len=torch.tensor([token.shape[1]], dtype=torch.int32), embedding=emb.to(DEV), finalize=True,
                            prompt_token=ptoken.to(DEV), prompt_token_len=torch.tensor([ptoken.shape[1]], dtype=torch.int32),
                            prompt_feat=pfeat.to(DEV), prompt_feat_len=torch.tensor([pfeat.shape[1]], dtype=torch.int32))
    _contract('fp16 22 blocks, 10-step mel with a prompt', mel.cpu().numpy(), g['mel'])


def test_bf16_and_fp32_handles_unchanged_by_an_fp16_handle():
    """the fp16 mode adds kernels and arguments the other modes share a library with: their bytes before and after an fp16 handle ran are identical"""
    from flowmirror_hydravox_amd import weights as W
    from flowmirror_hydravox_amd.config import cv3d_config
    from flowmirror_hydravox_amd.flow import HvxFlow
    g = load_golden('flow_cv3d.npz')
    c = cv3d_config().flow
    sd = W.make_flow_state(c, seed=int(g['weight_seed']), init='fan_in')
    handles = {dt: HvxFlow(c, sd, dtype=dt, max_t=512) for dt in (torch.bfloat16, torch.float32)}
    cases = []
    for tag in ('e0', 'e1'):
        T, lens, streaming = int(g[tag + '_T']), g[tag + '_lens'].tolist(), bool(g[tag + '_streaming'])
        cases.append((cv3w_flow_inputs(int(g[tag + '_seed']), T, lens), torch.from_numpy(g[tag + '_t']), streaming))
    run = lambda f: [f.estimator(*inp[:2], inp[2], t, inp[3], inp[4], streaming=st).cpu() for inp, t, st in cases]
    before = {dt: run(f) for dt, f in handles.items()}
    f16 = HvxFlow(c, sd, dtype=torch.float16, max_t=512)
    run(f16)
    after = {dt: run(f) for dt, f in handles.items()}
    for dt in handles:
        assert all(torch.equal(a, b) for a, b in zip(before[dt], after[dt])), dt


# ---- kernels ----------------------------------------------------------------------------------------------------------------------------------------
def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _ref64(q, k, v, kv_len, chunk=0):
    """float64 softmax(q k^T / 8) v with key padding and the static chunk mask; q, k, v [B][H][T][64] -> [B][T][H * 64]"""
    B, H, T, _ = q.shape
    s = q.double() @ k.double().transpose(-1, -2) / 8.0
    mask = torch.arange(T)[None, None, None, :] < kv_len[:, None, None, None]
    if chunk:
        pos = torch.arange(T)
        mask = mask & (pos[None, :] < ((pos // chunk + 1) * chunk)[:, None])[None, None]
    s = s.masked_fill(~mask, float('-inf'))
    return (torch.softmax(s, dim=-1) @ v.double()).transpose(1, 2).reshape(B, T, H * 64)


@pytest.mark.parametrize('case', ['plain', 'spike12', 'spike60', 'spike3000', 'sunk', 'sunk_row', 'dim', 'ragged', 'short_keys', 'one_key', 'chunk', 'short_rows'])
def test_fp16_attention_tile_vs_float64(case):
    """attention.hip, launch_dit_f16: the fp16 DiT tile (running row maximum, fp16 probabilities) on the rotated bf16 tile's stress cases — spikes far above the
    first key tile (what a reference-free or fixed-reference fp16 tile would overflow on), rows whose scores are all ~300 nats down (sunk) or ~85 (dim), ragged and
    very short key lengths, the static chunk mask, and fewer rows than the 64-rows-per-wave form takes — against float64 on the same fp16 operands"""
    from flowmirror_hydravox_amd import _lib, ops
    _lib.require_gpu()
    B, H = 2, 2
    T = 700 if case == 'short_rows' else 2300
    q, k, v = _rand(B, H, T, 64, seed=91), _rand(B, H, T, 64, seed=92), _rand(B, H, T, 64, seed=93)
    if case.startswith('spike'):
        spike = float(case[5:])
        for row, key in ((5, 100), (130, T - 70), (T - 1, 77), (2100, 2200)):
            d = q[0, 1, row] / q[0, 1, row].norm()
            k[0, 1, key] = d * (spike * 8.0 / q[0, 1, row].norm())
    if case.startswith('sunk') or case == 'dim':
        c = torch.zeros(64)
        c[3] = 40.0
        k[0, 1] = k[0, 1] + c
        if case == 'dim':
            q[0, 1] = q[0, 1] - c * (85.0 * 8.0 / 1600.0)
        else:
            for r in (range(T) if case == 'sunk' else (7, 1000, T - 2)):
                q[0, 1, r] = q[0, 1, r] * 0.1 - c * 1.5
    q, k, v = q.half(), k.half(), v.half()
    ql = (q.float() * (0.125 * math.log2(math.e))).half()                      # pre-scaled queries, as the fused QKV epilogue writes them
    Tp = (T + 63) // 64 * 64
    qp = torch.zeros(B, H, Tp, 64, dtype=torch.float16)
    kp = torch.zeros_like(qp)
    vT = torch.zeros(B, H, 64, Tp, dtype=torch.float16)
    qp[:, :, :T], kp[:, :, :T], vT[:, :, :, :T] = ql, k, v.transpose(-1, -2)
    kv_len = torch.tensor([T, T - 89 if case == 'ragged' else T - 9], dtype=torch.int32)
    if case == 'short_keys':
        kv_len = torch.tensor([70, 5], dtype=torch.int32)
    if case == 'one_key':
        kv_len = torch.tensor([T, 1], dtype=torch.int32)
    chunk = 50 if case == 'chunk' else 0
    ref = _ref64(ql.double() * (8.0 * math.log(2.0)), k, v, kv_len, chunk).float()
    out = ops.attention(qp.to(DEV), kp.to(DEV), vT.to(DEV), T, kv_len=kv_len.to(DEV), q_log2=True, chunk=chunk)
    assert out.dtype == torch.float16
    out = out.float().cpu()
    assert torch.isfinite(out).all()
    err = float((out - ref).abs().max())
    print('fp16 attention tile, %s: max |d| %.2e against float64' % (case, err))
    torch.testing.assert_close(out, ref, rtol=5e-3, atol=5e-3)


@pytest.mark.parametrize('T,B', [(4096, 1), (2300, 2), (192, 2), (100, 1)])
def test_fp16_gconv64_vs_float64(T, B):
    """conv_resident.hip, gconv64_kernel<.., f16_t>: the DiT's position-embedding convolution (D = 1024, 16 groups, k = 31, causal) with Mish on fp16 operands at every
    length (the fp16 mode takes this form below 2048 rows too: no tiled fp16 form exists) — Mish -> fp16, and Mish + fp32 residual -> fp32 — against float64"""
    from flowmirror_hydravox_amd import _lib, ops, packing
    _lib.require_gpu()
    D, groups, k = 1024, 16, 31
    x = _rand(B, D, T, seed=113).half().double()
    w = (_rand(D, D // groups, k, seed=114) / math.sqrt(D // groups * k)).half().double()
    b = _rand(D, seed=115)
    res = _rand(B, T, D, seed=116)
    lin = F.mish(F.conv1d(F.pad(x, (k - 1, 0)), w, b.double(), groups=groups)).transpose(1, 2)
    wp = packing.grouped_conv_weight(w.float(), groups).half().to(DEV)
    kw = dict(n_out=D // groups, taps=k, cin_pad=D // groups, pad_left=k - 1, groups=groups, act=_lib.ACT_MISH)
    xr = x.transpose(1, 2).contiguous().half().to(DEV)
    o16 = torch.zeros(B, T, D, dtype=torch.float16, device=DEV)
    ops.conv1d(xr, wp, b.to(DEV), out=o16, **kw)
    d16 = float((o16.double().cpu() - lin).abs().max())
    o32 = ops.conv1d(xr, wp, b.to(DEV), res=res.to(DEV), **kw)
    d32 = float((o32.double().cpu() - (lin + res.double())).abs().max())
    print('fp16 gconv64, T = %d, B = %d: Mish -> fp16 max |d| %.2e, + residual -> fp32 max |d| %.2e' % (T, B, d16, d32))
    torch.testing.assert_close(o16.double().cpu(), lin, rtol=2e-3, atol=2e-3)
    torch.testing.assert_close(o32.double().cpu(), lin + res.double(), rtol=1e-4, atol=1e-4)


# ---- end to end: configs[0] ---------------------------------------------------------------------------------------------------------------------
def test_configs0_fp32_lm_fp16_flow_vs_reference():
    """HvxPipeline(llm_dtype=float32, flow_dtype=float16): the 64-char utterance of configs[0] (K = 1, 352 tokens) — ids bit-exact, mel within the contract"""
    from functools import partial
    from flowmirror_hydravox_amd import cv3_config
    from flowmirror_hydravox_amd import weights as W
    from flowmirror_hydravox_amd.pipeline import HvxPipeline, Utterance
    from flowmirror_hydravox_amd.sampling import ras_sampling
    from oracle import hift_ref
    g = load_golden('single_cv3.npz')
    cfg = cv3_config()
    llm_sd = W.make_llm_state(cfg.llm, seed=1986, init='fan_in', with_lm_head=True)
    flow_sd = W.make_flow_state(cfg.flow, seed=1987, init='fan_in')
    hift_sd = W.make_hift_state(cfg.hift, seed=1988, init='fan_in')
    assert state_checksum(flow_sd) == str(g['flow_sha'])
    top_p, top_k, win, tau = g['sampling']
    pipe = HvxPipeline(cfg, llm_sd, flow_sd, hift_sd, llm_dtype=torch.float32, flow_dtype=torch.float16, max_batch=1, max_ctx=512, max_t=768,
                       hift_tables=hift_ref.make_tables(cfg.hift, seed=9), inference_head_num=1,
                       sampling=partial(ras_sampling, top_p=float(top_p), top_k=int(top_k), win_size=int(win), tau_r=float(tau)))
    assert pipe.flow.fp16
    u = Utterance(text=torch.from_numpy(g['text']), seed=int(g['seed']), embedding=torch.from_numpy(g['emb'][0]))
    wavs, st = pipe.synthesize([u], max_token_text_ratio=5.5, min_token_text_ratio=5.5)
    want = g['tokens'].tolist()
    assert list(st.token_ids[0]) == want
    assert np.isfinite(wavs[0].cpu().numpy()).all()
    mel, _ = pipe.flow.inference(token=torch.tensor(want, dtype=torch.int32, device=DEV)[None], token_len=torch.tensor([len(want)], dtype=torch.int32),
                                 embedding=u.embedding[None].to(DEV), finalize=True)
    _contract('configs[0], fp32 LM + fp16 flow: mel', mel.cpu().numpy(), g['mel'])
