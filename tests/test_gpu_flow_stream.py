"""The incremental streaming flow on the GPU: the windowed attention operator and the cache append against float64 / bit-exact copies, FlowStream pieces against
the CPU oracle beside today's whole-prefix solve, a refused job that leaves the state intact, and HvxPipeline.serve(stream=True, incremental_flow=True) against
the switch-off run.  tests/test_flow_stream_host.py holds the host side (window rule, refusals, the exactness statement on the float64 oracle)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CHUNK = 50
CAP = 512


# ------------------------------------------------------------------------------------------------------------------------
# 1. hvx_op_attention_window against a float64 softmax with the mask
# ------------------------------------------------------------------------------------------------------------------------
def _window_ref(q, k, v, r0, rows, kv_len, chunk):
    """q (H, rows, 64) pre-scaled to log2 units, k / v (H, cap, 64), all float64 -> (rows, H * 64)"""
    s = torch.einsum('hid,hjd->hij', q, k) * math.log(2.0)
    j = torch.arange(k.shape[1])[None, :]
    i = torch.arange(rows)[:, None]
    lim = torch.clamp(((r0 + i) // chunk + 1) * chunk, max=kv_len)
    s = s.masked_fill((j >= lim)[None], float('-inf'))
    return torch.einsum('hij,hjd->ihd', torch.softmax(s, dim=-1), v).reshape(rows, -1)


CASES = [
    ('first rows', [(0, 37, 37)] * 2, 0),
    ('start not a multiple of 8, across a key tile', [(50, 41, 91)] * 2, 0),
    ('two chunks', [(150, 100, 250)] * 2, 0),
    ('partial last chunk', [(150, 87, 237)] * 2, 0),
    ('last rows of the cache', [(450, 50, 500)] * 2, 0),
    ('two windows in one launch', [(50, 41, 91), (150, 87, 237)], 0),
    ('last split shorter than a key tile', [(150, 100, 250)] * 2, 64),          # splits of 64 keys: 192 + 58
]


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
@pytest.mark.parametrize('name,entries,split_chunk', CASES, ids=[c[0].replace(' ', '_') for c in CASES])
def test_attention_window_operator(dtype, name, entries, split_chunk):
    from flowmirror_hydravox_amd import ops
    H, B = 2, len(entries)
    rows = max(e[1] for e in entries)
    gen = torch.Generator().manual_seed(17 + rows)
    q_pad = (rows + 63) // 64 * 64
    q = (torch.randn(B, H, q_pad, 64, generator=gen) * (0.125 * math.log2(math.e))).to(dtype)
    k = torch.randn(B, H, CAP, 64, generator=gen).to(dtype)
    v = torch.randn(B, H, CAP, 64, generator=gen).to(dtype)
    slot = [1, 0]                                                              # entry b's cache is slot 1 - b
    kc, vc = torch.empty_like(k), torch.empty(B, H, 64, CAP, dtype=dtype)
    for b, (r0, n, kv_len) in enumerate(entries):
        k[b, :, kv_len:] = 1e4                                                 # finite garbage at and beyond kv_len: must not matter
        v[b, :, kv_len:] = 1e4
        kc[slot[b]] = k[b]
        vc[slot[b]] = v[b].transpose(1, 2)
    out = ops.attention_window(q.to(DEV), kc.to(DEV), vc.to(DEV), rows, r0=[e[0] for e in entries], kv_len=[e[2] for e in entries], kv_slot=slot, chunk=CHUNK,
                               q_log2=True, split_chunk=split_chunk).float().cpu()
    tol = dict(rtol=3e-2, atol=3e-2) if dtype == torch.bfloat16 else dict(rtol=1e-4, atol=1e-4)
    for b, (r0, n, kv_len) in enumerate(entries):
        ref = _window_ref(q[b, :, :n].double(), k[b].double(), v[b].double(), r0, n, kv_len, CHUNK).float()
        print('%s, %s, entry %d: max abs %.3e' % (name, dtype, b, float((out[b, :n] - ref).abs().max())))
        torch.testing.assert_close(out[b, :n], ref, **tol)


# ------------------------------------------------------------------------------------------------------------------------
# 2. the cache append
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_kv_window_append_lands_at_r0_and_nowhere_else(dtype):
    from flowmirror_hydravox_amd import ops
    H, t_pad = 2, 192
    r0s, rows = [0, 50, 150, 250], [37, 41, 137, 100]                          # (250 is not a multiple of 4)
    caps = [64, 128, 320, 384]
    n = len(r0s)
    gen = torch.Generator().manual_seed(3)
    k = torch.randn(2 * n, H, t_pad, 64, generator=gen).to(dtype).to(DEV)
    vT = torch.randn(2 * n, H, 64, t_pad, generator=gen).to(dtype).to(DEV)
    sentinel = -7.0
    dk = [torch.full((2, H, c, 64), sentinel, dtype=dtype, device=DEV) for c in caps]
    dv = [torch.full((2, H, 64, c), sentinel, dtype=dtype, device=DEV) for c in caps]
    ops.kv_window_append(k, vT, dk, dv, r0s, rows)
    torch.cuda.synchronize()
    for i in range(n):
        a, b = r0s[i], r0s[i] + rows[i]
        for br in range(2):
            assert torch.equal(dk[i][br, :, a:b], k[2 * i + br, :, :rows[i]]), (i, br)
            assert torch.equal(dv[i][br, :, :, a:b], vT[2 * i + br, :, :, :rows[i]]), (i, br)
        assert bool((dk[i][:, :, :a] == sentinel).all()) and bool((dk[i][:, :, b:] == sentinel).all()), i
        assert bool((dv[i][:, :, :, :a] == sentinel).all()) and bool((dv[i][:, :, :, b:] == sentinel).all()), i
    from flowmirror_hydravox_amd._lib import HvxError
    with pytest.raises(HvxError, match='leave a cache'):                        # rows that would leave a cache are refused before the launch
        ops.kv_window_append(k, vT, dk, dv, [0, 50, 150, 300], rows)


# ------------------------------------------------------------------------------------------------------------------------
# 3. pieces of a FlowStream beside the whole-prefix solve, both against the oracle
# ------------------------------------------------------------------------------------------------------------------------
PREFIXES = [37, 100, 237, 240, 350]            # covered = the prefix before: r0 = 0, 0, 100, 200, 200
STEPS = 4


@pytest.fixture(scope='module')
def flow_case(tiny_cfg):
    from flowmirror_hydravox_amd import weights as W
    c = tiny_cfg.flow
    sd = W.make_flow_state(c, seed=11, init='fan_in')
    gen = torch.Generator().manual_seed(5)
    T = PREFIXES[-1]
    mu = torch.randn(c.mel, T, generator=gen)
    cond = torch.zeros(c.mel, T)
    cond[:, :30] = torch.randn(c.mel, 30, generator=gen)                       # the prompt mel, then zeros
    spk = torch.randn(c.mel, generator=gen)
    return dict(cfg=c, sd=sd, mu=mu, cond=cond, spk=spk, oracle={})


def _oracle(case, flow, T):
    """oracle.flow_ref.cfm_forward(streaming=True) with the handle's emulation flags, once per (mode, prefix)"""
    from oracle import flow_ref
    key = (flow.dtype, T)
    if key not in case['oracle']:
        emu = flow.dtype == torch.bfloat16
        with torch.no_grad():
            case['oracle'][key] = flow_ref.cfm_forward(case['mu'][None, :, :T], torch.ones(1, 1, T), case['spk'][None], case['cond'][None, :, :T], case['sd'], case['cfg'],
                                                       n_timesteps=STEPS, streaming=True, emu=emu, resid16=emu and flow.half_stream, lin16=emu and flow.f16_linears,
                                                       small32=emu and flow.f32_small)[0]
    return case['oracle'][key]


def _piece(flow, st, case, T, covered):
    """frames [covered, T) from the stream"""
    dev = flow.device
    plane = torch.zeros(case['cfg'].mel, T - covered, dtype=torch.float32, device=dev)
    got = flow.solve_incremental_batch([st], [case['mu'][:, :T].to(dev)], [case['spk'].to(dev)], [case['cond'][:, :T].to(dev)], [covered], [plane], [0], n_timesteps=STEPS)
    assert got == [T - covered] and st.fill == T
    return plane.cpu()


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_pieces_against_the_oracle_beside_the_whole_prefix_solve(flow_case, dtype):
    """err = distance of the handed-out frames from the oracle, relative to the oracle's peak; asserted: err_incremental <= 1.5 x err_whole_prefix per prefix.
    Measured on MI355X: see DESIGN.md §8."""
    from flowmirror_hydravox_amd.flow import HvxFlow, window_rule
    case = flow_case
    flow = HvxFlow(case['cfg'], case['sd'], dtype=dtype, max_t=512)
    dev = flow.device
    st, st0 = flow.stream(384, n_timesteps=STEPS), flow.stream(384, n_timesteps=STEPS)
    figures, covered = [], 0
    for T in PREFIXES:
        ref = _oracle(case, flow, T)
        peak = float(ref.abs().max())
        whole = flow.solve(case['mu'][:, :T].to(dev), case['spk'].to(dev), case['cond'][:, :T].to(dev), n_timesteps=STEPS, streaming=True).cpu()
        r0, rows = window_rule(covered, T, CHUNK, fill=st.fill)
        before = st.rows_solved
        inc = _piece(flow, st, case, T, covered)
        assert st.rows_solved - before == rows
        again = _piece(flow, st0, case, T, 0)                                  # covered always 0: the r0 == 0 path, the whole prefix every time
        e_whole = float((whole[:, covered:] - ref[:, covered:]).abs().max()) / peak
        e_inc = float((inc - ref[:, covered:]).abs().max()) / peak
        e_whole0 = float((whole - ref).abs().max()) / peak
        e_again = float((again - ref).abs().max()) / peak
        direct = float((inc - whole[:, covered:]).abs().max()) / peak
        figures.append((T, covered, r0, e_whole, e_inc, e_whole0, e_again, direct))
        print('%s T=%d covered=%d r0=%d: whole-prefix %.3e, incremental %.3e (ratio %.2f); all frames: whole-prefix %.3e, r0 == 0 stream %.3e (ratio %.2f); '
              'incremental vs whole-prefix %.3e' % (dtype, T, covered, r0, e_whole, e_inc, e_inc / e_whole, e_whole0, e_again, e_again / e_whole0, direct))
        covered = T
    st.release()
    st0.release()
    for T, covered, r0, e_whole, e_inc, e_whole0, e_again, direct in figures:
        assert e_inc <= 1.5 * e_whole, (T, e_inc, e_whole)
        assert e_again <= 1.5 * e_whole0, (T, e_again, e_whole0)


# ------------------------------------------------------------------------------------------------------------------------
# 4. a refused job leaves the state as it was
# ------------------------------------------------------------------------------------------------------------------------
def test_refused_job_leaves_the_state_intact(flow_case):
    from flowmirror_hydravox_amd._lib import HvxError
    from flowmirror_hydravox_amd.flow import HvxFlow
    case = dict(flow_case)
    gen = torch.Generator().manual_seed(9)
    c = case['cfg']
    case['mu'] = torch.cat([case['mu'], torch.randn(c.mel, 50, generator=gen)], dim=1)            # 400 frames: more than the stream holds
    case['cond'] = torch.cat([case['cond'], torch.zeros(c.mel, 50)], dim=1)
    flow = HvxFlow(c, case['sd'], dtype=torch.bfloat16, max_t=512)
    frames = {}
    for refuse in (False, True):
        st = flow.stream(384, n_timesteps=STEPS)
        _piece(flow, st, case, 100, 0)
        if refuse:
            with pytest.raises(HvxError, match="exceeds the state's 384 frames"):
                _piece(flow, st, case, 400, 100)
            assert st.fill == 100
            with pytest.raises(HvxError, match='outside \\[0, fill=100\\]'):
                _piece(flow, st, case, 237, 101)
        frames[refuse] = _piece(flow, st, case, 237, 100)
        st.release()
    assert torch.equal(frames[True], frames[False])


# ------------------------------------------------------------------------------------------------------------------------
# 5. serve(stream=True, incremental_flow=True)
# ------------------------------------------------------------------------------------------------------------------------
RATIO = 15


class _Src:
    def __init__(self, items):
        self.it = iter(items)

    def poll(self, block):
        return next(self.it)


def _utts(cfg, hop):
    from flowmirror_hydravox_amd.pipeline import synthetic_utterance
    utts = [synthetic_utterance(cfg, 500, 8), synthetic_utterance(cfg, 501, 6), synthetic_utterance(cfg, 502, 10, n_prompt_speech=hop + 1, n_prompt_text=4)]
    for u in utts:
        u.max_token_text_ratio = u.min_token_text_ratio = RATIO
    return utts


def _serve(pipe, cfg, hop, **kw):
    pieces = {}
    for u, piece, info in pipe.serve(_Src(_utts(cfg, hop)), lm_slots=3, stream=True, **kw):
        assert not isinstance(piece, BaseException), piece
        pieces.setdefault(u.seed, []).append((piece.clone(), info))
    return dict(pieces=pieces, stats=dict(pipe.last_continuous))


def _expected_rows(pipe, cfg, hop, tokens, incremental):
    from flowmirror_hydravox_amd.flow import window_rule
    from flowmirror_hydravox_amd.pipeline import _flow_prompt
    from flowmirror_hydravox_amd.streaming import ChunkSchedule
    ratio, look = pipe.flow.token_mel_ratio, pipe.flow.pre_lookahead_len
    total = 0
    for u in _utts(cfg, hop):
        pt = _flow_prompt(u)
        n_prompt = 0 if pt is None else int(pt.numel())
        prompt_frames = 0 if u.prompt_feat is None else int(u.prompt_feat.reshape(-1, pipe.flow.output_size).shape[0])
        sched = ChunkSchedule(n_prompt, hop, look)
        fill = 0
        for n, covered in sched.feed(tokens[u.seed]):
            T = ratio * (n_prompt + n - look)
            total += window_rule(prompt_frames + covered * ratio, T, pipe.flow.static_chunk_size, fill=fill)[1] if incremental else T
            fill = T
        total += ratio * (n_prompt + sched.finish()[0])                        # the final job: the whole prefix, full mask, in both settings
    return total


def test_serve_with_incremental_flow(tiny_cfg):
    from flowmirror_hydravox_amd.pipeline import HvxPipeline
    hop = tiny_cfg.flow.static_chunk_size // tiny_cfg.flow.token_mel_ratio
    pipe = HvxPipeline(tiny_cfg, llm_dtype=torch.float32, flow_dtype=torch.float32, max_batch=3, max_ctx=512, max_t=1024, seed=7, init='fan_in',
                       inference_head_num=2)
    off = _serve(pipe, tiny_cfg, hop)
    tokens = {seed: ps[-1][1]['tokens'] for seed, ps in off['pieces'].items()}
    rows_off, rows_on = _expected_rows(pipe, tiny_cfg, hop, tokens, False), _expected_rows(pipe, tiny_cfg, hop, tokens, True)
    assert off['stats']['flow_rows'] == rows_off
    for kw in (dict(incremental_flow=True), dict(incremental_flow=True, incremental_vocoder=True)):
        on = _serve(pipe, tiny_cfg, hop, **kw)
        for seed, n_text in ((500, 8), (501, 6), (502, 10)):
            a, b = off['pieces'][seed], on['pieces'][seed]
            assert len(a) == len(b) >= 3, (seed, len(a), len(b))
            assert [i for _, i in a] == [i for _, i in b]                          # index, final and, on the last piece, the tokens
            assert [i['final'] for _, i in b] == [False] * (len(b) - 1) + [True]
            assert [p.numel() for p, _ in a] == [p.numel() for p, _ in b], seed    # the set of pieces tiles the utterance as before
            assert sum(p.numel() for p, _ in b) == 960 * RATIO * n_text
            err = max(float((p - q).abs().max()) for (p, _), (q, _) in zip(a, b))
            print('%s utterance %d: %d pieces, max abs %.3e' % (sorted(kw), seed, len(a), err))
            assert err < 2e-2, (seed, err)
        print('%s flow_rows: off %d, on %d' % (sorted(kw), off['stats']['flow_rows'], on['stats']['flow_rows']))
        assert on['stats']['flow_rows'] == rows_on < rows_off
        assert on['stats']['abandoned'] == []
    assert pipe.hift.live_streams == 0
