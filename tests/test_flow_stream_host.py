"""The incremental streaming flow on the host (flow.FlowStream, hvx_flow_stream_*, hvx_cfm_solve_incremental_batch): the window rule, the state layout, the
`flow_rows` accounting of a streamed utterance with the `incremental_flow` switch on and off, the ValueError rules, the new symbols against include/hvx.h, every
refusal of the native solve (none needs a device: the library loads without one), and the statement the feature rests on — under the static chunk mask the rows
below the last chunk boundary of a prefix repeat exactly in a longer solve — on the float64 oracle."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOK = 3
CHUNK = 50


# ------------------------------------------------------------------------------------------------------------------------
# window rule and state layout
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('covered,T,chunk,fill,want', [
    (0, 37, 50, None, (0, 37)),             # a partial first chunk
    (37, 100, 50, None, (0, 100)),          # covered below the first boundary: the whole prefix again
    (100, 237, 50, None, (100, 137)),       # covered on a boundary
    (237, 240, 50, None, (200, 40)),        # covered inside a chunk: back to its boundary
    (240, 350, 50, None, (200, 150)),
    (49, 50, 50, None, (0, 50)),
    (50, 51, 50, None, (50, 1)),
    (150, 200, 50, 150, (150, 50)),         # served traffic: whole chunks, the window is the new hop
    (120, 170, 50, 0, (0, 170)),            # an empty state takes the whole prefix (a prompt's frames are covered from the start)
    (7, 9, 2, None, (6, 3)),
])
def test_window_rule(covered, T, chunk, fill, want):
    from flowmirror_hydravox_amd.flow import window_rule
    assert window_rule(covered, T, chunk, fill=fill) == want


def test_window_rule_refuses_what_the_solve_refuses():
    from flowmirror_hydravox_amd.flow import window_rule
    for bad in ((50, 50, 50, None), (60, 50, 50, None), (-1, 50, 50, None), (0, 50, 0, None), (120, 170, 50, 100)):
        with pytest.raises(ValueError):
            window_rule(*bad[:3], fill=bad[3])


def _host_flow(lib, cfg, dtype_code, max_t=512):
    """a native flow handle without a device: hvx_flow_create keeps the weight pointers and touches nothing"""
    from flowmirror_hydravox_amd import _lib
    cc = _lib.FlowConfig(dtype=dtype_code, vocab=cfg.vocab, mel=cfg.mel, spk_dim=cfg.spk_embed_dim, pla_channels=cfg.pre_lookahead_channels,
                         pla_len=cfg.pre_lookahead_len, dim=cfg.dim, depth=cfg.depth, heads=cfg.heads, ff=cfg.ff, conv_kernel=cfg.conv_kernel,
                         conv_groups=cfg.conv_groups, time_freq_dim=cfg.time_freq_dim, max_t=max_t, cfg_rate=cfg.cfg_rate)
    n = 19 + 10 * cfg.depth + 4
    fake = (C.c_void_p * n)(*([64] * n))
    h = C.c_void_p()
    assert lib.hvx_flow_create(C.byref(cc), fake, n, C.byref(h)) == 0, lib.hvx_last_error()
    return h


@pytest.fixture(scope='module')
def lib():
    from flowmirror_hydravox_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail('libhvx.so is not built')
    return _lib.load()


def test_state_bytes_is_the_documented_layout(lib, tiny_cfg):
    from flowmirror_hydravox_amd.config import FlowConfig
    from flowmirror_hydravox_amd.flow import flow_stream_state_bytes
    for cfg in (tiny_cfg.flow, FlowConfig()):
        for code, dt in ((0, torch.float32), (1, torch.bfloat16)):
            h = _host_flow(lib, cfg, code)
            for frames, steps in ((1, 1), (64, 10), (65, 10), (384, 4), (2048, 10)):
                cap = (frames + 63) // 64 * 64
                es = 4 if code == 0 else 2
                kv = steps * cfg.depth * 2 * (cfg.heads * cap * 64 + cfg.heads * 64 * cap) * es          # K [H][cap][64] + V^T [H][64][cap] per (step, block, branch)
                traj = steps * cfg.mel * cap * 4                                                       # x-trajectory [steps][mel][cap] fp32
                got = lib.hvx_flow_stream_state_bytes(h, frames, steps)
                assert got == kv + traj == flow_stream_state_bytes(cfg, dt, frames, steps), (frames, steps, got)
            assert lib.hvx_flow_stream_state_bytes(h, 0, 10) == 0 and lib.hvx_flow_stream_state_bytes(h, 64, 0) == 0
            lib.hvx_flow_destroy(h)
    # the documented figures: 1.76 MB per frame at CV3 dimensions in bf16 (of which 3.2 KB are the trajectory), 3.6 GB at 2048 frames
    per_frame = flow_stream_state_bytes(FlowConfig(), torch.bfloat16, 2048, 10) / 2048
    assert abs(per_frame / 2 ** 20 - 1.72) < 0.01 and 10 * 80 * 4 == 3200
    assert abs(flow_stream_state_bytes(FlowConfig(), torch.bfloat16, 2048, 10) / 1e9 - 3.7) < 0.1


# ------------------------------------------------------------------------------------------------------------------------
# flow_rows of a streamed utterance, switch off and on, on stand-in models
# ------------------------------------------------------------------------------------------------------------------------
class FakeFlowStream:
    def __init__(self, owner, max_frames):
        self.owner, self.max_frames, self.fill, self.rows_solved, self.released = owner, max_frames, 0, 0, False

    def release(self):
        self.released = True


class FakeFlow:
    """frame j of the whole prefix holds the value j, whichever path produced it"""
    token_mel_ratio = 2
    pre_lookahead_len = LOOK
    static_chunk_size = CHUNK
    max_t = 4096
    device = 'cpu'

    def __init__(self):
        self.streams, self.prefix_calls, self.window_calls = [], [], []

    def inference(self, token, token_len, embedding, finalize=True, prompt_token=None, prompt_token_len=None, prompt_feat=None, prompt_feat_len=None,
                  streaming=False):
        n_p = 0 if prompt_token is None else int(prompt_token.shape[1])
        n = n_p + int(token.shape[1]) - (0 if finalize else LOOK)
        self.prefix_calls.append((2 * n, bool(streaming), bool(finalize)))
        n_pf = 0 if prompt_feat is None else int(prompt_feat.shape[1])
        return torch.arange(n_pf, 2 * n, dtype=torch.float32).expand(1, 80, -1).clone(), None

    def stream(self, max_frames):
        self.streams.append(FakeFlowStream(self, max_frames))
        return self.streams[-1]

    def encode(self, tok, emb, finalize=True):
        n = int(tok.numel()) - (0 if finalize else LOOK)
        return torch.zeros(80, 2 * n), torch.zeros(80)

    def solve_incremental_batch(self, streams, mus, spks, conds, covered, caches, cache_fill, n_timesteps=None):
        from flowmirror_hydravox_amd.flow import window_rule
        out = []
        for st, mu, cov, plane, fill in zip(streams, mus, covered, caches, cache_fill):
            T = int(mu.shape[-1])
            r0, rows = window_rule(cov, T, CHUNK, fill=st.fill)
            self.window_calls.append((r0, rows, T))
            plane[:, fill:fill + T - cov] = torch.arange(cov, T, dtype=torch.float32)
            st.fill, st.rows_solved = T, st.rows_solved + rows
            out.append(T - cov)
        return out


class FakeHift:
    max_stream_frames = 4096

    def inference(self, speech_feat, finalize=True):
        n = int(speech_feat.shape[2])
        assert [int(v) for v in speech_feat[0, 0].tolist()] == list(range(int(speech_feat[0, 0, 0]), int(speech_feat[0, 0, 0]) + n))      # consecutive frames
        return torch.arange(480 * (n if finalize else max(n - 8, 0)), dtype=torch.float32)[None], None


def _session(n_prompt, n_tokens, hop, **kw):
    """the pushes of stream_tts over a StreamSession that is kept, so that its counters can be read"""
    from flowmirror_hydravox_amd.streaming import ChunkSchedule, StreamSession
    flow, hift = FakeFlow(), FakeHift()
    sess = StreamSession(flow, hift, torch.zeros(1, n_prompt, dtype=torch.int32), torch.zeros(1, 2 * n_prompt, 80), torch.zeros(1, 192), **kw)
    sched = ChunkSchedule(n_prompt, hop, LOOK)
    pieces = []
    for t in range(n_tokens):
        for n, covered in sched.feed([t]):
            pieces.append(sess.push(torch.tensor(sched.tokens[:n], dtype=torch.int32)[None], covered, stream=True, finalize=False))
    n, covered = sched.finish()
    pieces.append(sess.push(torch.tensor(sched.tokens[:n], dtype=torch.int32)[None], covered, stream=False, finalize=True))
    return flow, sess, pieces


@pytest.mark.parametrize('n_prompt,n_tokens', [(0, 3 * 25 + LOOK + 1), (26, 131), (24, 1), (60, 200)])
def test_flow_rows_is_the_sum_of_windows_or_of_prefixes(n_prompt, n_tokens):
    from flowmirror_hydravox_amd.flow import window_rule
    from flowmirror_hydravox_amd.streaming import ChunkSchedule
    hop = CHUNK // 2
    sched = ChunkSchedule(n_prompt, hop, LOOK)
    jobs = sched.feed(range(n_tokens))
    last = sched.finish()
    prefixes = [2 * (n_prompt + n - LOOK) for n, _ in jobs]
    final_rows = 2 * (n_prompt + last[0])
    windows, fill = [], 0
    for (n, covered), T in zip(jobs, prefixes):
        windows.append(window_rule(2 * n_prompt + 2 * covered, T, CHUNK, fill=fill))
        fill = T
    flow_off, off, p_off = _session(n_prompt, n_tokens, hop)
    flow_on, on, p_on = _session(n_prompt, n_tokens, hop, incremental_flow=True)
    assert off.flow_rows == sum(prefixes) + final_rows
    assert on.flow_rows == sum(w for _, w in windows) + final_rows
    assert flow_off.window_calls == [] and flow_off.streams == []
    assert flow_on.window_calls == [(r0, w, T) for (r0, w), T in zip(windows, prefixes)]
    assert [c for c in flow_on.prefix_calls] == [(final_rows, False, True)]                  # the final, full-mask job stays a whole-prefix solve
    # served traffic: every non-final prefix is a whole number of chunks, so every window after the first is exactly the new hop
    assert all(T % CHUNK == 0 for T in prefixes)
    assert all(w == CHUNK and r0 == T - CHUNK for (r0, w), T in list(zip(windows, prefixes))[1:])
    if len(jobs) > 1:
        assert on.flow_rows < off.flow_rows
    assert len(p_on) == len(p_off) and all(torch.equal(a, b) for a, b in zip(p_on, p_off))
    assert len(flow_on.streams) == 1 and flow_on.streams[0].released                           # released with the final piece


def test_value_errors_and_release_on_early_stop():
    from flowmirror_hydravox_amd.pipeline import HvxPipeline
    from flowmirror_hydravox_amd.streaming import stream_tts
    from flowmirror_hydravox_amd.worker import serve_queue, worker_process_tts_batched
    import inspect
    flow, hift = FakeFlow(), FakeHift()
    args = (torch.zeros(1, 0, dtype=torch.int32), torch.zeros(1, 0, 80), torch.zeros(1, 192))
    with pytest.raises(ValueError, match='incremental_flow needs stream=True'):
        list(stream_tts(iter(range(30)), flow, hift, *args, stream=False, incremental_flow=True))
    assert flow.streams == []
    pipe = HvxPipeline.__new__(HvxPipeline)                              # (refused before the pipeline is looked at)
    pipe.acoustic_batch = 1
    with pytest.raises(ValueError, match='incremental_flow needs stream=True'):
        list(pipe.serve(None, incremental_flow=True))
    with pytest.raises(ValueError, match='incremental_flow needs stream=True'):
        serve_queue(None, None, {}, incremental_flow=True)
    assert inspect.signature(worker_process_tts_batched).parameters['incremental_flow'].default is False
    # independent of incremental_vocoder: that switch's own rule still speaks first
    with pytest.raises(ValueError, match='incremental_vocoder needs stream=True'):
        serve_queue(None, None, {}, incremental_vocoder=True, incremental_flow=True)
    # a consumer that stops after the first piece leaves no flow stream behind
    gen = stream_tts(iter(range(90)), flow, hift, *args, incremental_flow=True)
    next(gen)
    assert len(flow.streams) == 1 and not flow.streams[0].released
    gen.close()
    assert flow.streams[0].released


# ------------------------------------------------------------------------------------------------------------------------
# the binding against the header, and the refusals of the native solve
# ------------------------------------------------------------------------------------------------------------------------
NEW = {'hvx_flow_stream_state_bytes': 3, 'hvx_flow_stream_workspace_bytes': 3, 'hvx_flow_stream_bind': 7, 'hvx_flow_stream_reset': 3, 'hvx_flow_stream_info': 3,
       'hvx_flow_stream_set_fill': 3, 'hvx_flow_stream_release': 2, 'hvx_cfm_solve_incremental_batch': 20, 'hvx_op_attention_window': 2,
       'hvx_op_attention_window_splits': 7, 'hvx_op_kv_window_append': 13}


def test_new_symbols_are_declared_and_bound(lib):
    from flowmirror_hydravox_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'hvx.h')).read(), flags=re.S)
    assert sorted(n for n in _lib.SYMBOLS if n.startswith('hvx_flow_stream_') or 'incremental' in n or 'window' in n) == sorted(NEW)
    for name, n_args in NEW.items():
        m = re.search(r'\b%s\s*\(([^;]*?)\)\s*;' % name, src, flags=re.S)
        assert m, name
        assert len(m.group(1).split(',')) == n_args == len(_lib.SYMBOLS[name][1]), name
        assert hasattr(lib, name)
    assert _lib.HVX_ABI_VERSION == 8 and lib.hvx_abi_version() == 8                 # additive: the version existing tests pin stays
    assert re.search(r'}\s*hvx_attn_window_args\s*;', src)
    # the operator's argument struct is its own: hvx_attn_args has not grown
    assert C.sizeof(_lib.AttnArgs) == 104


def _solve(lib, h, states, T, covered, t_steps, chunk=CHUNK, t_max=400, null=None, n_steps=None):
    n = len(states)
    ia = lambda v: (C.c_int32 * n)(*v)
    fa = (C.c_float * len(t_steps))(*t_steps)
    planes = (C.c_void_p * n)(*([4096] * n))
    args = dict(ws=C.c_void_p(4096), states=(C.c_void_p * n)(*states), t_len=ia(T), x=C.c_void_p(4096), mu=C.c_void_p(4096), spks=C.c_void_p(4096),
                cond=C.c_void_p(4096), t_steps=fa, dt_steps=fa, covered=ia(covered), cache=planes, cache_ld=ia([4096] * n), cache_fill=ia([0] * n))
    if null:
        args[null] = None
    rc = lib.hvx_cfm_solve_incremental_batch(h, None, args['ws'], 1 << 40, n, t_max, args['states'], args['t_len'], args['x'], args['mu'], args['spks'], args['cond'],
                                             len(t_steps) if n_steps is None else n_steps, args['t_steps'], args['dt_steps'], chunk, args['covered'], args['cache'],
                                             args['cache_ld'], args['cache_fill'])
    return rc, lib.hvx_last_error()


def test_every_refusal_comes_before_any_launch(lib, tiny_cfg):
    """no device is present on the host that runs this: a call that got as far as a launch would fail with a HIP error instead of these messages"""
    from flowmirror_hydravox_amd.flow import euler_schedule
    cfg = tiny_cfg.flow
    h = _host_flow(lib, cfg, 1)
    ts, _ = euler_schedule(4)
    fa = (C.c_float * 4)(*ts)
    need = lib.hvx_flow_stream_state_bytes(h, 300, 4)
    state, other = 1 << 20, 1 << 30                                   # device addresses that are never touched
    # bind: a state that is too small, misaligned, or for a chunk size of 0
    assert lib.hvx_flow_stream_bind(h, C.c_void_p(state), need - 1, 300, 4, fa, CHUNK) == -1 and b'needs' in lib.hvx_last_error()
    assert lib.hvx_flow_stream_bind(h, C.c_void_p(state + 4), need, 300, 4, fa, CHUNK) == -1 and b'aligned' in lib.hvx_last_error()
    assert lib.hvx_flow_stream_bind(h, C.c_void_p(state), need, 300, 4, fa, 0) == -1
    assert lib.hvx_flow_stream_bind(h, None, need, 300, 4, fa, CHUNK) == -1
    rc, msg = _solve(lib, h, [state], [100], [0], ts)
    assert rc == -1 and b'no state bound' in msg
    assert lib.hvx_flow_stream_bind(h, C.c_void_p(state), need, 300, 4, fa, CHUNK) == 0
    info = (C.c_int32 * 4)()
    assert lib.hvx_flow_stream_info(h, C.c_void_p(state), info) == 0 and list(info) == [320, 4, CHUNK, 0]
    # ---- the refusals of hvx_cfm_solve_incremental_batch, on an empty state and on one that holds 150 frames
    for null in ('ws', 'states', 't_len', 'x', 'mu', 'spks', 'cond', 't_steps', 'dt_steps', 'covered', 'cache', 'cache_ld', 'cache_fill'):
        rc, msg = _solve(lib, h, [state], [100], [0], ts, null=null)
        assert rc == -1 and b'null argument' in msg, (null, msg)
    rc, msg = _solve(lib, None, [state], [100], [0], ts)
    assert rc == -1 and b'null argument' in msg
    assert lib.hvx_flow_stream_set_fill(h, C.c_void_p(state), 321) == -1
    assert lib.hvx_flow_stream_set_fill(h, C.c_void_p(state), 150) == 0
    rc, msg = _solve(lib, h, [state], [200], [151], ts)
    assert rc == -1 and b'covered=151 outside [0, fill=150]' in msg, msg
    rc, msg = _solve(lib, h, [state], [150], [150], ts)
    assert rc == -1 and b'adds nothing' in msg, msg
    rc, msg = _solve(lib, h, [state], [120], [150], ts)
    assert rc == -1 and b'adds nothing' in msg, msg
    rc, msg = _solve(lib, h, [state], [321], [150], ts)
    assert rc == -1 and b"exceeds the state's 320 frames" in msg, msg
    rc, msg = _solve(lib, h, [state], [320], [150], ts, t_max=300)
    assert rc == -1 and b'exceeds t_max' in msg, msg
    bits = list(ts)
    bits[2] = float(torch.nextafter(torch.tensor(ts[2], dtype=torch.float32), torch.tensor(2.0)))              # one ulp: compared bitwise
    rc, msg = _solve(lib, h, [state], [200], [150], bits)
    assert rc == -1 and b'schedule differs' in msg, msg
    rc, msg = _solve(lib, h, [state], [200], [150], ts[:3])
    assert rc == -1 and b'schedule differs' in msg, msg
    rc, msg = _solve(lib, h, [state], [200], [150], ts, chunk=25)
    assert rc == -1 and b'chunk size 25' in msg, msg
    rc, msg = _solve(lib, h, [state], [200], [150], ts, chunk=0)
    assert rc == -1 and b'static_chunk_size > 0' in msg, msg
    rc, msg = _solve(lib, h, [state, state], [200, 200], [150, 150], ts)
    assert rc == -1 and b'share a state' in msg, msg
    rc, msg = _solve(lib, h, [state] * 17, [200] * 17, [150] * 17, ts)
    assert rc == -1 and b'17 sessions' in msg, msg
    rc, msg = _solve(lib, h, [state, other], [200, 200], [150, 150], ts)
    assert rc == -1 and b'session 1: no state bound' in msg, msg
    # nothing above touched the state's bookkeeping
    assert lib.hvx_flow_stream_info(h, C.c_void_p(state), info) == 0 and list(info) == [320, 4, CHUNK, 150]
    # an empty state takes any `covered` below T (a prompt's frames): with fill = 0 the same call passes every check above and fails only at the planes' geometry
    assert lib.hvx_flow_stream_set_fill(h, C.c_void_p(state), 0) == 0
    n = 1
    rc = lib.hvx_cfm_solve_incremental_batch(h, None, C.c_void_p(4096), 1 << 40, n, 400, (C.c_void_p * 1)(state), (C.c_int32 * 1)(200), C.c_void_p(4096), C.c_void_p(4096),
                                             C.c_void_p(4096), C.c_void_p(4096), 4, fa, fa, CHUNK, (C.c_int32 * 1)(150), (C.c_void_p * 1)(4096), (C.c_int32 * 1)(10),
                                             (C.c_int32 * 1)(0))
    assert rc == -1 and b'overflow a cache row' in lib.hvx_last_error()
    # a workspace that is too small is the last refusal
    rc = lib.hvx_cfm_solve_incremental_batch(h, None, C.c_void_p(4096), 1024, n, 400, (C.c_void_p * 1)(state), (C.c_int32 * 1)(200), C.c_void_p(4096), C.c_void_p(4096),
                                             C.c_void_p(4096), C.c_void_p(4096), 4, fa, fa, CHUNK, (C.c_int32 * 1)(150), (C.c_void_p * 1)(4096), (C.c_int32 * 1)(4096),
                                             (C.c_int32 * 1)(0))
    assert rc == -1 and b'workspace too small' in lib.hvx_last_error()
    assert lib.hvx_flow_stream_workspace_bytes(h, 1, 50) < lib.hvx_flow_stream_workspace_bytes(h, 1, 200) < lib.hvx_flow_stream_workspace_bytes(h, 4, 200)
    assert lib.hvx_flow_stream_release(h, C.c_void_p(state)) == 0 and lib.hvx_flow_stream_release(h, C.c_void_p(state)) == -1
    lib.hvx_flow_destroy(h)
    # an fp16-mode handle is refused by name, at bind and at the solve
    from flowmirror_hydravox_amd.config import FlowConfig
    h16 = _host_flow(lib, FlowConfig(depth=2), 2)
    assert lib.hvx_flow_stream_bind(h16, C.c_void_p(state), 1 << 40, 300, 4, fa, CHUNK) == -1 and b'fp16 mode' in lib.hvx_last_error()
    rc, msg = _solve(lib, h16, [state], [200], [150], ts)
    assert rc == -1 and b'fp16 mode' in msg, msg
    lib.hvx_flow_destroy(h16)


def test_split_choice_is_a_multiple_of_64_and_fills_the_device(lib):
    from flowmirror_hydravox_amd.ops import attention_window_splits
    for dtype in (torch.bfloat16, torch.float32):
        for batch, heads, rows, kv in ((2, 16, 50, 3000), (2, 16, 100, 640), (2, 2, 87, 237), (2, 8, 150, 350), (16, 16, 50, 500), (2, 16, 50, 64)):
            n, sc = attention_window_splits(dtype, batch, heads, rows, kv, 16)
            assert sc % 64 == 0 and sc >= 64 and 1 <= n <= 16 and (n - 1) * sc < kv <= n * sc, (batch, heads, rows, kv, n, sc)
    # one session of 100 window rows against 3000 keys at CV3 width: 32 workgroups without splits, about two per CU with them
    n, sc = attention_window_splits(torch.bfloat16, 2, 16, 100, 3000, 16)
    assert n == 16 and n * 2 * 16 >= 2 * 256


# ------------------------------------------------------------------------------------------------------------------------
# why it is exact: the oracle, float64
# ------------------------------------------------------------------------------------------------------------------------
def test_rows_below_the_chunk_boundary_repeat_exactly_in_a_longer_solve(tiny_cfg):
    from flowmirror_hydravox_amd import weights as W
    from oracle import flow_ref
    c = tiny_cfg.flow
    assert c.static_chunk_size == CHUNK
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in W.make_flow_state(c, seed=11, init='fan_in').items()}
    gen = torch.Generator().manual_seed(5)
    T = 237
    mu = torch.randn(1, c.mel, T, generator=gen, dtype=torch.float64)
    cond = torch.zeros(1, c.mel, T, dtype=torch.float64)
    cond[:, :, :60] = torch.randn(1, c.mel, 60, generator=gen, dtype=torch.float64)                  # the prompt mel, then zeros
    spk = torch.randn(1, c.mel, generator=gen, dtype=torch.float64)
    noise = flow_ref.cfm_noise(c).double()

    def solve(n):
        with torch.no_grad():
            return flow_ref.cfm_forward(mu[:, :, :n].contiguous(), torch.ones(1, 1, n, dtype=torch.float64), spk, cond[:, :, :n].contiguous(), sd, c, noise=noise,
                                        n_timesteps=4, streaming=True)[0]
    full = solve(T).double()                       # (computed in float64; cfm_forward hands its result out as float32)
    peak = float(full.abs().max())
    for n in (100, 120):
        part = solve(n).double()
        b = n // CHUNK * CHUNK
        below = float((part[:, :b] - full[:, :b]).abs().max()) / peak
        print('prefix %d of %d: rows below %d differ by %.3e of the peak' % (n, T, b, below))
        assert below <= 1e-12, (n, below)
        if n > b:
            inside = float((part[:, b:n] - full[:, b:n]).abs().max()) / peak
            print('prefix %d of %d: rows [%d, %d) of the partial chunk differ by %.3e of the peak' % (n, T, b, n, inside))
            assert inside > 1e-4, (n, inside)
