"""HvxFlow — drop-in for `CausalMaskedDiffWithDiT` + `CausalConditionalCFM` + `DiT` inference on MI355X.

Mirrors server/model_utils/cosyvoice/flow/flow.py:367-430:
    inference(token, token_len, embedding, finalize, prompt_token=None, prompt_token_len=None, prompt_feat=None,
              prompt_feat_len=None, streaming=False) -> (mel float32 (1, 80, 2*N_tok), None)
with the loader-set attributes `bf16` / `fp16` (infer_speech_model.py:99-124).  The host keeps only plumbing: prompt
concatenation, the zero-padded `cond`, slicing the fixed noise (`set_all_random_seed(0); randn(1,80,15000)`,
flow_matching.py:200-201) and the t-grid `1 - cos(linspace(0,1,11) * pi/2)` accumulated exactly as solve_euler does
(flow_matching.py:71-124, 225-227).  All arithmetic runs in libhvx (csrc/hvx_flow.hip).
"""
import ctypes as C

import os

import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .config import FlowConfig
from .packing import conv_weight, grouped_conv_weight, linear_weight
from .weights import flow_spec, check_state, DROP_KEYS


def dit_rope_tables(max_t, head_dim):
    """x_transformers RotaryEmbedding(dim_head).forward_from_seq_len: inv_freq = 1/10000^(2i/d), freqs = pos * inv_freq
    (each duplicated for an interleaved pair) -> cos/sin [max_t][head_dim/2], fp32 on the host."""
    inv = 1.0 / (10000 ** (torch.arange(0, head_dim, 2).float() / head_dim))
    fr = torch.einsum('i,j->ij', torch.arange(max_t).float(), inv)
    return fr.cos().contiguous(), fr.sin().contiguous()


def euler_schedule(n_timesteps):
    """(t_k, dt_k) per step with the reference's accumulation `t = t + dt; dt = t_span[k+1] - t` (flow_matching.py:91-122)."""
    t_span = torch.linspace(0, 1, n_timesteps + 1, dtype=torch.float32)
    t_span = 1 - torch.cos(t_span * 0.5 * torch.pi)
    t, dt = t_span[0], t_span[1] - t_span[0]
    ts, dts = [], []
    for step in range(1, n_timesteps + 1):
        ts.append(float(t))
        dts.append(float(dt))
        t = t + dt
        if step < n_timesteps:
            dt = t_span[step + 1] - t
    return ts, dts


FLOW_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def window_rule(covered, T, chunk, fill=None):
    """The incremental flow's window for a job of T frames of which `covered` are handed out: (r0, rows) — rows [r0, T) are solved, r0 the last chunk boundary at or
    below `covered` (rows below it repeat in every longer solve; rows of a partial chunk do not, so [r0, covered) is solved again and dropped).  fill: frames of the
    state's last prefix, when known — an empty state (0) takes the whole prefix whatever is covered (a prompt's frames are covered from the start)."""
    covered, T, chunk = int(covered), int(T), int(chunk)
    if chunk <= 0 or covered < 0 or T <= covered or (fill is not None and 0 < fill < covered):
        raise ValueError('window_rule: chunk=%d, covered=%d, T=%d, fill=%s' % (chunk, covered, T, fill))
    r0 = 0 if fill == 0 else covered // chunk * chunk
    return r0, T - r0


def flow_stream_state_bytes(cfg, dtype, max_frames, n_steps):
    """bytes of a FlowStream state (include/hvx.h: hvx_flow_stream_state_bytes): K [heads][cap][64] + V^T [heads][64][cap] of every (step, block, CFG branch) in the
    attention's operand type, then the x-trajectory [n_steps][mel][cap] fp32; cap = max_frames rounded up to 64"""
    cap = (int(max_frames) + 63) // 64 * 64
    es = 4 if dtype == torch.float32 else 2
    return n_steps * cfg.depth * 2 * 2 * cfg.heads * cap * 64 * es + n_steps * cfg.mel * cap * 4


class FlowStream:
    """Per-utterance state of the incremental flow (HvxFlow.stream): the K / V^T caches and the x-trajectory of one utterance's chunk-masked solves, in one device
    tensor, plus what the host knows of it.  `fill`: frames of the last prefix solved; `rows_solved`: window rows solved so far (a whole-prefix path would have solved
    the sum of the prefixes).  release() frees the tensor and unregisters it from the flow handle."""

    def __init__(self, flow, max_frames, n_timesteps=None):
        self.flow = flow
        self.n_timesteps = int(n_timesteps or flow.cfg.n_timesteps)
        self.max_frames = int(max_frames)
        self.chunk = int(flow.static_chunk_size)
        need = flow.lib.hvx_flow_stream_state_bytes(flow._h, self.max_frames, self.n_timesteps)
        if need == 0:
            raise _lib.HvxError('FlowStream: max_frames=%d, n_timesteps=%d' % (self.max_frames, self.n_timesteps))
        self.state = torch.empty(need, dtype=torch.uint8, device=flow.device)
        ts, _ = euler_schedule(self.n_timesteps)
        check(flow.lib.hvx_flow_stream_bind(flow._h, ptr(self.state), need, self.max_frames, self.n_timesteps, (C.c_float * self.n_timesteps)(*ts), self.chunk),
              'hvx_flow_stream_bind')
        self.fill = 0
        self.rows_solved = 0
        self.reset()

    def reset(self):
        """a new utterance in the same memory"""
        check(self.flow.lib.hvx_flow_stream_reset(self.flow._h, stream_ptr(), ptr(self.state)), 'hvx_flow_stream_reset')
        self.fill = 0
        self.rows_solved = 0

    def release(self):
        if self.state is not None:
            try:
                if getattr(self.flow, '_h', None) is not None:
                    self.flow.lib.hvx_flow_stream_release(self.flow._h, ptr(self.state))
            finally:
                self.state = None

    close = release

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


def packed_flow_dtype(ws, depth):
    """The flow mode a packed weight list (HvxFlow.pack_state_dict) was made for.  The tell is the attention out-projection of block 0 (weights[23]): it is
    packed in the handle's dtype in every mode — fp32, bf16 (also with fp16 block Linears, whose QKV / FF matrices are fp16 while this one stays bf16), fp16."""
    if depth > 0:
        return ws[19 + 4].dtype
    return ws[15].dtype                                    # (no blocks: the position-embedding convolution, also packed in the handle's dtype)


def fp16_mode_supported(cfg):
    """hvx_flow_create's conditions for the fp16 mode (its fp16 GEMMs exist in the 256-tile Linear and the resident-row convolution only)"""
    return (cfg.dim >= 256 and cfg.dim % 64 == 0 and cfg.ff % 64 == 0 and cfg.ff >= 2 * cfg.dim and cfg.conv_groups > 0 and cfg.dim == 64 * cfg.conv_groups and
            2 <= cfg.conv_kernel <= 33)


def pack_flow_state(cfg, sd, dtype, device, max_t, f16_linears=False, f32_small=False):
    """reference checkpoint -> the tensors libhvx consumes for a flow handle of `dtype`, in the order include/hvx.h documents (HvxFlow.pack_state_dict;
    f16_linears / f32_small: the bf16 mode's switches).  fp16 mode: the DiT's block Linears, attention out-projections and position-embedding convolutions in
    fp16, every other matrix fp32 (small Linears and the pre-lookahead convolutions, as in the fp32 mode)."""
    sd = {k: v for k, v in sd.items() if k not in DROP_KEYS}
    fp16 = dtype == torch.float16
    f32_small = f32_small or fp16
    check_state(sd, flow_spec(cfg), 'CausalMaskedDiffWithDiT', optional=('decoder.estimator.rotary_embed.inv_freq',))
    c, dt, dev = cfg, dtype, torch.device(device)
    e = 'decoder.estimator.'

    def W(k):
        return sd[k].to(dev).float()

    def mat(t):
        return t.to(dt).contiguous()

    def emat(t):                                       # a pre-lookahead convolution of the token encoder: fp32 in the fp16 mode
        return t.float().contiguous() if fp16 else t.to(dt).contiguous()

    def smat(t):                                       # a small Linear of the estimator: fp32 operands when the handle runs them so
        return t.float().contiguous() if f32_small else t.to(dt).contiguous()

    def lmat(t):                                       # a DiT block Linear: fp16 operands when the handle runs them so
        return t.to(torch.float16 if f16_linears else dt).contiguous()

    def vec(t):
        return t.float().contiguous()

    cos, sin = dit_rope_tables(max_t, c.head_dim)
    melp = (c.mel + 31) // 32 * 32
    ws = [cos.to(dev), sin.to(dev), vec(W('input_embedding.weight')), vec(W('spk_embed_affine_layer.weight')),
          vec(W('spk_embed_affine_layer.bias')),
          emat(conv_weight(W('pre_lookahead_layer.conv1.weight'), melp)), vec(W('pre_lookahead_layer.conv1.bias')),
          emat(conv_weight(W('pre_lookahead_layer.conv2.weight'))), vec(W('pre_lookahead_layer.conv2.bias')),
          smat(W(e + 'time_embed.time_mlp.0.weight')), vec(W(e + 'time_embed.time_mlp.0.bias')),
          smat(W(e + 'time_embed.time_mlp.2.weight')), vec(W(e + 'time_embed.time_mlp.2.bias')),
          smat(linear_weight(W(e + 'input_embed.proj.weight'))), vec(W(e + 'input_embed.proj.bias')),
          mat(grouped_conv_weight(W(e + 'input_embed.conv_pos_embed.conv1.0.weight'), c.conv_groups)),
          vec(W(e + 'input_embed.conv_pos_embed.conv1.0.bias')),
          mat(grouped_conv_weight(W(e + 'input_embed.conv_pos_embed.conv2.0.weight'), c.conv_groups)),
          vec(W(e + 'input_embed.conv_pos_embed.conv2.0.bias'))]
    for i in range(c.depth):
        p = e + 'transformer_blocks.%d.' % i
        wqkv = torch.cat([W(p + 'attn.to_q.weight'), W(p + 'attn.to_k.weight'), W(p + 'attn.to_v.weight')], 0)
        bqkv = torch.cat([W(p + 'attn.to_q.bias'), W(p + 'attn.to_k.bias'), W(p + 'attn.to_v.bias')], 0)
        ws += [smat(W(p + 'attn_norm.linear.weight')), vec(W(p + 'attn_norm.linear.bias')), lmat(wqkv), vec(bqkv),
               mat(W(p + 'attn.to_out.0.weight')), vec(W(p + 'attn.to_out.0.bias')),
               lmat(W(p + 'ff.ff.0.0.weight')), vec(W(p + 'ff.ff.0.0.bias')), lmat(W(p + 'ff.ff.2.weight')), vec(W(p + 'ff.ff.2.bias'))]
    ws += [smat(W(e + 'norm_out.linear.weight')), vec(W(e + 'norm_out.linear.bias')), smat(W(e + 'proj_out.weight')), vec(W(e + 'proj_out.bias'))]
    return ws


class HvxFlow:
    def __init__(self, cfg: FlowConfig, state_dict=None, dtype=torch.bfloat16, device='cuda', max_t=None, half_stream=None, f16_linears=None, f32_small=None):
        """dtype: torch.bfloat16 (production: the switches below), torch.float32 (the exact parity mode) or torch.float16 — the reference's deployed dtype
        (`flow.eval().cuda().half()`, infer_speech_model.py:103) with ONE fixed arithmetic and no switches: every matrix-core operand of the DiT (block Linears,
        the attention's out-projection, q / k / V^T and the probabilities, the position-embedding convolutions) in IEEE fp16, the residual stream, the small
        Linears, the token encoder and the solver state in fp32 — within 1e-3 of the fp32 reference (tools/flow_fp16_study.py, tests/test_gpu_flow_fp16.py)."""
        if dtype not in FLOW_DTYPES:
            raise _lib.HvxError('HvxFlow computes in fp32, bf16 or fp16, not %s' % dtype)
        if dtype == torch.float16 and not fp16_mode_supported(cfg):
            raise _lib.HvxError('the fp16 flow mode needs dim >= 256, dim and ff multiples of 64, ff >= 2 dim, 64 channels per conv group and 2..33 conv taps')
        if dtype == torch.float16 and any(v for v in (half_stream, f16_linears, f32_small) if v is not None):
            raise ValueError('half_stream / f16_linears / f32_small belong to the bf16 mode: the fp16 mode has one fixed arithmetic')
        _lib.require_gpu()
        self.lib = _lib.load()
        self.cfg = cfg
        self.dtype = dtype
        self.device = torch.device(device)
        self.bf16 = dtype == torch.bfloat16
        self.fp16 = dtype == torch.float16                 # (the reference's loader attribute: the decoder runs `.half()`)
        # bf16 mode: the DiT's residual stream is kept in fp16, the arithmetic the reference itself runs (`flow.eval().cuda().half()`,
        # infer_speech_model.py:103); half_stream=False keeps it in fp32 (the fp32 mode always does).  HVX_FLOW_HALF_STREAM=0/1 overrides.
        if half_stream is None:
            half_stream = os.environ.get('HVX_FLOW_HALF_STREAM', '1') != '0'
        self.half_stream = bool(half_stream) and self.bf16
        # bf16 mode: the four Linears of every DiT block on IEEE fp16 operands (the reference deploys this decoder as `.half()`); q / k / v and the attention
        # stay bf16.  Together with f32_small below the mode sits at the reference's own fp16 distance from fp32 instead of 3.5x it (tools/
        # dit_rounding_study.py, tests/test_gpu_cv3d.py) for 2 % of the flow's time: ON by default where the 256-tile kernel applies (dim >= 256, dim and ff
        # multiples of 64); f16_linears=False / HVX_FLOW_F16_LINEARS=0 turn it off.
        if f16_linears is None:
            f16_linears = os.environ.get('HVX_FLOW_F16_LINEARS', '1') != '0'
        self.f16_linears = bool(f16_linears) and self.bf16 and cfg.dim >= 256 and cfg.dim % 64 == 0 and (cfg.dim * cfg.ff_mult) % 64 == 0
        # ... and the small Linears (time MLP, adaLN modulation, input / output projection) in fp32: with fp16 block Linears they carry what is left of the
        # bf16 mode's distance from fp32.  ON by default (ff >= 2 dim); f32_small=False / HVX_FLOW_F32_SMALL=0 turn it off.
        if f32_small is None:
            f32_small = os.environ.get('HVX_FLOW_F32_SMALL', '1') != '0'
        self.f32_small = bool(f32_small) and self.bf16 and cfg.ff_mult >= 2
        self.token_mel_ratio = cfg.token_mel_ratio
        self.pre_lookahead_len = cfg.pre_lookahead_len
        self.static_chunk_size = cfg.static_chunk_size            # DiT(static_chunk_size=...), dit.py:119,142
        self.output_size = cfg.mel
        self.max_t = max_t or cfg.noise_frames
        g = torch.Generator()
        g.manual_seed(0)
        self.rand_noise = torch.randn([1, cfg.mel, cfg.noise_frames], generator=g).to(self.device)
        self._h = None
        self._ws = None
        if state_dict is not None:
            self.load_state_dict(state_dict)

    def load_state_dict(self, sd, strict=True):
        return self.load_packed(self.pack_state_dict(sd))

    def pack_state_dict(self, sd):
        """reference checkpoint -> the device tensors libhvx consumes, in the order include/hvx.h documents"""
        return pack_flow_state(self.cfg, sd, self.dtype, self.device, self.max_t, f16_linears=self.f16_linears, f32_small=self.f32_small)

    def load_packed(self, ws):
        c, dt, dev = self.cfg, self.dtype, self.device
        got = packed_flow_dtype(ws, c.depth)
        if got != dt:
            raise ValueError('packed flow weights were made for the %s mode, this handle runs %s' % (got, dt))
        ws = [w.to(dev) for w in ws]
        self._weights = ws
        if self.bf16 and c.depth > 0:
            self.f16_linears = ws[19 + 2].dtype == torch.float16          # (packed weights say how the block Linears were packed)
        if self.bf16:
            self.f32_small = ws[9].dtype == torch.float32
        cc = _lib.FlowConfig(dtype=_lib.dtype_code(dt), vocab=c.vocab, mel=c.mel, spk_dim=c.spk_embed_dim, pla_channels=c.pre_lookahead_channels,
                             pla_len=c.pre_lookahead_len, dim=c.dim, depth=c.depth, heads=c.heads, ff=c.ff, conv_kernel=c.conv_kernel,
                             conv_groups=c.conv_groups, time_freq_dim=c.time_freq_dim, max_t=self.max_t, cfg_rate=c.cfg_rate)
        if self._h is not None:
            self.lib.hvx_flow_destroy(self._h)
            self._h = None
        h = C.c_void_p()
        check(self.lib.hvx_flow_create(C.byref(cc), _lib.ptr_array(ws), len(ws), C.byref(h)), 'hvx_flow_create')
        self._h = h
        # adaLN modulation cache: one slot per distinct Euler step time (the t-grid is a model constant)
        slot = (c.depth * 2 * 6 * c.dim + 2 * 2 * c.dim) * 4
        self._mod_cache = torch.zeros(16 * slot, dtype=torch.uint8, device=dev)
        check(self.lib.hvx_flow_set_mod_cache(self._h, ptr(self._mod_cache), self._mod_cache.numel()), 'hvx_flow_set_mod_cache')
        check(self.lib.hvx_flow_set_half_stream(self._h, 1 if self.half_stream else 0), 'hvx_flow_set_half_stream')
        check(self.lib.hvx_flow_set_f16_linears(self._h, 1 if self.f16_linears else 0), 'hvx_flow_set_f16_linears')
        check(self.lib.hvx_flow_set_f32_small(self._h, 1 if self.f32_small else 0), 'hvx_flow_set_f32_small')
        return self

    def eval(self):
        return self

    def cuda(self):
        return self

    def half(self):
        return self

    def to(self, *a, **k):
        return self

    def __del__(self):
        try:
            if getattr(self, '_h', None) is not None:
                self.lib.hvx_flow_destroy(self._h)
        except Exception:
            pass

    def _workspace(self, batch, t):
        need = self.lib.hvx_flow_workspace_bytes(self._h, batch, t)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    # ---- stage entry points (also used by the parity tests) ----------------------------------------------------------------
    def prelookahead(self, x, context=False):
        """x f32 [n][mel] -> [n][mel] (upsample_encoder.py:82-103); context=True: the last pre_lookahead_len rows are the look-ahead
        context of the rest (`forward(inputs[:-len], context=inputs[-len:])`) -> [n - len][mel]"""
        x = x.to(self.device, torch.float32).contiguous()
        n = x.shape[0]
        ws = self._workspace(2, max(n, 32))
        if context:
            y = torch.empty(n - self.pre_lookahead_len, x.shape[1], dtype=torch.float32, device=self.device)
            check(self.lib.hvx_flow_prelookahead_context(self._h, stream_ptr(), ptr(ws), ws.numel(), ptr(x), n, ptr(y)),
                  'hvx_flow_prelookahead_context')
            return y
        y = torch.empty_like(x)
        check(self.lib.hvx_flow_prelookahead(self._h, stream_ptr(), ptr(ws), ws.numel(), ptr(x), n, ptr(y)), 'hvx_flow_prelookahead')
        return y

    def encode(self, token, embedding, finalize=True):
        """token int [n] (prompt already prepended), embedding f32 [spk_dim] -> mu (mel, 2n), spk (mel,); finalize=False: the last
        pre_lookahead_len tokens are context only (flow.py:401-404) -> mu (mel, 2 (n - len))"""
        token = token.to(self.device, torch.int32).contiguous().view(-1)
        emb = embedding.to(self.device, torch.float32).contiguous().view(-1)
        n = token.numel()
        n_out = n if finalize else n - self.pre_lookahead_len
        if n_out <= 0:
            raise ValueError('a non-final chunk needs more than %d tokens' % self.pre_lookahead_len)
        mu = torch.empty(self.cfg.mel, self.token_mel_ratio * n_out, dtype=torch.float32, device=self.device)
        spk = torch.empty(self.cfg.mel, dtype=torch.float32, device=self.device)
        ws = self._workspace(2, max(2 * n, 32))
        check(self.lib.hvx_flow_encode_chunk(self._h, stream_ptr(), ptr(ws), ws.numel(), ptr(token), n, ptr(emb), 1 if finalize else 0, ptr(mu),
                                             ptr(spk)), 'hvx_flow_encode_chunk')
        return mu, spk

    def estimator(self, x, mask, mu, t, spks, cond, streaming=False):
        """TensorRT-order estimator call (flow_matching.py:126-153): x, mu, cond (B,80,T); mask (B,1,T); t (B,); spks (B,80);
        streaming=True adds the static chunk mask (dit.py:163-164)."""
        B, mel, T = x.shape
        f = lambda a: a.to(self.device, torch.float32).contiguous()
        x, mu, cond, spks, t = f(x), f(mu), f(cond), f(spks), f(t).view(-1)
        if t.numel() == 1 and B > 1:
            t = t.repeat(B)
        kv_len = None
        if mask is not None:
            kv_len = mask.to(self.device).reshape(B, T).ne(0).sum(dim=1).to(torch.int32).contiguous()
        out = torch.empty(B, mel, T, dtype=torch.float32, device=self.device)
        ws = self._workspace(B, T)
        check(self.lib.hvx_cfm_estimator_streaming(self._h, stream_ptr(), ptr(ws), ws.numel(), B, T, ptr(x), ptr(kv_len), ptr(mu), ptr(t),
                                                   ptr(spks), ptr(cond), self.static_chunk_size if streaming else 0, ptr(out)),
              'hvx_cfm_estimator_streaming')
        return out

    def solve(self, mu, spks, cond, n_timesteps=None, noise=None, streaming=False):
        """CausalConditionalCFM.forward (flow_matching.py:204-228): mu, cond (mel,T) f32; spks (mel,) -> mel (mel,T)"""
        T = mu.shape[-1]
        n = n_timesteps or self.cfg.n_timesteps
        z = (self.rand_noise if noise is None else noise.to(self.device))[0, :, :T].to(torch.float32).contiguous().clone()
        ts, dts = euler_schedule(n)
        ta = (C.c_float * n)(*ts)
        da = (C.c_float * n)(*dts)
        ws = self._workspace(2, T)
        check(self.lib.hvx_cfm_solve_streaming(self._h, stream_ptr(), ptr(ws), ws.numel(), T, ptr(z), ptr(mu.contiguous()),
                                               ptr(spks.contiguous()), ptr(cond.contiguous()), n, ta, da,
                                               self.static_chunk_size if streaming else 0), 'hvx_cfm_solve_streaming')
        return z

    def solve_batch(self, mus, spks, conds, n_timesteps=None, streaming=False):
        """Padded multi-utterance solve (hvx_cfm_solve_batch): lists of mu (mel, T_i), spk (mel,), cond (mel, T_i) -> list of mel (mel, T_i).
        The utterances are padded to the longest one; every one draws the same noise prefix the reference gives a single utterance
        (`rand_noise[:, :, :T_i]`, flow_matching.py:222) and key-padding masks keep the padding out of its attention."""
        n_utt = len(mus)
        lens = [int(m.shape[-1]) for m in mus]
        T = max(lens)
        mel, dev = self.cfg.mel, self.device
        n = n_timesteps or self.cfg.n_timesteps
        x = torch.zeros(n_utt, mel, T, dtype=torch.float32, device=dev)
        mu = torch.zeros(n_utt, mel, T, dtype=torch.float32, device=dev)
        cond = torch.zeros(n_utt, mel, T, dtype=torch.float32, device=dev)
        for i in range(n_utt):
            x[i, :, :lens[i]] = self.rand_noise[0, :, :lens[i]]
            mu[i, :, :lens[i]] = mus[i]
            cond[i, :, :lens[i]] = conds[i]
        spk = torch.stack([s_.to(dev, torch.float32).view(-1) for s_ in spks]).contiguous()
        t_len = None if min(lens) == T else torch.tensor(lens, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
        ts, dts = euler_schedule(n)
        ta = (C.c_float * n)(*ts)
        da = (C.c_float * n)(*dts)
        ws = self._workspace(2 * n_utt, T)
        check(self.lib.hvx_cfm_solve_batch(self._h, stream_ptr(), ptr(ws), ws.numel(), n_utt, T, ptr(t_len), ptr(x), ptr(mu), ptr(spk), ptr(cond), n, ta, da,
                                           self.static_chunk_size if streaming else 0), 'hvx_cfm_solve_batch')
        return [x[i, :, :lens[i]] for i in range(n_utt)]

    def solve_stream_batch(self, mus, spks, conds, covered, caches, cache_fill, streaming=True, n_timesteps=None):
        """Chunk jobs of several streaming sessions in ONE padded solve (hvx_cfm_solve_stream_batch): session i's prefix mu / cond (mel, T_i) and spk (mel,) are
        solved as solve_batch solves them (chunk mask when `streaming`), then frames [covered[i], T_i) go into its cache plane caches[i] ((mel, ld_i) fp32,
        contiguous) from column cache_fill[i] on.  `streaming` may be a list (a session's final job runs with the full mask, as `stream_tts`' last call): a
        mixed call is split here into two solves, the attention kernels know one mask mode per launch.  Returns the number of frames appended per session."""
        n_utt = len(mus)
        flags = list(streaming) if isinstance(streaming, (list, tuple)) else [bool(streaming)] * n_utt
        if len(set(flags)) > 1:
            fresh = [0] * n_utt
            for mode in (True, False):
                idx = [i for i in range(n_utt) if bool(flags[i]) == mode]
                pick = lambda v: [v[i] for i in idx]
                for i, f in zip(idx, self.solve_stream_batch(pick(mus), pick(spks), pick(conds), pick(covered), pick(caches), pick(cache_fill), mode, n_timesteps)):
                    fresh[i] = f
            return fresh
        from .ops import mel_append_block
        lens = [int(m.shape[-1]) for m in mus]
        T = max(lens) if lens else 0
        mel, dev = self.cfg.mel, self.device
        n = n_timesteps or self.cfg.n_timesteps
        x = torch.zeros(n_utt, mel, T, dtype=torch.float32, device=dev)
        mu = torch.zeros(n_utt, mel, T, dtype=torch.float32, device=dev)
        cond = torch.zeros(n_utt, mel, T, dtype=torch.float32, device=dev)
        for i in range(n_utt):
            x[i, :, :lens[i]] = self.rand_noise[0, :, :lens[i]]
            mu[i, :, :lens[i]] = mus[i]
            cond[i, :, :lens[i]] = conds[i]
        spk = torch.stack([s_.to(dev, torch.float32).view(-1) for s_ in spks]).contiguous() if n_utt else torch.zeros(0, mel, device=dev)
        tl, cov, pa, ld, fill = mel_append_block(lens, covered, caches, cache_fill)
        ts, dts = euler_schedule(n)
        ta = (C.c_float * n)(*ts)
        da = (C.c_float * n)(*dts)
        ws = self._workspace(2 * max(n_utt, 1), max(T, 1))
        # (equal lengths: no key-padding masks, as solve_batch and the single-session solve run them)
        check(self.lib.hvx_cfm_solve_stream_batch(self._h, stream_ptr(), ptr(ws), ws.numel(), n_utt, T, None if not lens or min(lens) == T else tl, ptr(x), ptr(mu),
                                                  ptr(spk), ptr(cond), n, ta, da, self.static_chunk_size if flags and flags[0] else 0, cov, pa, ld, fill),
              'hvx_cfm_solve_stream_batch')
        return [lens[i] - int(covered[i]) for i in range(n_utt)]

    def stream(self, max_frames, n_timesteps=None):
        """a FlowStream for one utterance of up to max_frames mel frames (prompt included).  Its state takes flow_stream_state_bytes: 1.76 MB per frame at CV3
        dimensions in bf16 (3.6 GB at 2048 frames)."""
        if self.fp16:
            raise _lib.HvxError('the incremental flow serves bf16 and fp32 handles, not the fp16 mode')
        return FlowStream(self, max_frames, n_timesteps)

    def solve_incremental_batch(self, streams, mus, spks, conds, covered, caches, cache_fill, n_timesteps=None):
        """solve_stream_batch(streaming=True) for sessions that own a FlowStream (hvx_cfm_solve_incremental_batch): session i's prefix mu / cond (mel, T_i) are given whole,
        as there, but only rows [r0_i, T_i) — window_rule(covered[i], T_i, static_chunk_size) — are solved, against the cached keys and values of the rows below; frames
        [covered[i], T_i) go into caches[i] from column cache_fill[i] on.  Up to 16 sessions per call (more: further calls).  Returns the frames appended per session."""
        from .ops import mel_append_block
        n_utt = len(mus)
        if n_utt > 16:
            out = []
            for a in range(0, n_utt, 16):
                sl = slice(a, a + 16)
                out += self.solve_incremental_batch(streams[sl], mus[sl], spks[sl], conds[sl], covered[sl], caches[sl], cache_fill[sl], n_timesteps)
            return out
        lens = [int(m.shape[-1]) for m in mus]
        T = max(lens) if lens else 0
        mel, dev = self.cfg.mel, self.device
        n = n_timesteps or self.cfg.n_timesteps
        x = torch.zeros(n_utt, mel, T, dtype=torch.float32, device=dev)
        mu = torch.zeros(n_utt, mel, T, dtype=torch.float32, device=dev)
        cond = torch.zeros(n_utt, mel, T, dtype=torch.float32, device=dev)
        for i in range(n_utt):
            x[i, :, :lens[i]] = self.rand_noise[0, :, :lens[i]]
            mu[i, :, :lens[i]] = mus[i]
            cond[i, :, :lens[i]] = conds[i]
        spk = torch.stack([s_.to(dev, torch.float32).view(-1) for s_ in spks]).contiguous() if n_utt else torch.zeros(0, mel, device=dev)
        tl, cov, pa, ld, fill = mel_append_block(lens, covered, caches, cache_fill)
        ts, dts = euler_schedule(n)
        ta = (C.c_float * n)(*ts)
        da = (C.c_float * n)(*dts)
        chunk = self.static_chunk_size
        rows = [lens[i] - (int(covered[i]) // chunk * chunk if chunk > 0 and streams[i].fill > 0 else 0) for i in range(n_utt)]
        need = self.lib.hvx_flow_stream_workspace_bytes(self._h, max(n_utt, 1), max(rows + [1]))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        ws = self._ws
        sa = (C.c_void_p * max(n_utt, 1))(*[st.state.data_ptr() for st in streams])
        check(self.lib.hvx_cfm_solve_incremental_batch(self._h, stream_ptr(), ptr(ws), ws.numel(), n_utt, T, sa, tl, ptr(x), ptr(mu), ptr(spk), ptr(cond), n, ta, da, chunk,
                                                       cov, pa, ld, fill), 'hvx_cfm_solve_incremental_batch')
        for i, st in enumerate(streams):
            st.fill = lens[i]
            st.rows_solved += rows[i]
        return [lens[i] - int(covered[i]) for i in range(n_utt)]

    @torch.inference_mode()
    def inference_batch(self, tokens, embeddings, prompt_tokens=None, prompt_feats=None, streaming=False):
        """Several utterances through ONE solve (length-bucketed acoustic batches; the reference's `inference` asserts
        batch 1, flow.py:387).  tokens: list of int tensors (n_i,); embeddings: list of (spk_dim,); prompt_tokens / prompt_feats: lists with
        None where an utterance has no prompt.  Returns a list of mels (1, mel, 2 n_i), each what `inference` returns for that utterance."""
        n_utt = len(tokens)
        mus, spks, conds, cut = [], [], [], []
        for i in range(n_utt):
            tok = tokens[i].reshape(-1)
            pt = None if prompt_tokens is None else prompt_tokens[i]
            pf = None if prompt_feats is None else prompt_feats[i]
            if pt is not None:
                tok = torch.concat([pt.reshape(-1).to(tok.device), tok])
            mu, spk = self.encode(tok, embeddings[i].reshape(-1), finalize=True)
            cond = torch.zeros(self.cfg.mel, mu.shape[-1], dtype=torch.float32, device=self.device)
            n1 = 0
            if pf is not None:
                pf = pf.reshape(-1, self.cfg.mel)
                n1 = pf.shape[0]
                cond[:, :n1] = pf.to(self.device, torch.float32).t()
            mus.append(mu)
            spks.append(spk)
            conds.append(cond)
            cut.append(n1)
        feats = self.solve_batch(mus, spks, conds, streaming=streaming)
        return [f[:, c:].unsqueeze(0).float() for f, c in zip(feats, cut)]

    # ---- reference surface ---------------------------------------------------------------------------------------------------
    @torch.inference_mode()
    def inference(self, token, token_len, embedding, finalize=True, prompt_token=None, prompt_token_len=None, prompt_feat=None,
                  prompt_feat_len=None, streaming=False):
        assert token.shape[0] == 1                                       # flow.py:387
        if prompt_token is not None and prompt_token_len is not None:
            token = torch.concat([prompt_token.to(token.device), token], dim=1)
        mu, spk = self.encode(token[0], embedding.reshape(-1), finalize=finalize)
        T = mu.shape[-1]
        mel_len1 = 0
        cond = torch.zeros(self.cfg.mel, T, dtype=torch.float32, device=self.device)
        if prompt_feat is not None and prompt_feat_len is not None:
            mel_len1 = prompt_feat.shape[1]
            cond[:, :mel_len1] = prompt_feat[0].to(self.device, torch.float32).t()
        feat = self.solve(mu, spk, cond, streaming=streaming)
        feat = feat[:, mel_len1:]
        assert feat.shape[1] == T - mel_len1
        return feat.unsqueeze(0).float(), None
