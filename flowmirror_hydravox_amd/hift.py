"""HvxHift — drop-in for `CausalHiFTGenerator` inference on MI355X (fp32, like the reference).

Mirrors server/model_utils/cosyvoice/hifigan/generator.py:713-726:
    inference(speech_feat, finalize=True) -> (wav float32 (1, 480*T), source (1, 1, 480*T))
The reference moves the F0 predictor to the CPU ("precision is crucial", :715-717); here it runs on the device in fp32
on the exact-fp32 MFMA path.  The fixed noise tables of the causal generator (`rand_ini`, `sine_waves`, `uv`; plain
attributes drawn from the global RNG at construction, generator.py:223-226, 355-356, absent from hift.pt) are explicit:
`tables=` or a seeded default.  All arithmetic runs in libhvx (csrc/hvx_hift.hip, csrc/hift_ops.hip).
"""
import ctypes as C
import weakref

import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .config import HiftConfig
from .packing import conv_weight, fold_weight_norm, pad_to, split_planes
from .weights import hift_spec, check_state, DROP_KEYS, hift_source_down_rates


def make_tables(cfg: HiftConfig, seed=0, n_samples=None):
    """uniform [0,1) tables shaped like the reference's: rand_ini (1,H), sine_waves (1,N,H), uv (1,N,1)."""
    n = cfg.noise_seconds * cfg.sampling_rate if n_samples is None else n_samples
    g = torch.Generator()
    g.manual_seed(seed)
    h = cfg.nb_harmonics + 1
    rand_ini = torch.rand(1, h, generator=g)
    rand_ini[:, 0] = 0
    sine_waves = torch.rand(1, n, h, generator=g)
    uv = torch.rand(1, n, 1, generator=g)
    return dict(rand_ini=rand_ini, sine_waves=sine_waves, uv=uv)


def pack_hift_weights(sd, cfg: HiftConfig, device):
    """Device tensors in the order csrc/hvx_hift.hip consumes them (all fp32, weight-norm folded, kernels [Cout][tap][Cin_pad32])."""
    out = []

    def conv(name, wn=True):
        w = fold_weight_norm(sd, name) if wn else sd[name + '.weight'].float()
        out.append(conv_weight(w.to(device)).contiguous())
        out.append(sd[name + '.bias'].float().to(device).contiguous())

    def resblock(pre, n):
        for d in range(n):
            conv('%sconvs1.%d' % (pre, d))
            conv('%sconvs2.%d' % (pre, d))
            out.append(sd['%sactivations1.%d.alpha' % (pre, d)].float().to(device).contiguous())
            out.append(sd['%sactivations2.%d.alpha' % (pre, d)].float().to(device).contiguous())

    for i in (0, 2, 4, 6, 8):
        conv('f0_predictor.condnet.%d' % i)
    out.append(pad_to(sd['f0_predictor.classifier.weight'].float().to(device), 1, 32).contiguous())
    out.append(sd['f0_predictor.classifier.bias'].float().to(device).contiguous())
    out.append(sd['m_source.l_linear.weight'].float().to(device).reshape(-1).contiguous())
    out.append(sd['m_source.l_linear.bias'].float().to(device).contiguous())
    conv('conv_pre')
    nk = len(cfg.resblock_kernel_sizes)
    for i in range(len(cfg.upsample_rates)):
        conv('ups.%d' % i)
        conv('source_downs.%d' % i, wn=False)
        resblock('source_resblocks.%d.' % i, len(cfg.source_resblock_dilations[i]))
        for j in range(nk):
            resblock('resblocks.%d.' % (i * nk + j), len(cfg.resblock_dilations[j]))
    conv('conv_post')
    return out


def hift_left_context(cfg: HiftConfig):
    """(f0_frames, decode_frames): how far back the causal generator looks, in mel frames.

    f0_frames: the F0 of frame t depends on mel frames [t - f0_frames, t + 3].  condnet.0 (k = 4, causal_type 'right') reads t .. t + 3 and
    has no left tap; condnet.2/4/6/8 are k = 3 causal convolutions with a left pad of 2 each; the classifier is pointwise: 4 * 2 = 8.

    decode_frames: a decoded sample of frame t depends on mel frames >= t - decode_frames and on the source samples of those frames (and,
    through the cached F0 / phase rows and the noise table's absolute index, on nothing else of the past).  Every stage i runs at
    r_i = prod(upsample_rates[:i + 1]) samples per mel frame; R = r_last.  A left reach of k samples at stage i is k / r_i frames =
    k * q_i / R with q_i = R / r_i, so the sum is kept as an integer count of 1 / R frames and rounded up once, at the end.  Going back from
    the samples:
      * the iSTFT's overlap: sample n is covered by the frames f with 4 f - 8 <= n <= 4 f + 7, i.e. ceil((n_fft / 2 - 1) / hop) frames back at rate R;
      * conv_post: a causal k = 7 convolution, 6 at rate R; the reflection pad (1, 0) of the last stage shifts x by 1 at rate R;
      * per stage, last to first: the ResBlocks run in parallel and are averaged, so the widest one counts: max over j of
        sum_d (k_j - 1) * (dilation_jd + 1) (convs1 with its dilation, convs2 with dilation 1), at rate r_i; then the up-sampling
        convolution, (upsample_kernel_sizes[i] - 1) at rate r_i, and the nearest up-sampling in front of it, whose floor(m / u) reaches
        up to (u - 1) further at rate r_i;
      * conv_pre looks right only (conv_pre_look_right frames) and adds nothing on the left.
    That is the mel path.  The source enters every stage i through its own branch: the stage's ResBlocks as above, the source ResBlock
    (source_resblock_kernel_sizes[i], source_resblock_dilations[i]) at rate r_i, the down-sampling convolution (kernel 2 q_i, stride q_i,
    left pad q_i - 1: q_i - 1 at rate R; kernel 1 at the last stage) and the STFT's n_fft / 2 samples = ceil(n_fft / 2 / hop) frames at
    rate R, plus whatever lies between that stage's output and the samples.  decode_frames is the longest of these paths.
    CV3 (rates 8, 5, 3): the mel path is 2669 / 120 = 22.2 frames, the source branch of stage 0 is 3435 / 120 = 28.6 -> 29."""
    f0_frames = 4 * 2
    R = 1
    for u in cfg.upsample_rates:
        R *= u

    def rb(k, dils):
        return sum((k - 1) * (d + 1) for d in dils)
    half = cfg.n_fft // 2
    after = -(-(half - 1) // cfg.hop) + (7 - 1) + 1
    q, best = 1, 0
    for i in reversed(range(len(cfg.upsample_rates))):
        main = max(rb(k, d) for k, d in zip(cfg.resblock_kernel_sizes, cfg.resblock_dilations))
        src = after + (main + rb(cfg.source_resblock_kernel_sizes[i], cfg.source_resblock_dilations[i])) * q + (q - 1) + -(-half // cfg.hop)
        best = max(best, src)
        after += (main + (cfg.upsample_kernel_sizes[i] - 1) + (cfg.upsample_rates[i] - 1)) * q
        q *= cfg.upsample_rates[i]
    best = max(best, after)
    return f0_frames, -(-best // R)


class HiftStream:
    """The vocoder of ONE utterance that is synthesised piece by piece (HvxHift.stream): piece(mel_cache, fill, finalize) returns the samples
    that `hift.inference(mel_cache[:, :fill], finalize)` would add to those already handed out, from a window of the cache — left context
    (hift_left_context) + new frames + look-ahead — and the state carried on the device (F0, phase rows, the phase scan's running sums).
    `frames_vocoded`: mel frames that went through the decode, summed over this object's calls (resets included).
    context: test-only, another (f0_frames, decode_frames)."""

    def __init__(self, hift, max_frames, context=None):
        self.hift, self.lib, self.max_frames = hift, hift.lib, int(max_frames)
        self._st = None
        st = C.c_void_p()
        check(self.lib.hvx_hift_stream_create(hift._h, self.max_frames, C.byref(st)), 'hvx_hift_stream_create')
        self._st = st
        self._state = torch.empty(self.lib.hvx_hift_stream_state_bytes(hift._h, self.max_frames), dtype=torch.uint8, device=hift.device)
        check(self.lib.hvx_hift_stream_bind(st, ptr(self._state), self._state.numel(), ptr(hift.sine_table), hift.sine_table.shape[0]), 'hvx_hift_stream_bind')
        self._context = context
        if context is not None:
            check(self.lib.hvx_hift_stream_set_context(st, int(context[0]), int(context[1])), 'hvx_hift_stream_set_context')
        self._inputs = None
        self._ws = None
        hift._streams.add(self)

    def close(self):
        """release the native state and the device memory (idempotent); the owner's `live_streams` no longer counts it"""
        if self._st is not None:
            self.lib.hvx_hift_stream_destroy(self._st)
            self._st = None
            self._state = self._inputs = self._ws = None
        self.hift._streams.discard(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        check(self.lib.hvx_hift_stream_reset(self._st), 'hvx_hift_stream_reset')
        if self._context is not None:
            check(self.lib.hvx_hift_stream_set_context(self._st, int(self._context[0]), int(self._context[1])), 'hvx_hift_stream_set_context')

    def _info(self):
        out = (C.c_int64 * 8)()
        check(self.lib.hvx_hift_stream_info(self._st, out), 'hvx_hift_stream_info')
        return list(out)

    @property
    def frames_vocoded(self):
        return self._info()[3]

    @property
    def f0(self):
        """the state's F0 array: the final F0 [Hz] of every frame vocoded so far"""
        return self._state[:4 * self.max_frames].view(torch.float32)[:self._info()[1]]

    def set_inputs(self, f0=None, source=None):
        """tests: the F0 of every frame / the source of every sample of the utterance, in place of the predictor / the source stage"""
        keep = [None if t is None else t.to(self.hift.device, torch.float32).contiguous().view(-1) for t in (f0, source)]
        self._inputs = keep
        check(self.lib.hvx_hift_stream_set_inputs(self._st, ptr(keep[0]), ptr(keep[1])), 'hvx_hift_stream_set_inputs')

    def last_source(self):
        """(first sample, source samples) of the latest piece's decode window; a view of the workspace, valid until the handle's next piece"""
        _, _, _, _, w0, frames, off, _ = self._info()
        up = self.hift.up
        return w0 * up, self._ws[off:off + 4 * frames * up].view(torch.float32)

    @torch.inference_mode()
    def piece(self, mel_cache, fill, finalize):
        """mel_cache: the utterance's fp32 mel cache plane (80, ld) or (1, 80, ld) on the device, `fill` valid frames -> (1, L) new samples"""
        hift = self.hift
        mel = mel_cache[0] if mel_cache.dim() == 3 else mel_cache
        if mel.dtype != torch.float32 or mel.device.type != hift.device.type or mel.stride(-1) != 1:
            mel = mel.to(hift.device, torch.float32).contiguous()
        plan = (C.c_int64 * 4)()
        check(self.lib.hvx_hift_stream_plan(self._st, int(fill), 1 if finalize else 0, plan), 'hvx_hift_stream_piece')
        # (one workspace per handle, shared by its streams like HvxHift._ws by its passes: a window's worth, whatever the number of utterances in flight)
        need = self.lib.hvx_hift_stream_workspace_bytes(hift._h, int(plan[1]))
        if hift._stream_ws is None or hift._stream_ws.numel() < need:
            hift._stream_ws = torch.empty(need, dtype=torch.uint8, device=hift.device)
        self._ws = hift._stream_ws
        out = torch.empty(int(plan[0]), dtype=torch.float32, device=hift.device)
        check(self.lib.hvx_hift_stream_piece(hift._h, stream_ptr(), ptr(self._ws), self._ws.numel(), self._st, ptr(mel), mel.stride(0), int(fill),
                                             1 if finalize else 0, ptr(out), out.numel()), 'hvx_hift_stream_piece')
        return out.unsqueeze(0)


class HvxHift:
    def __init__(self, cfg: HiftConfig, state_dict=None, device='cuda', tables=None, table_seed=0, exact_fp32=False):
        """exact_fp32: the decode convolutions on the exact fp32 MFMA forms (hvx_hift_config.exact_fp32: the reference's fp32 vocoder arithmetic, 2.8e-5 of it at
        5632 frames) instead of 3 bf16 MFMAs on (hi, lo) operand pairs (1.5e-4; the default, 2.2x faster).  The F0 predictor is exact fp32 either way."""
        _lib.require_gpu()
        self.exact_fp32 = bool(exact_fp32)
        self.lib = _lib.load()
        self.cfg = cfg
        self.device = torch.device(device)
        self.sampling_rate = cfg.sampling_rate
        self.up = cfg.upsample_total
        t = tables if tables is not None else make_tables(cfg, seed=table_seed)
        self.rand_ini = t['rand_ini']
        self.sine_table = t['sine_waves'][0].to(self.device, torch.float32).contiguous()        # [N][H]
        self._h = None
        self._ws = None
        self._streams = weakref.WeakSet()                # the HiftStream objects alive on this handle (live_streams)
        self._stream_ws = None
        if state_dict is not None:
            self.load_state_dict(state_dict)

    def load_state_dict(self, sd, strict=True):
        return self.load_packed(self.pack_state_dict(sd))

    def pack_state_dict(self, sd):
        sd = {k: v for k, v in sd.items() if k not in DROP_KEYS}
        check_state(sd, hift_spec(self.cfg), 'CausalHiFTGenerator')
        return pack_hift_weights(sd, self.cfg, self.device)

    def load_packed(self, ws):
        c = self.cfg
        if any(len(d) != 3 for d in c.resblock_dilations + c.source_resblock_dilations):
            raise _lib.HvxError('hvx_hift supports three dilations per ResBlock')
        ws = [w.to(self.device) for w in ws]
        self._weights = ws
        cc = _lib.HiftConfig()
        cc.mel, cc.base_channels, cc.nb_harmonics, cc.f0_channels = c.mel, c.base_channels, c.nb_harmonics, c.f0_channels
        cc.n_up = len(c.upsample_rates)
        cc.n_rb = len(c.resblock_kernel_sizes)
        for i, (u, k) in enumerate(zip(c.upsample_rates, c.upsample_kernel_sizes)):
            cc.up_rates[i], cc.up_kernels[i] = u, k
        for j, k in enumerate(c.resblock_kernel_sizes):
            cc.rb_kernels[j] = k
            for d in range(3):
                cc.rb_dils[j][d] = c.resblock_dilations[j][d]
        for i, k in enumerate(c.source_resblock_kernel_sizes):
            cc.src_rb_kernels[i] = k
            for d in range(3):
                cc.src_rb_dils[i][d] = c.source_resblock_dilations[i][d]
        cc.n_fft, cc.hop, cc.conv_pre_kernel, cc.conv_post_kernel = c.n_fft, c.hop, c.conv_pre_look_right + 1, 7
        cc.sampling_rate, cc.nsf_alpha, cc.nsf_sigma = c.sampling_rate, c.nsf_alpha, c.nsf_sigma
        cc.voiced_threshold, cc.lrelu_slope, cc.audio_limit = c.nsf_voiced_threshold, c.lrelu_slope, c.audio_limit
        cc.exact_fp32 = 1 if self.exact_fp32 else 0
        assert hift_source_down_rates(c)[-1] == 1
        if self._h is not None:
            self.lib.hvx_hift_destroy(self._h)
        h = C.c_void_p()
        check(self.lib.hvx_hift_create(C.byref(cc), _lib.ptr_array(ws), len(ws), C.byref(h)), 'hvx_hift_create')
        self._h = h
        # (hi, lo) bf16 plane pairs of the decode convolutions' weights (every 2-D tensor behind the F0 predictor / source linear / conv_pre,
        # except the source down-sampling convolutions, whose input is the fp32 source STFT): hvx_hift_set_weight_planes
        skip = {14}                                                           # conv_pre (its input is the fp32 mel)
        i = 16
        for r in range(cc.n_up):
            skip.add(i + 2)                                                   # source_downs.r
            i += 4 + 18 + cc.n_rb * 18
        self._planes = []
        for k, w in enumerate(ws):
            if k >= 14 and w.dim() == 2 and k not in skip:
                self._planes.append(split_planes(w))
            else:
                self._planes.append(None)
        arr = (C.c_void_p * len(ws))(*[None if p is None else p.data_ptr() for p in self._planes])
        check(self.lib.hvx_hift_set_weight_planes(self._h, arr, len(ws)), 'hvx_hift_set_weight_planes')
        return self

    def eval(self):
        return self

    def cuda(self):
        return self

    def to(self, *a, **k):
        return self

    def __del__(self):
        try:
            if getattr(self, '_h', None) is not None:
                self.lib.hvx_hift_destroy(self._h)
        except Exception:
            pass

    def _workspace(self, t):
        need = self.lib.hvx_hift_workspace_bytes(self._h, t)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def stream(self, max_frames, context=None):
        """a per-utterance streaming vocoder over this handle's weights and noise table, for an utterance of up to max_frames mel frames"""
        return HiftStream(self, max_frames, context=context)

    @property
    def max_stream_frames(self):
        """the longest utterance the fixed noise table covers, in mel frames"""
        return int(self.sine_table.shape[0]) // self.up

    @property
    def live_streams(self):
        """HiftStream objects of this handle that have not been closed"""
        return len(self._streams)

    def piece_samples(self, prev_fill, fill, finalize):
        """samples that a pass over `fill` frames adds to a non-final pass over `prev_fill` (0: nothing handed out yet); host arithmetic"""
        n = self.lib.hvx_hift_stream_piece_samples(self._h, int(prev_fill), int(fill), 1 if finalize else 0)
        if n < 0:
            check(-1, 'hvx_hift_stream_piece_samples')
        return int(n)

    # ---- stages (generator.py:716-721 / :672-711) ------------------------------------------------------------------------------
    def f0(self, mel):
        """mel (80, T) f32 -> f0 [T]"""
        mel = mel.to(self.device, torch.float32).contiguous()
        T = mel.shape[-1]
        out = torch.empty(T, dtype=torch.float32, device=self.device)
        ws = self._workspace(T)
        check(self.lib.hvx_hift_f0(self._h, stream_ptr(), ptr(ws), ws.numel(), ptr(mel), T, ptr(out)), 'hvx_hift_f0')
        return out

    def source(self, f0):
        """f0 [T] -> excitation [T*up]"""
        f0 = f0.to(self.device, torch.float32).contiguous()
        T = f0.numel()
        if T * self.up > self.sine_table.shape[0]:
            raise ValueError('utterance longer than the fixed noise tables (%d samples)' % self.sine_table.shape[0])
        out = torch.empty(T * self.up, dtype=torch.float32, device=self.device)
        ws = self._workspace(T)
        check(self.lib.hvx_hift_source(self._h, stream_ptr(), ptr(ws), ws.numel(), ptr(f0), T, ptr(self.sine_table), ptr(out)), 'hvx_hift_source')
        return out

    def decode(self, mel, source):
        """mel (80, T), source [T*up] -> wav [T*up]"""
        mel = mel.to(self.device, torch.float32).contiguous()
        source = source.to(self.device, torch.float32).contiguous().view(-1)
        T = mel.shape[-1]
        out = torch.empty(T * self.up, dtype=torch.float32, device=self.device)
        ws = self._workspace(T)
        check(self.lib.hvx_hift_decode(self._h, stream_ptr(), ptr(ws), ws.numel(), ptr(mel), ptr(source), T, ptr(out)), 'hvx_hift_decode')
        return out

    def decode_chunk(self, mel, source):
        """finalize=False (generator.py:672-711): the last conv_pre_look_right frames of mel (80, T_in) are look-ahead context;
        source [T_in*up] -> wav [(T_in - look_right - 1) * up] (the last up samples are dropped, generator.py:708-709)"""
        mel = mel.to(self.device, torch.float32).contiguous()
        source = source.to(self.device, torch.float32).contiguous().view(-1)
        T_in, look = mel.shape[-1], self.cfg.conv_pre_look_right
        if T_in - look - 1 <= 0:
            raise ValueError('a non-final chunk needs more than %d mel frames' % (look + 1 + self.f0_look_right))
        out = torch.empty((T_in - look) * self.up, dtype=torch.float32, device=self.device)
        ws = self._workspace(T_in)
        check(self.lib.hvx_hift_decode_chunk(self._h, stream_ptr(), ptr(ws), ws.numel(), ptr(mel), ptr(source), T_in, look, ptr(out)),
              'hvx_hift_decode_chunk')
        return out[:(T_in - look - 1) * self.up]

    # the F0 predictor's first conv looks (kernel 4, causal_type 'right') 3 frames ahead: convolution.py:172, f0_predictor.py:97-100
    f0_look_right = 3

    @torch.inference_mode()
    def inference(self, speech_feat, finalize=True):
        assert speech_feat.shape[0] == 1
        mel = speech_feat[0]
        f0 = self.f0(mel)
        if finalize:
            s = self.source(f0)
            wav = self.decode(mel, s)
        else:
            # f0_predictor.py:97-100: the last 3 frames are real right context, so the f0 of the frames before them is what the full
            # (zero-padded) pass gives for them; source and decode then run on mel[:, :-3] (generator.py:717-725)
            n = mel.shape[-1] - self.f0_look_right
            if n <= 0:
                raise ValueError('a non-final chunk needs more than %d mel frames' % self.f0_look_right)
            s = self.source(f0[:n])
            wav = self.decode_chunk(mel[:, :n], s)
        return wav.unsqueeze(0), s.view(1, 1, -1)
