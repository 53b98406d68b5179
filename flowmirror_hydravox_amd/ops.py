"""Operator-level wrappers over the C-ABI (used by the parity tests and by the model classes).
Every function launches HIP kernels from libhvx on the current torch stream; tensors are plain device buffers."""
import ctypes as C
import math

import torch

from . import _lib
from .packing import sinc_resample_len
from ._lib import GemmArgs, AttnArgs, LlmAttnArgs, SampleArgs, DecodeGemmArgs, ReduceNormArgs, ptr, stream_ptr, check, dtype_code


def _pad32(n):
    return (n + 31) // 32 * 32


def _strides(t):
    """(batch stride, row stride) in elements of a [B][rows][cols] tensor or view whose columns are contiguous"""
    assert t.dim() == 3 and t.stride(2) == 1
    return t.stride(0) if t.shape[0] > 1 else t.shape[1] * t.stride(1), t.stride(1)


def conv1d(x, w_packed, bias, *, n_out, taps, cin_pad, pad_left=0, dil=1, stride=1, up=1, m_out=None, groups=1,
           act=_lib.ACT_NONE, act_param=0.0, act_alpha=None, gate=None, res=None, res_row_off=0, scale=1.0,
           out=None, out_dtype=None, out_row_off=0, out2=None, act2=_lib.ACT_NONE, act2_param=0.0, act2_alpha=None, out2_row_off=0, x3=False,
           a_plane=None, w_plane=None, out_plane=None, out2_plane=None, res2=None, div=0.0):
    """Implicit-GEMM Conv1d / Linear on time-major rows.  x: [B][rows_in][lda] (f32 or bf16), w_packed: [groups][n_out][taps*cin_pad].
    Plane pairs (packing.split_planes; csrc/hvx_kernels.h: GemmArgs.a_planes): a non-None a_plane / w_plane says that x / w_packed is a bf16 tensor
    [2][B][rows_in][lda] / [2][n_out][taps*cin_pad] holding the (hi, lo) planes of fp32 values, the lo plane that many elements behind hi; out_plane /
    out2_plane make `out` / `out2` (bf16 buffers shaped [B][rows][ld] that start at the hi plane) leave as a pair.  The GEMM itself stays fp32."""
    lib = _lib.load()
    if a_plane is not None:
        assert x.dtype == torch.bfloat16 and x.dim() == 4 and x.shape[0] == 2
        B, rows_in, lda = x.shape[1:]
    else:
        B, rows_in, lda = x.shape
    M = rows_in if m_out is None else m_out
    a = GemmArgs()
    a.dtype = _lib.F32 if (a_plane is not None or w_plane is not None) else dtype_code(x.dtype)
    if a_plane is not None:
        a.a_planes, a.a_plane = 1, a_plane
    if w_plane is not None:
        assert w_packed.dtype == torch.bfloat16
        a.w_planes, a.w_plane = 1, w_plane
    a.M, a.N, a.K, a.batch, a.groups = M, n_out, taps * cin_pad, B, groups
    a.A, a.a_bs, a.lda, a.a_gs, a.rows_in = ptr(x), rows_in * lda, lda, (cin_pad if groups > 1 else 0), rows_in
    a.cin_pad, a.conv_stride, a.conv_dil, a.pad_left, a.up = cin_pad, stride, dil, pad_left, up
    a.W, a.w_gs = ptr(w_packed), n_out * taps * cin_pad
    a.bias = ptr(bias)
    a.act, a.act_param, a.act_alpha = act, act_param, ptr(act_alpha)
    if gate is not None:
        a.gate, a.gate_bs = ptr(gate), gate.shape[-1]
    total = groups * n_out
    if res is not None:
        (a.res_bs, a.ldres), a.res, a.res_row_off = _strides(res), ptr(res), res_row_off
        a.res_f16 = int(res.dtype == torch.float16)                 # the DiT's half residual stream (hvx_flow_set_half_stream)
    if res2 is not None:
        (a.res2_bs, a.ldres2), a.res2 = _strides(res2), ptr(res2)
    a.scale, a.div = scale, div
    a.x3 = int(x3)
    if out is None and out2 is None:
        od = out_dtype or torch.float32
        out = torch.zeros(B, M + max(out_row_off, 0), _pad32(total) if od != torch.float32 else total, dtype=od, device=x.device)
    if out is not None:
        (a.out_bs, a.ldo), a.out, a.out_f32 = _strides(out), ptr(out), int(out.dtype == torch.float32)
        a.out_f16 = int(out.dtype == torch.float16)
        if out_plane is not None:
            assert out.dtype == torch.bfloat16
            a.out_planes, a.out_plane, a.out_f32 = 1, out_plane, 1
        a.out_row_off, a.out_cols = out_row_off, out.shape[2]
    if out2 is not None:
        if out2_plane is not None:
            assert out2.dtype == torch.bfloat16
            a.out2_planes, a.out2_plane = 1, out2_plane
        else:
            assert out2.dtype == (torch.float32 if a.dtype == _lib.F32 else x.dtype)
        a.out2, a.act2, a.act2_param, a.act2_alpha = ptr(out2), act2, act2_param, ptr(act2_alpha)
        (a.out2_bs, a.ldo2), a.out2_row_off, a.out2_cols = _strides(out2), out2_row_off, out2.shape[2]
    check(lib.hvx_op_gemm(C.byref(a), stream_ptr()), 'hvx_op_gemm')
    return out


def qkv_gemm_args(x, w, bias, *, heads, t_pad, rope=None, q_scale=0.0, qkv_dtype=None, q=None, k=None, vT=None):
    """the hvx_gemm_args of ops.qkv_gemm and the (q, k, vT) buffers they point to, nothing launched (a test alters a field and calls hvx_op_gemm itself)"""
    B, M, K = x.shape
    N = 3 * heads * 64
    assert x.stride(2) == 1 and w.dtype == x.dtype and tuple(w.shape) == (N, K) and w.is_contiguous(), (x.stride(), w.dtype, w.shape)
    assert bias is None or (bias.dtype == torch.float32 and bias.numel() == N)
    if qkv_dtype is None:
        qkv_dtype = torch.float32 if x.dtype == torch.float32 else torch.bfloat16
    bufs = []
    for t, shape in ((q, (B, heads, t_pad, 64)), (k, (B, heads, t_pad, 64)), (vT, (B, heads, 64, t_pad))):
        if t is None:
            t = torch.zeros(shape, dtype=qkv_dtype, device=x.device)
        assert t.dtype == qkv_dtype, (t.dtype, qkv_dtype)
        bufs.append(t)
    a = GemmArgs()
    a.dtype, a.M, a.N, a.K, a.batch, a.groups = dtype_code(x.dtype), M, N, K, B, 1
    (a.a_bs, a.lda), a.A, a.rows_in = _strides(x), ptr(x), M
    a.cin_pad, a.conv_stride, a.conv_dil, a.pad_left, a.up = K, 1, 1, 0, 1
    a.W, a.w_gs, a.bias, a.scale = ptr(w), N * K, ptr(bias), 1.0
    a.epi, a.heads, a.t_pad, a.q_scale = _lib.EPI_QKV_DIT, heads, t_pad, q_scale
    a.q, a.k, a.vT = (ptr(t) for t in bufs)
    if rope is not None:
        for t in rope:
            assert t is None or (t.dtype == torch.float32 and tuple(t.shape) == (M, 32) and t.stride(1) == 1 and t.stride(0) == 32), (t.dtype, t.shape, t.stride())
        a.rope_cos, a.rope_sin = ptr(rope[0]), ptr(rope[1])
    a.qkv_f16 = int(qkv_dtype == torch.float16)
    return a, tuple(bufs)


def qkv_gemm(x, w, bias, *, heads, t_pad, rope=None, q_scale=0.0, qkv_dtype=None, q=None, k=None, vT=None):
    """The fused QKV Linear of the DiT / Matcha transformer blocks, one launch (csrc/gemm_epilogue.h: EPI_QKV_DIT).  x: [B][M][K] (f32, bf16 or f16),
    w: [3 * heads * 64][K] in the same dtype, bias: f32 [3 * heads * 64] or None, rope: (cos, sin), f32 [M][32] each, or None; q_scale 0.0: q is not scaled.
    -> (q, k, vT): q, k [B][heads][t_pad][64], vT [B][heads][64][t_pad], in qkv_dtype — bf16 for bf16 and for f16 operands, f32 for f32 operands, torch.float16
    (f16 operands only) selects the kernel that writes IEEE fp16.  Caller-provided buffers are written in place (rows / columns t < M only); absent ones are
    allocated zero-filled.  What the kernels cannot take (include/hvx.h: hvx_gemm_args.epi) raises HvxError before anything is launched."""
    a, bufs = qkv_gemm_args(x, w, bias, heads=heads, t_pad=t_pad, rope=rope, q_scale=q_scale, qkv_dtype=qkv_dtype, q=q, k=k, vT=vT)
    check(_lib.load().hvx_op_gemm(C.byref(a), stream_ptr()), 'hvx_op_gemm')
    return bufs


def act_rows(x, act, *, act_param=0.0, alpha=None, out=None, plane=None):
    """y = act(x) for an fp32 [rows][ldx] matrix (per-column alpha for Snake).  plane None: fp32 `out` (allocated when absent); else `out` is a bf16
    buffer [rows][ldy] at the hi plane of a (hi, lo) pair whose lo plane lies `plane` elements behind (elementwise.hip: act_rows_planes_kernel)."""
    lib = _lib.load()
    rows, cols = x.shape
    if out is None:
        assert plane is None
        out = torch.empty_like(x)
    assert out.dtype == (torch.float32 if plane is None else torch.bfloat16)
    check(lib.hvx_op_act_rows(ptr(x), x.stride(0), ptr(out), out.stride(0), int(plane is not None), plane or 0, act, act_param, ptr(alpha), rows, cols,
                              stream_ptr()), 'hvx_op_act_rows')
    return out


def attention(q, k, vT, t, *, kv_len=None, causal=False, scale=None, n_splits=1, split_chunk=0, chunk=0, q_log2=False):
    """q, k: [B][H][Tpad][64]; vT: [B][H][64][Tpad]  ->  [B][t][H*64]"""
    lib = _lib.load()
    B, H, Tp, d = q.shape
    assert d == 64 and vT.shape == (B, H, 64, Tp) and Tp % 32 == 0
    out = torch.empty(B, t, H * 64, dtype=q.dtype, device=q.device)
    a = AttnArgs()
    a.dtype, a.batch, a.heads, a.t, a.t_pad = dtype_code(q.dtype), B, H, t, Tp
    a.q, a.k, a.vT, a.out, a.kv_len = ptr(q), ptr(k), ptr(vT), ptr(out), ptr(kv_len)
    a.causal, a.scale = int(causal), (1.0 / math.sqrt(64)) if scale is None else scale
    a.chunk = int(chunk)
    a.q_log2 = int(q_log2)
    keep = []
    if n_splits > 1:
        rp = _pad32(t)
        po = torch.empty(B * H * n_splits * rp * 64, dtype=torch.float32, device=q.device)
        pm = torch.empty(B * H * n_splits * rp * 2, dtype=torch.float32, device=q.device)
        keep = [po, pm]
        a.n_splits, a.split_chunk, a.part_o, a.part_ml = n_splits, split_chunk, ptr(po), ptr(pm)
    else:
        a.n_splits = 1
    check(lib.hvx_op_attention(C.byref(a), stream_ptr()), 'hvx_op_attention')
    return out


def attention_window(q, k, vT, rows, *, r0, kv_len, kv_slot=None, chunk=0, scale=None, q_log2=False, split_chunk=0, max_splits=16):
    """The windowed DiT attention (hvx_op_attention_window; csrc/attention.hip: attn_window_kernel for bf16, the generic kernel with key splits for fp32).
    q: [B][H][q_pad][64], window-local rows; k: [S][H][cap][64] and vT: [S][H][64][cap], the caches of S slots; entry b reads slot kv_slot[b] (default b), its `rows`
    query rows are rows r0[b] .. of the sequence and see keys j < min(kv_len[b], ((r0[b] + i) / chunk + 1) * chunk).  r0, kv_len: ints or lists per entry.
    -> [B][rows][H*64]"""
    lib = _lib.load()
    B, H, qp, d = q.shape
    S, cap = k.shape[0], k.shape[2]
    assert d == 64 and k.shape == (S, H, cap, 64) and vT.shape == (S, H, 64, cap) and cap % 64 == 0 and k.is_contiguous() and vT.is_contiguous() and q.is_contiguous()
    dev = q.device
    as_list = lambda v: [int(v)] * B if isinstance(v, int) else [int(x) for x in v]
    r0l, kvl = as_list(r0), as_list(kv_len)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    keep = [i32(r0l), i32(kvl), None if kv_slot is None else i32([int(x) for x in kv_slot])]
    out = torch.empty(B, rows, H * 64, dtype=q.dtype, device=dev)
    rp = _pad32(rows)
    po = torch.empty(B * H * max_splits * rp * 64, dtype=torch.float32, device=dev)
    pm = torch.empty(B * H * max_splits * rp * 2, dtype=torch.float32, device=dev)
    a = _lib.AttnWindowArgs()
    a.dtype, a.batch, a.heads, a.rows, a.q_pad = dtype_code(q.dtype), B, H, int(rows), qp
    a.q, a.out, a.k, a.vT, a.cap, a.slot_stride = ptr(q), ptr(out), ptr(k), ptr(vT), cap, H * cap * 64
    a.kv_slot, a.r0, a.kv_len = ptr(keep[2]), ptr(keep[0]), ptr(keep[1])
    a.r0_const, a.kv_max, a.chunk = 0, max(kvl), int(chunk)
    a.scale, a.q_log2 = (1.0 / math.sqrt(64)) if scale is None else scale, int(q_log2)
    a.split_chunk, a.max_splits, a.part_o, a.part_ml = int(split_chunk), int(max_splits), ptr(po), ptr(pm)
    check(lib.hvx_op_attention_window(C.byref(a), stream_ptr()), 'hvx_op_attention_window')
    return out


def attention_window_splits(dtype, batch, heads, rows, kv_max, max_splits=16):
    """(splits, keys per split) that attention_window(split_chunk=0) chooses for a shape: host arithmetic (needs no GPU beyond the CU count, 256 without one)"""
    lib = _lib.load()
    sc = C.c_int32(0)
    n = lib.hvx_op_attention_window_splits(dtype_code(dtype), batch, heads, rows, kv_max, max_splits, C.byref(sc))
    check(0 if n > 0 else -1, 'hvx_op_attention_window_splits')
    return int(n), int(sc.value)


def kv_window_append(k, vT, dk, dv, r0, rows):
    """The cache append of the incremental flow (hvx_op_kv_window_append; csrc/elementwise.hip: kv_window_append_kernel).  k: [2n][H][t_pad][64], vT: [2n][H][64][t_pad]
    (entry 2 i + branch); dk[i]: [2][H][cap_i][64] and dv[i]: [2][H][64][cap_i], session i's caches of both branches; rows [r0[i], r0[i] + rows[i]) of them are written."""
    lib = _lib.load()
    E, H, tp, d = k.shape
    n = len(dk)
    assert E == 2 * n and d == 64 and vT.shape == (E, H, 64, tp) and k.is_contiguous() and vT.is_contiguous()
    for a_, b_ in zip(dk, dv):
        assert a_.dtype == k.dtype and b_.dtype == k.dtype and a_.is_contiguous() and b_.is_contiguous() and a_.shape[0] == 2 and b_.shape == (2, H, 64, a_.shape[2])
    pa = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    ia = lambda v: (C.c_int32 * n)(*[int(x) for x in v])
    bs = (C.c_int64 * n)(*[int(t.shape[1] * t.shape[2] * 64) for t in dk])
    check(lib.hvx_op_kv_window_append(ptr(k), ptr(vT), k.element_size(), H, tp, n, pa(dk), pa(dv), bs, ia([t.shape[2] for t in dk]), ia(r0), ia(rows), stream_ptr()),
          'hvx_op_kv_window_append')


def skinny_gemm(x, w_packed, n_out, bias=None, split_k=1):
    """x: [M][K] (f32/bf16), w_packed: pack_frag([N][K]) -> f32 [M][N]"""
    lib = _lib.load()
    M, K = x.shape
    out = torch.empty(M, n_out, dtype=torch.float32, device=x.device)
    part = torch.empty(max(split_k, 1) * M * n_out, dtype=torch.float32, device=x.device)
    check(lib.hvx_op_skinny_gemm(dtype_code(x.dtype), M, n_out, K, ptr(x), K, ptr(w_packed), ptr(bias), split_k, ptr(part), ptr(out),
                                 n_out, stream_ptr()), 'hvx_op_skinny_gemm')
    return out


def decode_gemm(form, epi, M, N, K, A, W, *, lda=0, split_k=1, bias=None, part=None, out=None, ldo=0, out2=None, ldo2=0,
                kn=0, q_heads=0, kv_heads=0, slot=None, pos0=None, n_new=None, rope_cos=None, rope_sin=None, qbuf=None, kcache=None, vTcache=None,
                max_ctx=0, kv_frag=False, nz=1, w_zs=0, a_zs=0, bias_zs=0, out_zs=0, part_zs=0, n_valid=0, a_norm=False, norm_eps=0.0,
                out_frag=False, w_scale=None, w_scale_zs=0, w_narrow=False, att_o=None, att_ml=None, att_kvlen=None, att_splits=0, att_chunk=0, att_rows_pad=0):
    """One GEMM of the AR decode step, out = A @ W^T through epilogue `epi` (_lib.SK_*), on the kernels `form` names: 0 = the generic kernels
    (csrc/gemm_skinny.hip; A row-major [M][lda]), 1 = the wide-grid kernels (csrc/gemm_dec.hip; A = packing.frag_rows of the rows).  The arguments
    are the fields of csrc/hvx_kernels.h: SkinnyArgs; buffers are the caller's, results land in them.  W: packing.pack_frag of [N][K], or uint8
    packing.pack_frag_fp8 codes with `w_scale` (form 1, SwiGLU).  A shape form 1 does not instantiate raises HvxError: nothing falls through to
    the other kernels.  Form 0, SK_RESID: w_narrow — W = packing.pack_narrow4 of [N][K] —, and with it att_o / att_ml (+ att_kvlen, att_splits, att_chunk,
    att_rows_pad; kn, q_heads, kv_heads, pos0, n_new): A is then not read (it may be None when W tells the dtype) — its rows are combined from the partials an
    ops.llm_attention(..., skip_combine=True) launch left."""
    lib = _lib.load()
    a = DecodeGemmArgs()
    a.form, a.dtype, a.M, a.N, a.K = int(form), dtype_code((A if A is not None else W).dtype), M, N, K
    a.A, a.lda, a.W, a.split_k, a.epi, a.bias, a.part = ptr(A), lda, ptr(W), split_k, int(epi), ptr(bias), ptr(part)
    if out is not None:
        a.out, a.out_f32, a.ldo = ptr(out), int(out.dtype == torch.float32), ldo
    a.out2, a.ldo2 = ptr(out2), ldo2
    a.kn, a.q_heads, a.kv_heads, a.slot, a.pos0, a.n_new = kn, q_heads, kv_heads, ptr(slot), ptr(pos0), ptr(n_new)
    for t in (slot, pos0, n_new):
        assert t is None or t.dtype == torch.int32
    a.rope_cos, a.rope_sin, a.qbuf, a.kcache, a.vTcache = ptr(rope_cos), ptr(rope_sin), ptr(qbuf), ptr(kcache), ptr(vTcache)
    a.max_ctx, a.kv_frag = max_ctx, int(kv_frag)
    a.nz, a.w_zs, a.a_zs, a.bias_zs, a.out_zs, a.part_zs = nz, w_zs, a_zs, bias_zs, out_zs, part_zs
    a.n_valid, a.a_norm, a.norm_eps = n_valid, int(a_norm), norm_eps
    a.a_frag, a.out_frag = int(form == 1), int(out_frag)
    if W.dtype == torch.uint8:
        a.w_fp8, a.w_scale, a.w_scale_zs = 1, ptr(w_scale), w_scale_zs
    assert att_kvlen is None or att_kvlen.dtype == torch.int32
    assert all(t is None or t.dtype == torch.float32 for t in (att_o, att_ml))
    a.w_narrow, a.att_o, a.att_ml, a.att_kvlen = int(w_narrow), ptr(att_o), ptr(att_ml), ptr(att_kvlen)
    a.att_splits, a.att_chunk, a.att_rows_pad = att_splits, att_chunk, att_rows_pad
    check(lib.hvx_op_decode_gemm(C.byref(a), stream_ptr()), 'hvx_op_decode_gemm')


def llm_attention(q, k, vT, out, *, batch, heads, n_rows, kn, q_strides, k_strides, v_strides, v_ld, o_strides=(0, 0, 0, 0), kv_slot=None, kv_len=None,
                  kv_len_const=0, causal=True, pos0=None, n_valid_lo=None, chunk=0, scale=0.125, q_log2=False, n_splits=1, split_chunk=0, n_sub=0, sub_chunk=0,
                  part_o=None, part_ml=None, n_rows_pad=0, skip_combine=False, kv_frag=False, o_frag_kt=0):
    """The LM layers' cache attention as hvx_llm_forward launches it (csrc/hvx_kernels.h: AttnArgs, field for field; csrc/attention.hip: attn_fwd_kernel,
    attn_combine_kernel).  q_strides = (q_bs, q_hs, q_hi, q_lo), k_strides = (k_bs, k_hs), v_strides = (v_bs, v_hs), o_strides = (o_bs, o_hs, o_hi, o_lo), in
    elements.  Buffers are the caller's, results land in them (`out`, or part_o / part_ml alone with skip_combine); nothing is defaulted beyond what
    launch_attention itself applies."""
    lib = _lib.load()
    a = LlmAttnArgs()
    given = [t for t in (q, k, vT, out) if t is not None]
    assert given and all(t.dtype == given[0].dtype for t in given)
    a.dtype, a.batch, a.heads, a.n_rows, a.kn = dtype_code(given[0].dtype), batch, heads, n_rows, kn
    a.q, (a.q_bs, a.q_hs, a.q_hi, a.q_lo) = ptr(q), q_strides
    a.k, (a.k_bs, a.k_hs) = ptr(k), k_strides
    a.vT, (a.v_bs, a.v_hs), a.v_ld = ptr(vT), v_strides, v_ld
    for t in (kv_slot, kv_len, pos0, n_valid_lo):
        assert t is None or t.dtype == torch.int32
    for t in (part_o, part_ml):
        assert t is None or t.dtype == torch.float32
    a.kv_slot, a.kv_len, a.kv_len_const, a.causal, a.pos0, a.n_valid_lo = ptr(kv_slot), ptr(kv_len), kv_len_const, int(causal), ptr(pos0), ptr(n_valid_lo)
    a.chunk, a.scale, a.q_log2 = int(chunk), scale, int(q_log2)
    a.out, (a.o_bs, a.o_hs, a.o_hi, a.o_lo) = ptr(out), o_strides
    a.n_splits, a.split_chunk, a.n_sub, a.sub_chunk = n_splits, split_chunk, n_sub, sub_chunk
    a.part_o, a.part_ml, a.n_rows_pad, a.skip_combine = ptr(part_o), ptr(part_ml), n_rows_pad, int(skip_combine)
    a.kv_frag, a.o_frag_kt = int(kv_frag), o_frag_kt
    check(lib.hvx_op_llm_attention(C.byref(a), stream_ptr()), 'hvx_op_llm_attention')


def reduce_rmsnorm(x, *, M, H, ldx, part=None, split_k=0, part_stride=0, part_zs=0, bias=None, bias_zs=0, gain=None, gain_zs=0, eps=0.0, do_norm=False,
                   y=None, ldy=0, rows_per_z=0, y_frag=False, y_frag_zrows=0):
    """x[m, :] += sum_s part[s][m][:] (+ bias) in place on the fp32 rows x; y[m, :] = dtype(rmsnorm(x[m, :]) * gain), or dtype(x[m, :]) without do_norm
    (csrc/hvx_kernels.h: ReduceNormArgs).  y_frag: the 16-bit y leaves in fragment order (packing.frag_rows)."""
    lib = _lib.load()
    assert x.dtype == torch.float32
    a = ReduceNormArgs()
    a.x, a.ldx, a.part, a.split_k, a.part_stride, a.part_zs = ptr(x), ldx, ptr(part), split_k, part_stride, part_zs
    a.bias, a.bias_zs, a.gain, a.gain_zs, a.eps, a.do_norm = ptr(bias), bias_zs, ptr(gain), gain_zs, eps, int(do_norm)
    a.y, a.ldy, a.dtype = ptr(y), ldy, dtype_code(y.dtype) if y is not None else _lib.F32
    a.M, a.H, a.rows_per_z, a.y_frag, a.y_frag_zrows = M, H, rows_per_z, int(y_frag), y_frag_zrows
    check(lib.hvx_op_reduce_rmsnorm(C.byref(a), stream_ptr()), 'hvx_op_reduce_rmsnorm')


SEQ_PARAM_KEYS = ('top_k', 'top_p', 'win_size', 'rep_thresh')


def seq_sampling_block(seq_params, n_seq, device):
    """dict of four [n_seq] tensors (top_k int32, top_p float32, win_size int32, rep_thresh int32) -> (_lib.SeqSampling, the device tensors it
    points to).  Validated on the host before anything is launched: the kernel can only clamp what it finds in a device array."""
    if sorted(seq_params) != sorted(SEQ_PARAM_KEYS):
        raise ValueError('seq_params needs exactly %s, got %s' % (list(SEQ_PARAM_KEYS), sorted(seq_params)))
    host = {k: torch.as_tensor(seq_params[k]).detach().cpu().reshape(-1) for k in SEQ_PARAM_KEYS}
    for k, v in host.items():
        if v.numel() != n_seq:
            raise ValueError('seq_params[%r] has %d entries for %d sequences' % (k, v.numel(), n_seq))
    if n_seq:
        tk, tp, ws, th = (host[k] for k in SEQ_PARAM_KEYS)
        if int(tk.min()) < 1 or int(tk.max()) > 64:
            raise ValueError('seq_params top_k outside [1, 64]')
        if not bool((tp.double() > 0).all()):
            raise ValueError('seq_params top_p must be positive')
        if int(ws.min()) < 0:
            raise ValueError('seq_params win_size is negative')
        if int(th.min()) < 0:
            raise ValueError('seq_params rep_thresh is negative')
    dev = {k: host[k].to(torch.float32 if k == 'top_p' else torch.int32).contiguous().to(device) for k in SEQ_PARAM_KEYS}
    q = _lib.SeqSampling()
    q.top_k, q.top_p, q.win_size, q.rep_thresh = (dev[k].data_ptr() for k in SEQ_PARAM_KEYS)
    return q, dev


def ras_sample(logp, hist, hist_len, min_len, noise, cursor, *, speech_tokens, top_k=25, top_p=0.8, win_size=10, rep_thresh=1, active=None,
               max_trials=100, seq_params=None, seq_entry=None, seq_heads=None, mixed_entry=None):
    """logp f32 [S][K][V]; hist int32 [S][Hcap]; hist_len/min_len int32 [S]; noise f32 [S][Ncap]; cursor int64 [S] (updated in place)
    -> ids int32 [S][K].  seq_params: dict of four [S] tensors (top_k, top_p, win_size, rep_thresh) — every sequence samples with its own
    values and the scalar keywords are not read (hvx_ras_sample_seq).  seq_entry=True takes that entry point with a NULL block.
    seq_heads: [S] head counts — sequence s samples heads j < clamp(seq_heads[s], 1, K) only, the other ids come back -3
    (hvx_ras_sample_mixed, with or without seq_params).  mixed_entry=True takes that entry point with a NULL heads block."""
    lib = _lib.load()
    S, K, V = logp.shape
    out = torch.empty(S, K, dtype=torch.int32, device=logp.device)
    a = SampleArgs()
    a.n_seq, a.head_k, a.vocab, a.speech_tokens = S, K, V, speech_tokens
    a.logp, a.logp_seq_stride, a.logp_head_stride = ptr(logp), K * V, V
    a.hist, a.hist_seq_stride, a.hist_len = ptr(hist), hist.shape[1], ptr(hist_len)
    a.min_len, a.active = ptr(min_len), ptr(active)
    a.top_k, a.top_p, a.win_size, a.rep_thresh = top_k, top_p, win_size, rep_thresh
    a.noise, a.noise_seq_stride, a.noise_len = ptr(noise), noise.shape[1], noise.shape[1]
    a.cursor, a.out_ids, a.max_trials = ptr(cursor), ptr(out), max_trials
    if seq_heads is not None or mixed_entry:
        q = keep = None
        if seq_params is not None:
            q, keep = seq_sampling_block(seq_params, S, logp.device)
        hd = None
        if seq_heads is not None:
            heads = torch.as_tensor(seq_heads).detach().reshape(-1).to(torch.int32).contiguous().to(logp.device)
            if heads.numel() != S:
                raise ValueError('seq_heads has %d entries for %d sequences' % (heads.numel(), S))
            hd = _lib.SeqHeads()
            hd.head_k = heads.data_ptr()
        check(lib.hvx_ras_sample_mixed(C.byref(a), None if q is None else C.byref(q), None if hd is None else C.byref(hd), stream_ptr()), 'hvx_ras_sample_mixed')
    elif seq_params is not None:
        q, keep = seq_sampling_block(seq_params, S, logp.device)      # (`keep`: the arrays live until the launch is enqueued; the allocator reuses them in stream order)
        check(lib.hvx_ras_sample_seq(C.byref(a), C.byref(q), stream_ptr()), 'hvx_ras_sample_seq')
    elif seq_entry:
        check(lib.hvx_ras_sample_seq(C.byref(a), None, stream_ptr()), 'hvx_ras_sample_seq')
    else:
        check(lib.hvx_ras_sample(C.byref(a), stream_ptr()), 'hvx_ras_sample')
    return out


def resample_linear(x, t_out):
    """F.interpolate(x, size=t_out, mode='linear') for a float32 (..., T) tensor on the device (the `speed` knob of the synthesis calls)"""
    lib = _lib.load()
    x = x.to(torch.float32).contiguous()
    t_in = x.shape[-1]
    rows = x.numel() // max(t_in, 1)
    y = torch.empty(*x.shape[:-1], t_out, dtype=torch.float32, device=x.device)
    check(lib.hvx_op_resample_linear(ptr(x), rows, t_in, ptr(y), t_out, stream_ptr()), 'hvx_op_resample_linear')
    return y


def resample_sinc(x, taps_dev, orig, new, width):
    """torchaudio.transforms.Resample (sinc_interp_hann) of the rows of a float32 (rows, L) device tensor or view (unit stride along L, any row stride):
    taps_dev = the device table [2 * width + orig][new] of packing.sinc_resample_taps (its taps transposed: the phases of a tap contiguous); orig / new = the
    rates over their gcd.  -> (rows, ceil(new * L / orig)).  csrc/resample.hip; a geometry the launcher cannot tile raises HvxError."""
    lib = _lib.load()
    assert x.dim() == 2 and x.dtype == torch.float32 and (x.shape[1] <= 1 or x.stride(1) == 1), (x.shape, x.dtype, x.stride())
    assert taps_dev.dtype == torch.float32 and taps_dev.is_contiguous() and tuple(taps_dev.shape) == (2 * width + orig, new), taps_dev.shape
    rows, L = x.shape
    out = torch.empty(rows, sinc_resample_len(L, orig, new), dtype=torch.float32, device=x.device)
    check(lib.hvx_op_resample_sinc(ptr(x), rows, L, x.stride(0) if rows > 1 else L, ptr(taps_dev), orig, new, width, ptr(out), out.shape[1], out.shape[1],
                                   stream_ptr()), 'hvx_op_resample_sinc')
    return out


def mel_append_block(t_len, covered, caches, cache_fill):
    """the host argument arrays of hvx_op_mel_cache_append / hvx_cfm_solve_stream_batch for cache planes `caches` (each a contiguous fp32 (mel, ld_i) tensor):
    (t_len, covered, cache pointers, cache_ld, cache_fill) as ctypes arrays"""
    n = len(caches)
    if not (len(t_len) == len(covered) == len(cache_fill) == n):
        raise ValueError('t_len, covered, caches and cache_fill must have one entry per session')
    for c in caches:
        assert c.dim() == 2 and c.dtype == torch.float32 and c.is_contiguous(), (c.shape, c.dtype, c.stride())
    ia = lambda v: (C.c_int32 * max(n, 1))(*[int(x) for x in v])
    pa = (C.c_void_p * max(n, 1))(*[c.data_ptr() for c in caches])
    return ia(t_len), ia(covered), pa, ia([c.shape[1] for c in caches]), ia(cache_fill)


def mel_cache_append(x, t_len, covered, caches, cache_fill):
    """Frames [covered[i], t_len[i]) of all mel rows of x[i] — x a float32 (n, mel, t_max) device tensor — are copied into session i's cache plane `caches[i]`
    ((mel, ld_i) float32, contiguous) from column cache_fill[i] on; nothing else of a plane is touched.  An append that would overflow its plane,
    covered[i] > t_len[i] or no session at all raises HvxError before anything is launched.  csrc/elementwise.hip: mel_cache_append_kernel."""
    lib = _lib.load()
    assert x.dim() == 3 and x.dtype == torch.float32 and x.is_contiguous(), (x.shape, x.dtype)
    if x.shape[0] != len(caches):
        raise ValueError('x holds %d sessions, %d cache planes given' % (x.shape[0], len(caches)))
    tl, cov, pa, ld, fill = mel_append_block(t_len, covered, caches, cache_fill)
    check(lib.hvx_op_mel_cache_append(ptr(x), len(caches), x.shape[1], x.shape[2], tl, cov, pa, ld, fill, stream_ptr()), 'hvx_op_mel_cache_append')
