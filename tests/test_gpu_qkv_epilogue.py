"""The fused QKV epilogue of the implicit-GEMM kernels (csrc/gemm_epilogue.h: EPI_QKV_DIT), one launch at a time against float64, through ops.qkv_gemm
(hvx_op_gemm with epi = 1): bias, interleaved-pair RoPE on channels [0, 64) of q and k (head 0 only), q * q_scale, and the scatter of a [T][3 heads 64] tile
into q, k [b][head][t_pad][64] and V^T [b][head][64][t_pad].  The model tests see this store only through 22 blocks of attention and residual adds.

Every case builds its operands on the CPU in the operand type, computes the reference in float64 FROM THOSE ROUNDED VALUES, pre-fills q, k and V^T with a
sentinel that is exact in bf16, fp16 and fp32, and compares each kernel form with the reference (never with another form).  Every element with t < M is held
to its bound; every element with t >= M — rows [M, t_pad) of q and k, columns [M, t_pad) of V^T, in every batch entry and head — must still hold the sentinel
bit for bit.  The RoPE tables have exactly M rows: position x a geometric frequency ladder, as flow.dit_rope_tables builds them.

The five compiled forms and the shapes that reach them (csrc/gemm_tiled.hip: launch_gemm / launch_t, csrc/gemm_big.hip: launch_gemm_big):
  a   gemm_tiled 64 x 64 (WN = 32: two lanes per row, V^T 16 time steps per lane): fewer than 256 tiles of 128 x 128; bf16 and fp32; the DiT call (bias + RoPE +
      q_scale) and the Matcha call (no bias, no table, q_scale 0)
  b   gemm_tiled 128 x 128 (WN = 64): 52 x 5 = 260 tiles, K = 96 (no multiple of 64: the 256-tile form is not eligible), N = 576: the second wave column of the last
      column tile lies past N (wave_ok false); a pad of 37 columns and one wider than a tile (101)
  c   gemm_big, bf16, at the default gemm_big_min_tiles: 12 x 12 = 144 tiles in column groups of 4; 2833 % 32 = 17: the scalar V^T tail with more than 16 rows
  d   gemm_big, bf16, gemm_big_min_tiles = 1: N = 576 = 2.25 column tiles of 256; 300 % 32 = 12 (tail of fewer than 16 rows, t_pad = 304: no multiple of 64), and
      M = 320: no tail at all
  e   gemm_big with fp16 operands (every size takes it): bf16 q / k / V^T, and qkv_f16: fp16 q / k / V^T

Bounds, derived from the number formats and not from what a device returned.  U = 2^-24 (fp32 unit roundoff), x = A W^T + bias and mag = |A| |W|^T + |bias| in
float64:
  accumulator + bias     e_x = K U mag + 2 U |x|: an fp32 sum of K exact 16-bit x 16-bit products in any order, plus the bias add.  fp32 operands:
                         e_x = (K + 2) U mag (the products are themselves rounded)
  rotation               out = x c -+ p s, p the pair partner:  e = |c| e_x + |s| e_p + 2 U (|x c| + |p s|)  (two products and a sum, each rounded once)
  q_scale                e <- q_scale e + U |ref|
  stored value           fp32: e;   bf16: 2^-8 |ref| + (1 + 2^-8) e;   fp16: 2^-11 |ref| + (1 + 2^-11) e + 2^-25 (the subnormal range) — the rounding acts
                         on the fp32 value, not on ref: hence the factors 1 + 2^-8, 1 + 2^-11
The input scale keeps everything far from the fp16 limit; saturation has its own test.

test_fp32_emulation_stays_inside_the_bounds (CPU) runs an fp32 emulation of the arithmetic — products accumulated in fp32 k-step by k-step, the epilogue in
fp32, one rounding to the storage type — through the same bound functions for the same seeds and every case: the bounds hold for a correct implementation
before a device is involved.
"""
import ctypes as C
import functools

import pytest
import torch

from flowmirror_hydravox_amd import _lib, ops

gpu = pytest.mark.gpu

U = 2.0 ** -24
SENT = -77.0                                                       # exact in bf16, fp16 and fp32
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
QS = float(torch.tensor(0.125 * 1.4426950408889634, dtype=F32))    # the DiT's q_scale (dim_head^-0.5 in log2 units), as the fp32 value the kernel receives

# name: (heads, K, M, B, t_pad, ((operand type, q / k / V^T type), ...), (variants), options)
CASES = {
    'a': (2, 64, 203, 2, 256, ((BF16, BF16), (F32, F32)), ('dit', 'plain'), {}),
    'b_pad37': (3, 96, 6619, 1, 6656, ((BF16, BF16), (F32, F32)), ('dit',), {}),
    'b_pad101': (3, 96, 6619, 1, 6720, ((BF16, BF16), (F32, F32)), ('dit',), {}),
    'c': (16, 128, 2833, 1, 2880, ((BF16, BF16),), ('dit',), {}),
    'd_tail12': (3, 64, 300, 2, 304, ((BF16, BF16),), ('dit',), dict(gemm_big_min_tiles=1)),
    'd_no_tail': (3, 64, 320, 2, 384, ((BF16, BF16),), ('dit',), dict(gemm_big_min_tiles=1)),
    'e': (4, 128, 203, 2, 256, ((F16, BF16), (F16, F16)), ('dit',), {}),
}
ROPE_HEAD0_CASES = ('a', 'c', 'e')


def _randn(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _rope_tables(M):
    inv_freq = 10000.0 ** (-torch.arange(32, dtype=torch.float64) / 32)
    ang = torch.arange(M, dtype=torch.float64)[:, None] * inv_freq[None, :]
    return ang.cos().float().contiguous(), ang.sin().float().contiguous()


@functools.lru_cache(maxsize=4)
def _operands(name, dt):
    heads, K, M, B, _, _, _, _ = CASES[name]
    N, seed = 3 * heads * 64, 1000 * (sorted(CASES).index(name) + 1)
    A = _randn((B, M, K), seed + 1).to(dt)
    W = _randn((N, K), seed + 2, K ** -0.5).to(dt)
    bias = _randn((N,), seed + 3, 0.5)
    return A, W, bias


def _variant(name, variant, bias):
    """-> bias, (cos, sin) or None, q_scale"""
    if variant == 'plain':
        return None, None, 0.0
    return bias, _rope_tables(CASES[name][2]), QS


def _rotate(x, cos, sin):
    """interleaved-pair RoPE of [..., M, 64] values by the table rows [M][32], in the dtype of x"""
    c, s = cos.to(x.dtype), sin.to(x.dtype)
    ev, od = x[..., 0::2], x[..., 1::2]
    return torch.stack([ev * c - od * s, od * c + ev * s], dim=-1).flatten(-2)


def _reference(A, W, bias, rope, q_scale, heads):
    """float64 value and fp32-arithmetic bound e of every element, as [B][M][3][heads][64]"""
    a, w = A.double(), W.double()
    B, M, K = a.shape
    x, mag = a @ w.t(), a.abs() @ w.abs().t()
    if bias is not None:
        x, mag = x + bias.double(), mag + bias.double().abs()
    e = (K + 2) * U * mag if A.dtype == F32 else K * U * mag + 2 * U * x.abs()
    x, e = x.view(B, M, 3, heads, 64).clone(), e.view(B, M, 3, heads, 64).clone()
    if rope is not None:
        c, s = rope[0].double()[:, None, :], rope[1].double()[:, None, :]            # [M][1][32] against head 0 of q and k: [B][M][2][64]
        h0, e0 = x[:, :, :2, 0].clone(), e[:, :, :2, 0].clone()
        ev, od, eev, eod = h0[..., 0::2], h0[..., 1::2], e0[..., 0::2], e0[..., 1::2]
        x[:, :, :2, 0] = _rotate(h0, rope[0][:, None, :], rope[1][:, None, :])
        e[:, :, :2, 0] = torch.stack([c.abs() * eev + s.abs() * eod + 2 * U * ((ev * c).abs() + (od * s).abs()),
                                      c.abs() * eod + s.abs() * eev + 2 * U * ((od * c).abs() + (ev * s).abs())], dim=-1).flatten(-2)
    if q_scale != 0.0:
        x[:, :, 0] = x[:, :, 0] * q_scale
        e[:, :, 0] = q_scale * e[:, :, 0] + U * x[:, :, 0].abs()
    return x, e


def _store_bound(ref, e, qdt):
    if qdt == F32:
        return e
    if qdt == BF16:
        return 2.0 ** -8 * ref.abs() + (1 + 2.0 ** -8) * e
    return 2.0 ** -11 * ref.abs() + (1 + 2.0 ** -11) * e + 2.0 ** -25


def _emulate(A, W, bias, rope, q_scale, heads, qdt):
    """the kernels' arithmetic in fp32: products accumulated k-step (32 columns) by k-step, bias, rotation, q_scale, ONE rounding to the storage type
    (fp16 saturated) -> [B][M][3][heads][64]"""
    a, w = A.float(), W.float()
    B, M, K = a.shape
    acc = torch.zeros(B, M, w.shape[0])
    for k in range(0, K, 32):
        acc += a[..., k:k + 32] @ w[:, k:k + 32].t()
    if bias is not None:
        acc = acc + bias
    x = acc.view(B, M, 3, heads, 64).clone()
    if rope is not None:
        x[:, :, :2, 0] = _rotate(x[:, :, :2, 0].clone(), rope[0][:, None, :], rope[1][:, None, :])
    if q_scale != 0.0:
        x[:, :, 0] = x[:, :, 0] * torch.tensor(q_scale, dtype=F32)
    return (x.clamp(-65504.0, 65504.0) if qdt == F16 else x).to(qdt)


def _layout(v, t_pad, fill):
    """[B][M][3][heads][64] -> q, k [B][heads][t_pad][64] and V^T [B][heads][64][t_pad], `fill` wherever t >= M"""
    B, M, _, H, _ = v.shape
    q, k, vT = (torch.full(s, fill, dtype=v.dtype) for s in ((B, H, t_pad, 64), (B, H, t_pad, 64), (B, H, 64, t_pad)))
    q[:, :, :M], k[:, :, :M], vT[..., :M] = v[:, :, 0].permute(0, 2, 1, 3), v[:, :, 1].permute(0, 2, 1, 3), v[:, :, 2].permute(0, 2, 3, 1)
    return q, k, vT


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _check(what, got, ref, bound, mask=None):
    """every element with t < M inside its bound (NaN fails), the sentinel's bits at every other element; prints the worst error / bound ratio first"""
    got = got.detach().cpu()
    if mask is not None:
        rest = _bits(got)[~mask]
        want = _bits(torch.tensor([SENT], dtype=got.dtype))[0]
        assert bool((rest == want).all()), '%s: %d elements with t >= M were written' % (what, int((rest != want).sum()))
        got, ref, bound = got[mask], ref[mask], bound[mask]
    err = (got.double() - ref).abs()
    ok = err <= bound
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print('%s: %d elements, worst error / bound %.3f' % (what, err.numel(), worst))
    assert err.numel() > 0 and bool(ok.all()), '%s: %d of %d elements outside the bound, worst error / bound %.3f' % (what, int((~ok).sum()), ok.numel(), worst)
    return worst


def _dev(t):
    return None if t is None else t.to('cuda')


def _launch(name, A, W, bias, rope, q_scale, qdt):
    """one launch into sentinel-filled buffers -> (q, k, vT) on the CPU"""
    heads, _, _, B, t_pad, _, _, opts = CASES[name]
    q, k, vT = (torch.full(s, SENT, dtype=qdt, device='cuda') for s in ((B, heads, t_pad, 64), (B, heads, t_pad, 64), (B, heads, 64, t_pad)))
    with _lib.option_scope(**opts):
        ops.qkv_gemm(_dev(A), _dev(W), _dev(bias), heads=heads, t_pad=t_pad, rope=None if rope is None else tuple(_dev(t) for t in rope), q_scale=q_scale,
                     qkv_dtype=qdt, q=q, k=k, vT=vT)
    torch.cuda.synchronize()
    return q.cpu(), k.cpu(), vT.cpu()


def _forms(name):
    return [pytest.param(name, odt, qdt, v, id='%s-%s-%s-%s' % (name, str(odt)[6:], str(qdt)[6:], v)) for odt, qdt in CASES[name][5] for v in CASES[name][6]]


ALL_FORMS = [p for name in CASES for p in _forms(name)]


@gpu
@pytest.mark.parametrize('name,odt,qdt,variant', ALL_FORMS)
def test_qkv_epilogue_lands_every_element_and_nothing_else(name, odt, qdt, variant):
    """Cases a - e of the module docstring.  In cases a, c and e the launch is repeated without the RoPE tables: heads >= 1 of q and k and all of V^T must come
    back bit-identical, head 0 of q and k must differ — RoPE reaches head 0 only, whatever the bounds say."""
    heads, K, M, B, t_pad, _, _, _ = CASES[name]
    A, W, bias0 = _operands(name, odt)
    bias, rope, q_scale = _variant(name, variant, bias0)
    ref, e = _reference(A, W, bias, rope, q_scale, heads)
    refs, bounds, masks = _layout(ref, t_pad, 0.0), _layout(_store_bound(ref, e, qdt), t_pad, 0.0), _layout(torch.ones_like(ref), t_pad, 0.0)
    got = _launch(name, A, W, bias, rope, q_scale, qdt)
    tag = 'qkv %s M=%d K=%d heads=%d B=%d t_pad=%d %s->%s %s ' % (name, M, K, heads, B, t_pad, str(odt)[6:], str(qdt)[6:], variant)
    for what, g_, r_, b_, m_ in zip(('q', 'k', 'vT'), got, refs, bounds, masks):
        _check(tag + what, g_, r_, b_, m_ > 0)
    if rope is not None and name in ROPE_HEAD0_CASES:
        q0, k0, v0 = _launch(name, A, W, bias, None, q_scale, qdt)
        assert torch.equal(_bits(v0), _bits(got[2])), tag + 'V^T depends on the RoPE tables'
        for what, g0, g1 in (('q', q0, got[0]), ('k', k0, got[1])):
            assert torch.equal(_bits(g0[:, 1:]), _bits(g1[:, 1:])), tag + what + ': a head other than 0 depends on the RoPE tables'
            # position 0 has angle 0 (c = 1, s = 0: the same bits); every later row of head 0 is rotated by its own angles
            assert torch.equal(_bits(g0[:, 0, 0]), _bits(g1[:, 0, 0])), tag + what + ': row 0 is rotated by another row\'s angle'
            changed = (_bits(g0[:, 0, 1:M]) != _bits(g1[:, 0, 1:M])).any(dim=-1)
            assert bool(changed.all()), tag + what + ': %d rows of head 0 are not rotated' % int((~changed).sum())


@gpu
def test_qkv_f16_saturates_instead_of_overflowing():
    """qkv_f16 (case e's shape): a bias that drives V^T past the fp16 limit comes back clipped at +-65504 and finite (csrc/hvx_device.h: f32_to_f16_sat), q and k keep
    their bounds, the padding keeps the sentinel."""
    name = 'e'
    heads, K, M, B, t_pad, _, _, _ = CASES[name]
    A, W, bias0 = _operands(name, F16)
    bias = bias0.clone()
    sign = torch.where(torch.arange(heads) % 2 == 0, 1.0, -1.0)
    bias.view(3, heads, 64)[2] = (70000.0 * sign)[:, None]
    rope = _rope_tables(M)
    ref, e = _reference(A, W, bias, rope, QS, heads)
    refs, bounds, masks = _layout(ref, t_pad, 0.0), _layout(_store_bound(ref, e, F16), t_pad, 0.0), _layout(torch.ones_like(ref), t_pad, 0.0)
    q, k, vT = _launch(name, A, W, bias, rope, QS, F16)
    _check('qkv f16 saturation q', q, refs[0], bounds[0], masks[0] > 0)
    _check('qkv f16 saturation k', k, refs[1], bounds[1], masks[1] > 0)
    assert bool((refs[2][..., :M].abs() > 65504.0 + 1000.0).all())                 # (every V value does lie past the limit)
    want = torch.full((B, heads, 64, t_pad), SENT, dtype=F16)
    want[..., :M] = (65504.0 * sign).to(F16)[None, :, None, None]
    assert bool(torch.isfinite(vT.float()).all()) and torch.equal(_bits(vT), _bits(want))


# ================================================================================================================================================
# refusals: what the kernels assume and do not check is an error of the call, before anything is launched
# ================================================================================================================================================
def _refusal_args(dt, qdt, alter, device):
    """hvx_gemm_args of a small legal launch (heads 4, K = 128, M = 203, t_pad = 256, bias, RoPE, q_scale) with one field altered -> (args, the buffers to keep alive)"""
    heads, K, M, B, t_pad = 4, 128, 203, 2, 256
    N = 3 * heads * 64
    x, w = torch.zeros(B, M, K, dtype=dt, device=device), torch.zeros(N, K, dtype=dt, device=device)
    spare = torch.zeros(N + M * 32 + 16, dtype=F32, device=device)
    bias, cos, sin = torch.zeros(N, dtype=F32, device=device), torch.zeros(M, 32, dtype=F32, device=device), torch.zeros(M, 32, dtype=F32, device=device)
    # (generous buffers: a launch that should have been refused would still stay inside them)
    q, k, vT = (torch.full(s, SENT, dtype=qdt, device=device) for s in ((B, heads, t_pad, 64), (B, heads, t_pad, 64), (B, heads, 64, t_pad)))
    a, _ = ops.qkv_gemm_args(x, w, bias, heads=heads, t_pad=t_pad, rope=(cos, sin), q_scale=QS, qkv_dtype=qdt, q=q, k=k, vT=vT)
    alter(a, dict(q=q, k=k, vT=vT, spare=spare, esz=q.element_size()))
    return a, (x, w, spare, bias, cos, sin, q, k, vT)


def _set(**kv):
    return lambda a, env: [setattr(a, k, v) for k, v in kv.items()]


def _shift(field, nbytes, from_spare=False):
    """move a pointer off its 16-byte alignment (bias / tables: into a spare buffer of their size + 4 floats)"""
    def alter(a, env):
        base = env['spare'].data_ptr() if from_spare else env[field].data_ptr()
        setattr(a, field, base + nbytes)
    return alter


# (id, operand type, q / k / V^T type, options, the alteration, a word of the error text)
REFUSALS = [
    ('t_pad_below_M', BF16, BF16, {}, _set(t_pad=200), 'shorter than M'),
    ('t_pad_below_M_f32', F32, F32, {}, _set(t_pad=200), 'shorter than M'),
    ('t_pad_row_pitch_bf16', BF16, BF16, {}, _set(t_pad=204), 'multiple of 16 bytes'),
    ('t_pad_row_pitch_f16', F16, F16, {}, _set(t_pad=252), 'multiple of 16 bytes'),
    ('t_pad_row_pitch_f32', F32, F32, {}, _set(t_pad=206), 'bad QKV geometry'),
    ('null_q', BF16, BF16, {}, _set(q=None), 'null q, k or vT'),
    ('null_k', F32, F32, {}, _set(k=None), 'null q, k or vT'),
    ('null_vT', F16, F16, {}, _set(vT=None), 'null q, k or vT'),
    ('cos_without_sin', BF16, BF16, {}, _set(rope_sin=None), 'one RoPE table'),
    ('sin_without_cos', F32, F32, {}, _set(rope_cos=None), 'one RoPE table'),
    ('qkv_f16_bf16_operands', BF16, BF16, {}, _set(qkv_f16=1), 'qkv_f16 needs fp16 operands'),
    ('qkv_f16_f32_operands', F32, F32, {}, _set(qkv_f16=1), 'qkv_f16 needs fp16 operands'),
    ('x3', F32, F32, {}, _set(x3=1), 'plain operands only'),
    ('plane_pairs', F32, F32, {}, _set(a_planes=1, w_planes=1), 'plain operands only'),
    ('a_planes_alone', F32, F32, {}, _set(a_planes=1), 'plain operands only'),
    ('heads_do_not_match_N', BF16, BF16, {}, _set(heads=3), 'bad QKV geometry'),
    ('groups', BF16, BF16, {}, _set(groups=2), 'bad QKV geometry'),
    ('unknown_epi', BF16, BF16, {}, _set(epi=2), 'epi 2'),
    ('misaligned_q', BF16, BF16, {}, _shift('q', 8), '16-byte aligned'),
    ('misaligned_k', F32, F32, {}, _shift('k', 8), '16-byte aligned'),
    ('misaligned_vT', F16, F16, {}, _shift('vT', 8), '16-byte aligned'),
    ('misaligned_bias_f16', F16, BF16, {}, _shift('bias', 4, True), 'bias and RoPE tables must be 16-byte aligned'),
    ('misaligned_bias_big_bf16', BF16, BF16, dict(gemm_big_min_tiles=1), _shift('bias', 8, True), 'bias and RoPE tables must be 16-byte aligned'),
    ('misaligned_cos_f16', F16, F16, {}, _shift('rope_cos', 4, True), 'bias and RoPE tables must be 16-byte aligned'),
    ('misaligned_sin_f16', F16, F16, {}, _shift('rope_sin', 12, True), 'bias and RoPE tables must be 16-byte aligned'),
]


@gpu
@pytest.mark.parametrize('rid,dt,qdt,opts,alter,text', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_launcher_refuses_what_the_kernels_assume(rid, dt, qdt, opts, alter, text):
    """Each call returns -1 with its reason and launches nothing: the sentinel-filled q, k and V^T are untouched."""
    lib = _lib.load()
    a, keep = _refusal_args(dt, qdt, alter, 'cuda')
    with _lib.option_scope(**opts):
        rc = lib.hvx_op_gemm(C.byref(a), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1, rid
    assert text in lib.hvx_last_error().decode(), (rid, lib.hvx_last_error())
    want = _bits(torch.tensor([SENT], dtype=qdt))[0]
    for t in keep[-3:]:
        assert bool((_bits(t.cpu()) == want).all()), rid


# ================================================================================================================================================
# the bounds, without a device
# ================================================================================================================================================
@pytest.mark.parametrize('name,odt,qdt,variant', ALL_FORMS)
def test_fp32_emulation_stays_inside_the_bounds(name, odt, qdt, variant):
    heads = CASES[name][0]
    A, W, bias0 = _operands(name, odt)
    bias, rope, q_scale = _variant(name, variant, bias0)
    ref, e = _reference(A, W, bias, rope, q_scale, heads)
    emu = _emulate(A, W, bias, rope, q_scale, heads, qdt)
    worst = _check('emulation %s %s->%s %s' % (name, str(odt)[6:], str(qdt)[6:], variant), emu, ref, _store_bound(ref, e, qdt))
    assert worst > 0.0                                                             # (the emulation is not the reference itself)
