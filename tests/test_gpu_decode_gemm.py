"""The decode GEMMs, operator by operator against float64: every epilogue of csrc/gemm_dec.hip (form 1: fragment-order activations, LDS weight ring, XCD-aware
grid) and of the generic kernels of csrc/gemm_skinny.hip (form 0) through ops.decode_gemm, and the split-K reduce + RMSNorm that feeds them through
ops.reduce_rmsnorm.  tests/test_gpu_fullsize.py holds the two forms to each other through a whole model; here each launch is held to the mathematics.

Every case builds bf16 operands on the CPU, computes the reference in float64 FROM THOSE bf16 VALUES, and compares each form with it separately (the forms
sum in different orders: they are never compared with each other).  Operands and fragment-order results are laid out / decoded with packing.frag_rows,
kfrag, vfrag and their inverses (tests/test_host_cpu.py holds those to the index formulas), not with the kernels' own addressing.  No element is left out
of a comparison and no element may miss its bound.

Bounds (derived from the number formats, U = 2^-24 the fp32 unit roundoff, UB = 2^-8 one bf16 rounding to nearest, mag = |A| @ |W|^T in float64):

  fp32 outputs (split-K partials, SK_STORE, the SK_RESID stream):   |got - ref| <= K U mag + 2 U |ref|
      an fp32 sum of K exact bf16 x bf16 products in any order, plus the rounding of the epilogue's add.
  bf16 outputs:   |got - ref| <= UB |ref| + (1 + UB) e,   e = the fp32 bound of the value that is rounded (the factor 1 + UB: the rounding acts on the fp32
      value, not on ref), carried through the epilogue's float64 Jacobian:
      fused RMSNorm (a_norm):  g = acc inv;  e_g = inv K U mag + (d_r + U) |g|,  d_r = (K / 2 + 1) U + 2^-22: the relative error of rsqrt(ssq / K + eps) from an
                    fp32 sum of K squares (all terms positive: relative error K U, halved by the square root), two roundings, and a 2-ulp rsqrt;
      SK_QKV_ROPE:  x = acc inv + bias: e_x = e_g + 2 U |x|;  out = x c -+ p s (p the rotate-half partner):  e = |c| e_x + |s| e_p + 2 U (|x c| + |p s|)
                    (the last term: the two products and the sum of the rotation itself, each rounded once); v heads: e = e_x;
      SK_SWIGLU:    f = g sigmoid(g) u:  e = |df/dg| e_g + |df/du| e_u + 2 U |f| + 4 * 2^-23 |f|  — the two fp32 products, and the allowance for the
                    hardware rcp / exp2 approximations (1 ulp each, plus the roundings of the exponent's argument and of 1 + e^-g);
      16-bit copy of SK_RESID: e = the fp32 bound of the stream.
  reduce_rmsnorm: x' = x + sum_s part_s + bias in fp32: e_x = (S + 2) U (|x| + sum_s |part_s| + |bias|); y = bf16(x'): UB |ref| + (1 + UB) e_x; with the norm,
      y = bf16(gain * bf16(x' inv)) (two bf16 roundings, as Qwen2's RMSNorm casts before the gain):  |ref| ((1 + UB)^2 - 1 + 1.02 (d_r(H) + 2 U + |e_x|_2 / |x'|_2))
      + 1.02 |gain| inv e_x.

test_fp32_emulation_stays_inside_the_bounds (CPU) runs an fp32 emulation of the kernels' arithmetic — the bf16 products accumulated in fp32 k-step by
k-step, the epilogue in fp32, one rounding to bf16 — through the same bounds: they hold without a device, for the seeds used here.
"""
import functools

import pytest
import torch

from flowmirror_hydravox_amd import _lib, ops, packing
from flowmirror_hydravox_amd._lib import SK_PARTIAL, SK_STORE, SK_QKV_ROPE, SK_SWIGLU, SK_RESID

gpu = pytest.mark.gpu

K = 896                          # the only K gemm_dec instantiates (28 k-steps); SK_PARTIAL: split_k x 608
U = 2.0 ** -24
UB = 2.0 ** -8
ROWS = (33, 64, 65, 100, 129, 256)      # one chunk whose last three waves re-read the last row tile; an exact chunk; chunks of a single row; a partial tile; four chunks
SENT = -77.0                     # exact in bf16
EPS = 1e-6


def _randn(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _bf(shape, seed, scale=1.0):
    return _randn(shape, seed, scale).to(torch.bfloat16)


def _prod(A, W):
    """float64 product of bf16 operands, and |A| @ |W|^T"""
    a, w = A.double(), W.double()
    return a @ w.t(), a.abs() @ w.abs().t()


def _acc32(A, W):
    """the kernels' sum, emulated: exact bf16 x bf16 products accumulated in fp32, k-step (32 columns) by k-step"""
    a, w = A.float(), W.float()
    acc = torch.zeros(A.shape[0], W.shape[0])
    for k in range(0, A.shape[1], 32):
        acc += a[:, k:k + 32] @ w[:, k:k + 32].t()
    return acc


def _d_r(n):
    return (n / 2 + 1) * U + 2.0 ** -22


def _inv_rms(A, dt):
    x = A.to(dt)
    return torch.rsqrt((x * x).sum(1, keepdim=True) / A.shape[1] + EPS)


def _f32_bound(kk, mag, ref):
    return kk * U * mag + 2 * U * ref.abs()


def _bf_bound(ref, e):
    return UB * ref.abs() + (1 + UB) * e


def _check(what, got, ref, bound, mask=None):
    """every element inside its bound (NaN fails), the sentinel intact outside `mask`; prints the worst error / bound ratio first"""
    got = got.detach().double().cpu().reshape(ref.shape)
    err = (got - ref).abs()
    ok = err <= bound
    if mask is not None:
        rest = got[~mask]
        assert bool((rest == SENT).all()), '%s: %d elements outside the result were written' % (what, int((rest != SENT).sum()))
        ok, err, bound = ok[mask], err[mask], bound[mask]
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print('%s: %d elements, worst error / bound %.3f' % (what, err.numel(), worst))
    assert err.numel() > 0 and bool(ok.all()), '%s: %d of %d elements outside the bound, worst error / bound %.3f' % (what, int((~ok).sum()), ok.numel(), worst)


def _dev(t):
    return None if t is None else t.to('cuda')


def _sent(n, dtype):
    return torch.full((n,), SENT, dtype=dtype, device='cuda')


# ================================================================================================================================================
# SK_QKV_ROPE
# ================================================================================================================================================
def _rope_tables(n_pos):
    inv_freq = 10000.0 ** (-torch.arange(32, dtype=torch.float64) / 32)
    ang = torch.arange(n_pos, dtype=torch.float64)[:, None] * inv_freq[None, :]
    return ang.cos().float().contiguous(), ang.sin().float().contiguous()


def _qkv_values(acc, inv, bias, cos_r, sin_r, n_rot, dt):
    """acc [M][N] in the projection's own (unpermuted) column order -> rotated q | k | plain v, in dt.  cos_r / sin_r: [M][32] table rows of each row's position;
    the first n_rot heads (q and k) are rotated: d < 32 -> x c - x[d + 32] s, d >= 32 -> x c + x[d - 32] s  (HF Qwen2 rotate_half)"""
    M = acc.shape[0]
    x = (acc.to(dt) * inv.to(dt) + bias.to(dt)).view(M, -1, 64)
    c, s = cos_r.to(dt)[:, None, :], sin_r.to(dt)[:, None, :]
    lo, hi = x[:, :n_rot, :32], x[:, :n_rot, 32:]
    rot = torch.cat([lo * c - hi * s, hi * c + lo * s], dim=2)
    return torch.cat([rot, x[:, n_rot:]], dim=1).reshape(M, -1)


def _qkv_bound(acc, mag, inv, bias, cos_r, sin_r, n_rot, a_norm):
    M = acc.shape[0]
    g = acc * inv
    x = g + bias.double()
    e_x = (inv * K * U * mag + ((_d_r(K) + U) * g.abs() if a_norm else 0.0) + 2 * U * x.abs()).view(M, -1, 64)
    xv = x.view(M, -1, 64)
    c, s = cos_r.double().abs()[:, None, :], sin_r.double().abs()[:, None, :]
    elo, ehi, alo, ahi = e_x[:, :n_rot, :32], e_x[:, :n_rot, 32:], xv[:, :n_rot, :32].abs(), xv[:, :n_rot, 32:].abs()
    e_rot = torch.cat([c * elo + s * ehi + 2 * U * (alo * c + ahi * s), c * ehi + s * elo + 2 * U * (ahi * c + alo * s)], dim=2)
    e = torch.cat([e_rot, e_x[:, n_rot:]], dim=1).reshape(M, -1)
    ref = _qkv_values(acc, inv, bias, cos_r, sin_r, n_rot, torch.float64)
    return ref, _bf_bound(ref, e)


@functools.lru_cache(maxsize=2)
def _qkv_operands(M, qh, kvh):
    N = (qh + 2 * kvh) * 64
    A = _bf((M, K), 100 + M)
    W = _bf((N, K), 200 + N, K ** -0.5)
    bias = _randn((N,), 300 + N, 0.5)
    acc, mag = _prod(A, W)
    return A, W, bias, acc, mag


def _qkv_controls(M, kn, ctx, seed):
    """ragged n_new (some sequences inactive, some partly), non-zero pos0, permuted slots; an inactive sequence's position lies far past the RoPE table"""
    g = torch.Generator().manual_seed(seed)
    n_seq = (M + kn - 1) // kn
    n_slots = n_seq + 2
    n_new = torch.randint(0, kn + 1, (n_seq,), generator=g)
    n_new[0], n_new[n_seq // 2], n_new[-1] = kn, 0, max(kn - 1, 0) if kn > 1 else 1
    pos0 = torch.randint(3, ctx - kn + 1, (n_seq,), generator=g)
    pos0[n_new == 0] = 1_000_000
    slot = torch.randperm(n_slots, generator=g)[:n_seq]
    r = torch.arange(M)
    si, lt = r // kn, r % kn
    active = lt < n_new[si]
    pos = torch.where(active, pos0[si] + lt, torch.zeros_like(lt))
    return n_seq, n_slots, n_new.int(), pos0.int(), slot.int(), active, pos, slot[si]


def _qkv_scatter(vals, fill, qh, kvh, n_slots, ctx, active, pos, rslot):
    """[M][N] values -> the q buffer [M][qh][64], K cache [slot][kvh][ctx][64], V^T cache [slot][kvh][64][ctx]; rows that are not active leave `fill`"""
    M = vals.shape[0]
    v = vals.view(M, qh + 2 * kvh, 64)
    q = torch.full((M, qh, 64), fill, dtype=vals.dtype)
    q[active] = v[active, :qh]
    kc = torch.full((n_slots, kvh, ctx, 64), fill, dtype=vals.dtype)
    vt = torch.full((n_slots, kvh, 64, ctx), fill, dtype=vals.dtype)
    kc[rslot[active], :, pos[active]] = v[active, qh:qh + kvh]
    vt[rslot[active], :, :, pos[active]] = v[active, qh + kvh:]
    return q, kc, vt


def _run_qkv(M, qh, kvh, kn, a_norm, runs, ctx=64):
    """runs: (form, kv_frag, options) launches, each compared with the float64 reference"""
    A, W, bias, acc, mag = _qkv_operands(M, qh, kvh)
    N = W.shape[0]
    n_seq, n_slots, n_new, pos0, slot, active, pos, rslot = _qkv_controls(M, kn, ctx, 7 * M + kn)
    cos, sin = _rope_tables(ctx)
    inv = _inv_rms(A, torch.float64) if a_norm else torch.ones(M, 1, dtype=torch.float64)
    ref, bound = _qkv_bound(acc, mag, inv, bias, cos[pos], sin[pos], qh + kvh, a_norm)
    sc = functools.partial(_qkv_scatter, qh=qh, kvh=kvh, n_slots=n_slots, ctx=ctx, active=active, pos=pos, rslot=rslot)
    refs, bounds, masks = sc(ref, 0.0), sc(bound, 0.0), sc(torch.ones_like(ref), 0.0)
    perm = packing.qkv_row_perm(qh + 2 * kvh)
    Wd, bd = _dev(packing.pack_frag(W[perm])), _dev(bias[perm].contiguous())
    Af, Ar = _dev(packing.frag_rows(A)), _dev(A)
    ctl = dict(kn=kn, q_heads=qh, kv_heads=kvh, slot=_dev(slot), pos0=_dev(pos0), n_new=_dev(n_new), rope_cos=_dev(cos), rope_sin=_dev(sin), max_ctx=ctx)
    for form, kv_frag, opts in runs:
        qb, kc, vt = _sent(M * qh * 64, torch.bfloat16), _sent(n_slots * kvh * ctx * 64, torch.bfloat16), _sent(n_slots * kvh * ctx * 64, torch.bfloat16)
        with _lib.option_scope(**opts):
            ops.decode_gemm(form, SK_QKV_ROPE, M, N, K, Af if form else Ar, Wd, lda=K, bias=bd, qbuf=qb, kcache=kc, vTcache=vt, kv_frag=kv_frag,
                            a_norm=a_norm, norm_eps=EPS, **ctl)
        torch.cuda.synchronize()
        kc, vt = kc.cpu().view(n_slots, kvh, ctx * 64), vt.cpu().view(n_slots, kvh, ctx * 64)
        got = (qb.cpu(), packing.unkfrag(kc, ctx) if kv_frag else kc, packing.unvfrag(vt, ctx) if kv_frag else vt)
        for name, g_, r_, b_, m_ in zip(('q', 'k cache', 'v^T cache'), got, refs, bounds, masks):
            _check('qkv M=%d kn=%d norm=%d form=%d frag=%d %s %s' % (M, kn, a_norm, form, kv_frag, opts, name), g_, r_, b_, m_ > 0)


@gpu
@pytest.mark.parametrize('a_norm', [0, 1])
@pytest.mark.parametrize('kn', [1, 2, 4])
@pytest.mark.parametrize('M', ROWS)
def test_qkv_rope_lands_every_active_element_and_nothing_else(M, kn, a_norm):
    """(q, kv) heads = (3, 1): N = 320, 20 column tiles — at dec_gpw_qkv 1 (20 column groups: workgroups with xcd >= 4 of the third round return at once) and
    3 (7 groups, the last with 2 of 3 tiles: dummy-slot DMAs).  q / k / v^T of every active row at its address in row-major and fragment-order caches, the
    sentinel everywhere else.  Bound: the module docstring, SK_QKV_ROPE."""
    _run_qkv(M, 3, 1, kn, a_norm, [(1, f, dict(dec_gpw_qkv=g)) for f in (0, 1) for g in (1, 3)] + [(0, f, {}) for f in (0, 1)])


@gpu
def test_qkv_rope_at_the_production_head_counts():
    """(14, 2) heads: N = 1152, 72 tiles, at 129 rows (three chunks, the last of one row)"""
    _run_qkv(129, 14, 2, 2, 1, [(1, 1, {}), (1, 0, dict(dec_gpw_qkv=3)), (0, 1, {})])


# ================================================================================================================================================
# SK_RESID
# ================================================================================================================================================
@functools.lru_cache(maxsize=2)
def _resid_case(M, N):
    A, W, bias, x0 = _bf((M, K), 400 + M), _bf((N, K), 500 + N, K ** -0.5), _randn((N,), 600 + N, 0.5), _randn((M, N), 700 + M + N, 2.0)
    acc, mag = _prod(A, W)
    ref = x0.double() + (acc + bias.double())
    return A, W, bias, x0, ref, _f32_bound(K, mag, ref)


@gpu
@pytest.mark.parametrize('N', [96, 896])
@pytest.mark.parametrize('M', ROWS)
def test_resid_updates_the_stream_in_place_and_copies_it(M, N):
    """x += A W^T + bias on the fp32 stream in place (6 and 56 column tiles; dec_gpw_res 1 and 4: 96 columns then are two groups of 4 and 2 tiles), with no
    16-bit copy, a row-major one, a fragment-order one (out_frag: form 1 only).  The strides' padding and the fragment matrix's padding rows keep the sentinel."""
    A, W, bias, x0, ref, e = _resid_case(M, N)
    ldo, ldo2, R16 = N + 4, N + 8, (M + 15) // 16 * 16
    Wd, bd, Af, Ar = _dev(packing.pack_frag(W)), _dev(bias), _dev(packing.frag_rows(A)), _dev(A)
    pad = lambda t, ld: torch.cat([t, torch.zeros(M, ld - N, dtype=t.dtype)], 1)
    mx, mc = pad(torch.ones(M, N), ldo) > 0, pad(torch.ones(M, N), ldo2) > 0
    mfr = torch.zeros(R16, N)
    mfr[:M] = 1
    for form, mode, opts in [(1, m, dict(dec_gpw_res=g)) for m in ('none', 'rows', 'frag') for g in (1, 4)] + [(0, m, {}) for m in ('none', 'rows')]:
        x = _sent(M * ldo, torch.float32).view(M, ldo)
        x[:, :N] = _dev(x0)
        c = None if mode == 'none' else _sent(R16 * N if mode == 'frag' else M * ldo2, torch.bfloat16)
        with _lib.option_scope(**opts):
            ops.decode_gemm(form, SK_RESID, M, N, K, Af if form else Ar, Wd, lda=K, bias=bd, out=x, ldo=ldo, out2=c, ldo2=ldo2, out_frag=mode == 'frag')
        torch.cuda.synchronize()
        tag = 'resid M=%d N=%d form=%d copy=%s %s ' % (M, N, form, mode, opts)
        _check(tag + 'stream', x, pad(ref, ldo), pad(e, ldo), mx)
        if mode == 'rows':
            _check(tag + 'copy', c, pad(ref, ldo2), pad(_bf_bound(ref, e), ldo2), mc)
        elif mode == 'frag':
            z = torch.zeros(R16 - M, N, dtype=torch.float64)
            _check(tag + 'copy', packing.unfrag_rows(c.cpu(), R16, N), torch.cat([ref, z]), torch.cat([_bf_bound(ref, e), z]), mfr > 0)


# ================================================================================================================================================
# SK_RESID in the narrow weight layout (gemm_narrow_resid_kernel: the o_proj / down_proj of every decode grid of 32 rows or fewer)
# ================================================================================================================================================
@functools.lru_cache(maxsize=2)
def _narrow_case(M, Kn, dtype):
    N = 100
    A, W = _randn((M, Kn), 1900 + M + Kn).to(dtype), _randn((N, Kn), 2000 + Kn, Kn ** -0.5).to(dtype)
    bias, x0 = _randn((N,), 2100 + Kn, 0.5), _randn((M, N), 2200 + M + Kn, 2.0)
    acc, mag = _prod(A, W)
    return A, W, bias, x0, acc, mag


@gpu
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'fp32'])
@pytest.mark.parametrize('Kn', [896, 4864, 5248])
@pytest.mark.parametrize('M', [1, 7, 16, 17, 32])
def test_narrow_resid_updates_the_stream_in_place_and_copies_it(M, Kn, dtype):
    """x += A W^T + bias with W = packing.pack_narrow4 ([N/4][K/128][64][8]: a workgroup owns 4 output columns over the whole K, 8 waves share the 128-wide K blocks):
    K = 896 (7 blocks: one per wave, wave 7 idle), 4864 (38 blocks: 5 per wave and request — 3 in fp32 —, a short last wave), 5248 (41 blocks: the K > 40 blocks form);
    1 and 2 row tiles (blockIdx.z) with a clamped last row; N = 100 (25 workgroups) in strides of 104 / 108, the sentinel beyond N and beyond M; with and without
    bias, with and without the copy in the operand type.  Bounds: the module docstring, fp32 outputs and the 16-bit copy of SK_RESID."""
    A, W, bias, x0, acc, mag = _narrow_case(M, Kn, dtype)
    N = W.shape[0]
    ldo, ldo2 = N + 4, N + 8
    Wd, Ad = _dev(packing.pack_narrow4(W)), _dev(A)
    pad = lambda t, ld: torch.cat([torch.cat([t, torch.zeros(M, ld - N, dtype=t.dtype)], 1), torch.zeros(2, ld, dtype=t.dtype)])
    for with_bias in (True, False):
        ref = x0.double() + (acc + bias.double() if with_bias else acc)
        e = _f32_bound(Kn, mag, ref)
        for with_copy in (True, False):
            x = _sent((M + 2) * ldo, torch.float32).view(M + 2, ldo)
            x[:M, :N] = _dev(x0)
            c = _sent((M + 2) * ldo2, dtype) if with_copy else None
            ops.decode_gemm(0, SK_RESID, M, N, Kn, Ad, Wd, lda=Kn, bias=_dev(bias) if with_bias else None, out=x, ldo=ldo, out2=c, ldo2=ldo2, w_narrow=True)
            torch.cuda.synchronize()
            tag = 'narrow resid M=%d K=%d %s bias=%d copy=%d ' % (M, Kn, str(dtype)[6:], with_bias, with_copy)
            _check(tag + 'stream', x, pad(ref, ldo), pad(e, ldo), pad(torch.ones(M, N), ldo) > 0)
            if with_copy:
                _check(tag + 'copy', c, pad(ref, ldo2), pad(_bf_bound(ref, e) if dtype == torch.bfloat16 else e, ldo2), pad(torch.ones(M, N), ldo2) > 0)


# ================================================================================================================================================
# SK_STORE: the stacked output projection
# ================================================================================================================================================
def _run_store(nz, S, N, n_valid, runs):
    A, W, bias = _bf((nz * S, K), 800 + nz * S), _bf((N, K), 900 + N, K ** -0.5), _randn((N,), 1000 + N, 0.5)
    acc, mag = _prod(A, W)
    val = acc + bias.double()
    keep = torch.arange(N) < n_valid
    to_out = lambda t: t.view(nz, S, N).permute(1, 0, 2).contiguous()          # rows z * S + s come back at out[s][z][:]
    ref, e, mask = to_out(val), to_out(_f32_bound(K, mag, val)), to_out(torch.ones(nz * S, N) * keep) > 0
    Wd, bd, Af, Ar = _dev(packing.pack_frag(W)), _dev(bias), _dev(packing.frag_rows(A)), _dev(A)
    for form, opts in runs:
        out = _sent(S * nz * N, torch.float32)
        with _lib.option_scope(**opts):
            ops.decode_gemm(form, SK_STORE, S, N, K, Af if form else Ar, Wd, lda=K, bias=bd, out=out, ldo=nz * N, nz=nz, a_zs=S * K, out_zs=N, n_valid=n_valid)
        torch.cuda.synchronize()
        _check('store nz=%d S=%d N=%d form=%d %s' % (nz, S, N, form, opts), out, ref, e, mask)


@gpu
@pytest.mark.parametrize('nz,S', [(1, 100), (2, 50), (4, 40), (4, 64)])
def test_store_routes_the_stacked_heads_rows(nz, S):
    """The shared output projection over nz heads' rows as ONE stacked fragment-order matrix (a head's block crosses a 64-row chunk: rows 50..99, 40..79, 120..159),
    back at out[s][z][:]; N = 112 (7 tiles) with 100 valid columns, dec_gpw_out 3 (groups of 3, 3, 1) and 2; columns >= n_valid keep the sentinel."""
    _run_store(nz, S, 112, 100, [(1, dict(dec_gpw_out=3)), (1, dict(dec_gpw_out=2)), (0, {})])


@gpu
def test_store_at_the_vocabulary_width():
    """N = 6768 (423 tiles) with 6761 valid columns, 4 heads x 64 rows = the 256-row maximum"""
    _run_store(4, 64, 6768, 6761, [(1, {}), (0, {})])


# ================================================================================================================================================
# SK_SWIGLU
# ================================================================================================================================================
def _swiglu_values(acc_g, acc_u, inv, dt):
    g, u = acc_g.to(dt) * inv.to(dt), acc_u.to(dt) * inv.to(dt)
    return g * torch.sigmoid(g) * u


def _swiglu_bound(acc_g, mag_g, acc_u, mag_u, inv, a_norm):
    g, u = acc_g * inv, acc_u * inv
    rel = (_d_r(K) + U) if a_norm else 0.0
    e_g, e_u = inv * K * U * mag_g + rel * g.abs(), inv * K * U * mag_u + rel * u.abs()
    sg = torch.sigmoid(g)
    ref = g * sg * u
    e = (u * (sg + g * sg * (1 - sg))).abs() * e_g + (g * sg).abs() * e_u + (2 * U + 4 * 2.0 ** -23) * ref.abs()
    return ref, _bf_bound(ref, e)


def _swiglu_operands(rows, I, seed, heads=1):
    A = _bf((heads, rows, K), seed)
    Wg, Wu = _randn((heads, I, K), seed + 1, K ** -0.5), _randn((heads, I, K), seed + 2, K ** -0.5)
    return A, Wg, Wu


@functools.lru_cache(maxsize=2)
def _swiglu_case(M, I, a_norm):
    A, Wg, Wu = _swiglu_operands(M, I, 1100 + M + I)
    A, Wg, Wu = A[0], Wg[0].to(torch.bfloat16), Wu[0].to(torch.bfloat16)
    inv = _inv_rms(A, torch.float64) if a_norm else torch.ones(M, 1, dtype=torch.float64)
    (ag, mg), (au, mu) = _prod(A, Wg), _prod(A, Wu)
    return (A, Wg, Wu) + _swiglu_bound(ag, mg, au, mu, inv, a_norm)


@gpu
@pytest.mark.parametrize('a_norm', [0, 1])
@pytest.mark.parametrize('I', [96, 128])
@pytest.mark.parametrize('M', ROWS)
def test_swiglu_rows(M, I, a_norm):
    """silu(gate) * up over (gate, up) tile pairs (packing.pack_gate_up): I = 96 (6 pairs, row-major rows out) and 128 (8 pairs, fragment-order rows out in
    form 1), dec_gpw_mlp 3 and 4, with and without the fused RMSNorm.  Bound: the module docstring, SK_SWIGLU; the fast-math allowance is the 4 * 2^-23 |ref| of
    the issue, not widened."""
    A, Wg, Wu, ref, bound = _swiglu_case(M, I, a_norm)
    frag, R16, ldo = I == 128, (M + 15) // 16 * 16, I + (0 if I == 128 else 8)
    Wd, Af, Ar = _dev(packing.pack_gate_up(Wg, Wu)), _dev(packing.frag_rows(A)), _dev(A)
    z = torch.zeros(R16 - M, I, dtype=torch.float64)
    mfr = torch.cat([torch.ones(M, I), z.float()]) > 0
    padc = lambda t: torch.cat([t, torch.zeros(M, ldo - I, dtype=t.dtype)], 1)
    for form, opts in [(1, dict(dec_gpw_mlp=3)), (1, dict(dec_gpw_mlp=4)), (0, {})]:
        fo = bool(frag and form)
        out = _sent(R16 * I if fo else M * ldo, torch.bfloat16)
        with _lib.option_scope(**opts):
            ops.decode_gemm(form, SK_SWIGLU, M, 2 * I, K, Af if form else Ar, Wd, lda=K, out=out, ldo=ldo, a_norm=a_norm, norm_eps=EPS, out_frag=fo)
        torch.cuda.synchronize()
        tag = 'swiglu M=%d I=%d norm=%d form=%d %s' % (M, I, a_norm, form, opts)
        if fo:
            _check(tag, packing.unfrag_rows(out.cpu(), R16, I), torch.cat([ref, z]), torch.cat([bound, z]), mfr)
        else:
            _check(tag, out, padc(ref), padc(bound), padc(torch.ones(M, I)) > 0)


def _heads_case(nz, S, I, seed, quantise):
    """nz heads, S rows each padded to S16 in A, every head its own weights; quantise: the weights are the dequantised e4m3 x power-of-two matrices"""
    A, Wg, Wu = _swiglu_operands(S, I, seed, nz)
    W = torch.stack([packing.interleave_gate_up(Wg[z], Wu[z]) for z in range(nz)])            # [nz][2 I][K], alternating 16-row tiles
    codes = scales = None
    if quantise:
        q = [packing.quantize_e4m3_pow2(W[z]) for z in range(nz)]
        codes, scales, W = torch.stack([packing.pack_frag_fp8(c) for c, _, _ in q]), torch.stack([s for _, s, _ in q]), torch.stack([d for _, _, d in q])
    W = W.to(torch.bfloat16)
    assert not quantise or all(torch.equal(W[z].float(), q[z][2]) for z in range(nz))         # the dequantised weights are bf16 values exactly
    Wt = W.view(nz, I // 16, 2, 16, K)
    refs, bounds = [], []
    for z in range(nz):
        (ag, mg), (au, mu) = _prod(A[z], Wt[z, :, 0].reshape(I, K)), _prod(A[z], Wt[z, :, 1].reshape(I, K))
        r, b = _swiglu_bound(ag, mg, au, mu, torch.ones(S, 1, dtype=torch.float64), 0)
        refs.append(r)
        bounds.append(b)
    return A, W, codes, scales, torch.stack(refs), torch.stack(bounds)


def _run_heads(nz, S, I, A, Wd, form, opts, w_scale=None):
    S16 = (S + 15) // 16 * 16
    if form:
        Ad = _dev(torch.cat([packing.frag_rows(A[z]) for z in range(nz)]))
    else:
        Ad = _dev(torch.cat([A, torch.zeros(nz, S16 - S, K, dtype=A.dtype)], 1).contiguous())    # row-major, the same padded blocks
    out = _sent(nz * S * I, torch.bfloat16)
    with _lib.option_scope(**opts):
        ops.decode_gemm(form, SK_SWIGLU, S, 2 * I, K, Ad, Wd, lda=K, out=out, ldo=I, nz=nz, a_zs=S16 * K, w_zs=2 * I * K, out_zs=S * I,
                        w_scale=w_scale, w_scale_zs=2 * I)
    torch.cuda.synchronize()
    return out


@gpu
@pytest.mark.parametrize('nz', [2, 4])
def test_swiglu_stacked_heads(nz):
    """The MTP heads' MLP: nz heads over blockIdx.y, 40 rows per head padded to 48 in A, per-head a_zs / w_zs / out_zs; I = 368 (23 pairs: at dec_gpw_hmlp 11 three
    groups of 11, 11, 1; at 2 twelve groups, the last of one pair)"""
    S, I = 40, 368
    A, W, _, _, ref, bound = _heads_case(nz, S, I, 1300 + nz, False)
    Wd = _dev(torch.stack([packing.pack_frag(W[z]) for z in range(nz)]))
    for form, opts in [(1, dict(dec_gpw_hmlp=11)), (1, dict(dec_gpw_hmlp=2)), (0, {})]:
        _check('heads mlp nz=%d form=%d %s' % (nz, form, opts), _run_heads(nz, S, I, A, Wd, form, opts), ref, bound)


@gpu
@pytest.mark.parametrize('nz,S', [(1, 100), (2, 40)])
def test_swiglu_e4m3_weights_are_the_bf16_stream_bit_for_bit(nz, S):
    """csrc/gemm_dec.hip, W8: e4m3 codes x per-column power-of-two scales (packing.quantize_e4m3_pow2 + pack_frag_fp8) compute the products of the bf16 stream of
    the dequantised weights in the same order — torch.equal, at dec_gpw_hmlp 11 and 2; the bf16 form itself is held to float64."""
    I = 368
    A, W, codes, scales, ref, bound = _heads_case(nz, S, I, 1400 + nz, True)
    Wd, Cd, Sd = _dev(torch.stack([packing.pack_frag(W[z]) for z in range(nz)])), _dev(codes), _dev(scales)
    assert Cd.dtype == torch.uint8
    for g in (11, 2):
        y16 = _run_heads(nz, S, I, A, Wd, 1, dict(dec_gpw_hmlp=g))
        y8 = _run_heads(nz, S, I, A, Cd, 1, dict(dec_gpw_hmlp=g), w_scale=Sd)
        _check('heads mlp bf16 weights nz=%d gpw=%d' % (nz, g), y16, ref, bound)
        assert torch.equal(y8, y16), 'e4m3 form differs from the bf16 form in %d elements' % int((y8 != y16).sum())


# ================================================================================================================================================
# SK_PARTIAL and the reduce that follows it
# ================================================================================================================================================
KS = 608                         # 19 k-steps per slice


@functools.lru_cache(maxsize=2)
def _partial_case(M, N, split):
    A, W = _bf((M, split * KS), 1500 + M + split), _bf((N, split * KS), 1600 + N + split, (split * KS) ** -0.5)
    sl = [_prod(A[:, s * KS:(s + 1) * KS], W[:, s * KS:(s + 1) * KS]) for s in range(split)]
    ref, mag = torch.stack([r for r, _ in sl]), torch.stack([m for _, m in sl])
    return A, W, ref, _f32_bound(KS, mag, ref)


def _run_partial(M, N, split, form, opts, A, W):
    part = _sent(split * M * N, torch.float32)
    with _lib.option_scope(**opts):
        ops.decode_gemm(form, SK_PARTIAL, M, N, split * KS, _dev(packing.frag_rows(A)) if form else _dev(A), _dev(packing.pack_frag(W)), lda=split * KS,
                        split_k=split, part=part)
    torch.cuda.synchronize()
    return part.view(split, M, N)


@gpu
@pytest.mark.parametrize('N', [96, 896])
@pytest.mark.parametrize('split', [8, 2, 3])
@pytest.mark.parametrize('M', ROWS)
def test_partials_slice_by_slice(M, split, N):
    """Split-K partials, K = split x 608: 8 slices take the slice = XCD grid, 2 and 3 the generic one; N = 96 / 896 are 3 / 28 tile pairs, at dec_gpw_down 2 (groups
    of 2, 1 pairs at N = 96) and 3 (28 pairs: 9 groups of 3 and one of 1).  Form 1: every slice against the float64 product over ITS K range, then the float64 sum of
    the slices against the whole product.  Form 0 cuts K elsewhere: its sum only, with the same bound (the fp32 sums of any partition of the K products)."""
    A, W, ref, e = _partial_case(M, N, split)
    for form, opts in [(1, dict(dec_gpw_down=2)), (1, dict(dec_gpw_down=3)), (0, {})]:
        part = _run_partial(M, N, split, form, opts, A, W).double().cpu()
        tag = 'partial M=%d N=%d split=%d form=%d %s ' % (M, N, split, form, opts)
        if form:
            _check(tag + 'slices', part, ref, e)
        _check(tag + 'sum', part.sum(0), ref.sum(0), e.sum(0))


def _reduce_ref(x0, part, bias, gain, do_norm, rows_per_z):
    """float64 reference and bound of reduce_rmsnorm from the very fp32 values it is given.  x0 [M][H], part [nzb][S][rows_per_z][H], bias / gain [nzb][H] or None"""
    M, H = x0.shape
    nzb, S = part.shape[0], part.shape[1]
    p = part.double().permute(1, 0, 2, 3).reshape(S, M, H)
    rep = lambda t: t.double()[:, None, :].expand(nzb, rows_per_z, H).reshape(M, H)
    b = rep(bias) if bias is not None else torch.zeros(M, H, dtype=torch.float64)
    x1 = x0.double() + p.sum(0) + b
    e_x = (S + 2) * U * (x0.double().abs() + p.abs().sum(0) + b.abs())
    if not do_norm:
        return x1, e_x, x1, _bf_bound(x1, e_x)
    inv = torch.rsqrt((x1 * x1).mean(1, keepdim=True) + EPS)
    gn = rep(gain) if gain is not None else torch.ones(M, H, dtype=torch.float64)
    y = x1 * inv * gn
    rel = (1 + UB) ** 2 - 1 + 1.02 * (_d_r(H) + 2 * U + e_x.norm(dim=1, keepdim=True) / x1.norm(dim=1, keepdim=True))
    return x1, e_x, y, y.abs() * rel + 1.02 * gn.abs() * inv * e_x


def _run_reduce(tag, x0, part, bias, gain, do_norm, rows_per_z, ldx, mode):
    """mode: 'rows' (y row-major, ldy = H + 8), 'frag' (one fragment-order matrix), 'zfrag' (every z block its own fragment-order matrix of rows_per_z padded to 16)"""
    M, H = x0.shape
    nzb, S = part.shape[0], part.shape[1]
    x1, e_x, y, e_y = _reduce_ref(x0, part, bias, gain, do_norm, rows_per_z)
    x = _sent(M * ldx, torch.float32).view(M, ldx)
    x[:, :H] = _dev(x0)
    zrows = (rows_per_z + 15) // 16 * 16 if mode == 'zfrag' else 0
    R16 = nzb * zrows if mode == 'zfrag' else (M + 15) // 16 * 16
    ldy = H + 8
    yb = _sent(M * ldy if mode == 'rows' else R16 * H, torch.bfloat16)
    ops.reduce_rmsnorm(x, M=M, H=H, ldx=ldx, part=_dev(part), split_k=S, part_stride=rows_per_z * H, part_zs=S * rows_per_z * H, bias=_dev(bias), bias_zs=H,
                       gain=_dev(gain), gain_zs=H, eps=EPS, do_norm=do_norm, y=yb, ldy=ldy, rows_per_z=rows_per_z, y_frag=mode != 'rows', y_frag_zrows=zrows)
    torch.cuda.synchronize()
    pad = lambda t, ld: torch.cat([t, torch.zeros(M, ld - H, dtype=t.dtype)], 1)
    ones = torch.ones(M, H)
    _check(tag + ' x', x, pad(x1, ldx), pad(e_x, ldx), pad(ones, ldx) > 0)
    if mode == 'rows':
        _check(tag + ' y', yb, pad(y, ldy), pad(e_y, ldy), pad(ones, ldy) > 0)
        return
    if mode == 'zfrag':          # row z * zrows + (m % rows_per_z) of the stacked fragment-order matrices
        put = lambda t: torch.cat([t.view(nzb, rows_per_z, H), torch.zeros(nzb, zrows - rows_per_z, H, dtype=t.dtype)], 1).reshape(R16, H)
    else:
        put = lambda t: torch.cat([t, torch.zeros(R16 - M, H, dtype=t.dtype)])
    _check(tag + ' y', packing.unfrag_rows(yb.cpu(), R16, H), put(y), put(e_y), put(ones) > 0)


@gpu
@pytest.mark.parametrize('mode', ['rows', 'frag', 'zfrag'])
@pytest.mark.parametrize('do_norm', [0, 1])
def test_reduce_rmsnorm_after_the_partials(do_norm, mode):
    """The decode step's chain: form-1 partials (100 rows, 8 slices, N = H = 896) -> x += sum of slices + bias in place -> (RMSNorm x gain) -> 16-bit y, row-major,
    in fragment order, or (rows_per_z = 50, y_frag_zrows = 64) as a 2-head block with per-head partials, bias and gain.  Bound: the module docstring."""
    M, H, split = 100, 896, 8
    A, W, _, _ = _partial_case(M, H, split)
    part = _run_partial(M, H, split, 1, {}, A, W).cpu()
    nzb = 2 if mode == 'zfrag' else 1
    rz = M // nzb
    part = part.view(split, nzb, rz, H).permute(1, 0, 2, 3).contiguous()                      # [z][s][rows_per_z][H]
    x0, bias, gain = _randn((M, H), 1700, 2.0), _randn((nzb, H), 1701, 0.5), 1.0 + _randn((nzb, H), 1702, 0.3)
    _run_reduce('reduce H=896 norm=%d %s' % (do_norm, mode), x0, part, bias, gain if do_norm else None, do_norm, rz, H + 4, mode)


@gpu
@pytest.mark.parametrize('ldx', [100, 102])
@pytest.mark.parametrize('do_norm', [0, 1])
def test_reduce_rmsnorm_at_a_width_of_100(do_norm, ldx):
    """H = 100 (no multiple of 32: row-major y only) on fp32 partials of three slices: with ldx = 100 the 16-byte path (H, ldx, the slice stride all multiples of 4),
    with ldx = 102 the scalar one."""
    M, H, S = 37, 100, 3
    x0, part, bias, gain = _randn((M, H), 1800, 2.0), _randn((1, S, M, H), 1801), _randn((1, H), 1802, 0.5), 1.0 + _randn((1, H), 1803, 0.3)
    _run_reduce('reduce H=100 norm=%d ldx=%d' % (do_norm, ldx), x0, part, bias, gain, do_norm, M, ldx, 'rows')


# ================================================================================================================================================
# the entry point refuses instead of falling through
# ================================================================================================================================================
@gpu
def test_form_1_refuses_a_shape_it_does_not_instantiate():
    A, W = _bf((100, 64), 1), _bf((32, 64), 2)
    out = _sent(100 * 32, torch.float32)
    with pytest.raises(_lib.HvxError, match='form 1 does not take this launch'):
        ops.decode_gemm(1, SK_STORE, 100, 32, 64, _dev(packing.frag_rows(A)), _dev(packing.pack_frag(W)), lda=64, out=out, ldo=32)
    with _lib.option_scope(dec_gemm=0):                                   # the model's A / B switch turns the form off: still an error here, never the other kernel
        A, W = _bf((100, K), 1), _bf((32, K), 2)
        with pytest.raises(_lib.HvxError, match='form 1 does not take this launch'):
            ops.decode_gemm(1, SK_STORE, 100, 32, K, _dev(packing.frag_rows(A)), _dev(packing.pack_frag(W)), lda=K, out=out, ldo=32)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


# ================================================================================================================================================
# the bounds hold for an fp32 emulation of the kernels' arithmetic (no device)
# ================================================================================================================================================
def _emu_check(what, got, ref, bound):
    err = (got.double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print('%s (fp32 emulation): worst error / bound %.3f' % (what, worst))
    assert bool((err <= bound).all()), (what, worst)


@pytest.mark.parametrize('M', [33, 100])
def test_fp32_emulation_stays_inside_the_bounds(M):
    f32, bf = torch.float32, torch.bfloat16
    # QKV + RoPE, with and without the fused norm
    A, W, bias, acc, mag = _qkv_operands(M, 3, 1)
    cos, sin = _rope_tables(64)
    pos = torch.randint(0, 64, (M,), generator=torch.Generator().manual_seed(5))
    a32 = _acc32(A, W)
    for a_norm in (0, 1):
        inv = _inv_rms(A, torch.float64) if a_norm else torch.ones(M, 1, dtype=torch.float64)
        ref, bound = _qkv_bound(acc, mag, inv, bias, cos[pos], sin[pos], 4, a_norm)
        emu = _qkv_values(a32, _inv_rms(A, f32) if a_norm else torch.ones(M, 1), bias, cos[pos], sin[pos], 4, f32).to(bf)
        _emu_check('qkv norm=%d' % a_norm, emu, ref, bound)
    # residual stream and its copy
    A, W, bias, x0, ref, e = _resid_case(M, 96)
    x1 = x0 + (_acc32(A, W) + bias)
    _emu_check('resid stream', x1, ref, e)
    _emu_check('resid copy', x1.to(bf), ref, _bf_bound(ref, e))
    # SwiGLU
    for a_norm in (0, 1):
        A, Wg, Wu, ref, bound = _swiglu_case(M, 96, a_norm)
        emu = _swiglu_values(_acc32(A, Wg), _acc32(A, Wu), _inv_rms(A, f32) if a_norm else torch.ones(M, 1), f32).to(bf)
        _emu_check('swiglu norm=%d' % a_norm, emu, ref, bound)
    # partials and the reduce
    A, W, ref, e = _partial_case(M, 96, 3)
    part = torch.stack([_acc32(A[:, s * KS:(s + 1) * KS], W[:, s * KS:(s + 1) * KS]) for s in range(3)])
    _emu_check('partials', part, ref, e)
    x0, bias, gain = _randn((M, 96), 11, 2.0), _randn((1, 96), 12, 0.5), 1.0 + _randn((1, 96), 13, 0.3)
    for do_norm in (0, 1):
        x1r, e_x, y, e_y = _reduce_ref(x0, part[None], bias, gain, do_norm, M)
        x1 = x0 + ((part[0] + part[1]) + part[2]) + bias
        _emu_check('reduce x', x1, x1r, e_x)
        if do_norm:
            inv = torch.rsqrt((x1 * x1).mean(1, keepdim=True) + EPS)
            _emu_check('reduce y norm', (gain * (x1 * inv).to(bf).float()).to(bf), y, e_y)
        else:
            _emu_check('reduce y cast', x1.to(bf), y, e_y)
