"""Operator-level parity of the vocoder's PLANE-PAIR convolution kernels (gemm_x3.hip: gemm_x3p_kernel<128,64>, gemm_x3p_kernel<128,128>, gemm_x3p8_kernel,
conv64_x3p_kernel<192>; gemm_epilogue.h: store_planes4 / store_planes1, res2, div; elementwise.hip: act_rows_planes_kernel) against a float64 convolution.

These are the kernels the default HiFT decode (hvx_hift_config.exact_fp32 == 0) launches behind conv_pre: operands and activated results are fp32 values stored as
(hi, lo) bf16 plane pairs (packing.split_planes; csrc/hvx_kernels.h: GemmArgs.a_planes ...).  Every case here builds its operands from fp32 values with
packing.split_planes, lays them out as hvx_hift.hip does (the lo plane `rows * ld` elements behind hi) and compares with torch.nn.functional.conv1d in float64 on the
CPU on the ORIGINAL fp32 values (left pad (k - 1) * dil, Snake = v + sin(alpha v)^2 / (alpha + 1e-9), LeakyReLU, residuals, all float64).

Bound: max |d| < 2e-5 of the output's max |ref| — the bound the project already asserts for the split form (test_gpu_ops.py: test_conv_split_bf16_form_matches_fp64).
The three-product arithmetic alone (hi.hi + hi.lo + lo.hi in float64, no accumulation error) sits at 4.3e-6 .. 5.0e-6 of the output scale at these shapes and fp32
accumulation adds ~3e-7, so correct arithmetic has a 4x margin; a dropped cross term costs ~2e-3.  A result that leaves as a plane pair is read back as
float(hi) + float(lo), i.e. it carries the pair's own representation error (<= 2^-17 |v| = 7.6e-6 |v|) on top.

Which kernel a case reaches is decided by launch_gemm_x3 (gemm_x3.hip), in this order, for plane-pair operands:
  (R)  conv64_resident && N <= 64 && cin_pad == 64 && stride == up == groups == batch == 1 && M >= 4096 && 128 + (k - 1) * dil <= 192   -> conv64_x3p_kernel<192>
  (S)  N <= 64                                                                                                                        -> gemm_x3p_kernel<128,64,32,64>
  (E)  x3p8 && K % 64 == 0 && cin_pad % 64 == 0                                                                                       -> gemm_x3p8_kernel (8 waves)
  (F)  otherwise                                                                                                                      -> gemm_x3p_kernel<128,128,64,64>
and for fp32 operands with x3: N <= 64 needs M > 4096, otherwise >= 256 tiles of 128 x 128                                               -> gemm_x3_kernel.
Every test's docstring names the condition that sends it there; profiles/kernel_stats_test_gpu_planes.csv is the kernel trace of this file.

Every output of every launch lies between 256 guard rows (both planes of a pair) filled with a sentinel bit pattern, which must come back untouched, and the pad
columns [N, out_cols) of the rows a launch owns must come back zero in both planes.

Measured on an MI355X (max |d| / max |ref|; worst case and worst epilogue of each group — every case prints its own figures).  fp32 results sit at 2.2e-6 .. 3.7e-6
on every form; the larger figures below are pair results, which add the pair's representation error:
    form                                   cases                                                   fp32 results   pair results (worst)
    gemm_x3p8_kernel (E)                   256 -> 256, k {3,7,11} x dil {1,3,5}, 45 061 rows        <= 3.7e-6      8.26e-6 (k 7, dil 1, Snake)
    gemm_x3p8_kernel (E)                   128 -> 128, the same, 40 003 rows; batch 2               <= 3.7e-6      7.61e-6 (k 11, dil 5)
    gemm_x3p_kernel<128,128> (F)           the same 22 cases under x3p8 = 0                         bit-identical to (E), every output
    gemm_x3p_kernel<128,128> (F)           80 -> 128 (cin_pad 96), default options                  <= 3.7e-6      6.87e-6
    gemm_x3p_kernel<128,64> (S)            64 -> 64, 64 -> 18, 32 -> 32, 128 -> 64; batch 2         <= 3.7e-6      7.75e-6 (32 -> 32, k 3)
    conv64_x3p_kernel<192> (R)             64 -> 64 / 18 at 4096, 4097, 36 121 rows                 <= 3.7e-6      7.54e-6 (k 7, dil 5, 36 121 rows)
    (S) under conv64_resident = 0          the same 44 cases (and 4095 rows, (k 11, dil 7))         bit-identical to (R), every output
    up-sampling on (E) / (F) / (S)         512 -> 256 up 8, 256 -> 128 up 5, 128 -> 64 up 3         <= 2.9e-6      7.55e-6
    last-stage pair of launches (S)        reflect-pad(1, 0)(x_up) + si, 36 004 rows                2.64e-6 (row 0 alone 1.18e-6)
    scalar pass (ldo = N + 2)              (E), (F), (S), (R)                                       <= 2.95e-6     exact split of the fp32 result
    act_rows_planes_kernel                 Snake / LeakyReLU, [36 121][64] .. [4507][256]           9.4e-8 / 5e-9  exact split of the fp32 result
    gemm_x3_kernel (in-kernel split)       every case above with > 4096 rows (N <= 64) or >= 256 tiles: distance 0 from the plane-pair form
    packing.split_planes                   1 M values, 1e-6 .. 1e6                                  max |x - (hi + lo)| / |x| = 7.614e-6 (2^-17 = 7.629e-6)
Every pair output is bit for bit the split of the fp32 output of the same launch, in the lean, the vector and the scalar pass, so the pair figures above are the fp32
figures plus at most 2^-17 of the value.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BOUND = 2e-5            # of the output scale: see the module docstring
GUARD = 256             # guard rows in front of and behind the rows a launch owns
SENT16, SENT32 = 0x5A5A, 0x5A5A5A5A        # finite as bf16 / fp32 (1.5e16), never produced by a test
SLOPE = 0.1


def _mods():
    from flowmirror_hydravox_amd import _lib, ops, packing
    _lib.require_gpu()
    return _lib, ops, packing


def _pad32(n):
    return (n + 31) // 32 * 32


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _snake(v, al):
    return v + torch.sin(v * al) ** 2 / (al + 1e-9)


class Buf:
    """An output [B][rows][ld] with GUARD sentinel rows on both sides, fp32 or a (hi, lo) bf16 plane pair [2][B][GUARD + rows + GUARD][ld] (the lo plane lies
    B * (rows + 2 GUARD) * ld elements behind hi: a row-count slip in one plane lands in the other's guard).  The launch gets the view of the owned rows."""

    def __init__(self, B, rows, ld, planes, cols=None):
        self.planes, self.rows, self.cols = planes, rows, ld if cols is None else cols
        tot = rows + 2 * GUARD
        if planes:
            self.t = torch.empty(2, B, tot, ld, dtype=torch.bfloat16, device=DEV)
            self.t.view(torch.int16).fill_(SENT16)
            self.view, self.plane = self.t[0][:, GUARD:GUARD + rows, :self.cols], self.t.stride(0)
        else:
            self.t = torch.empty(B, tot, ld, dtype=torch.float32, device=DEV)
            self.t.view(torch.int32).fill_(SENT32)
            self.view, self.plane = self.t[:, GUARD:GUARD + rows, :self.cols], None

    def _ints(self):
        return self.t.view(torch.int16 if self.planes else torch.int32)

    def owned(self):
        """raw bits of the owned rows, all ld columns: [2][B][rows][ld] or [B][rows][ld]"""
        return self._ints()[..., GUARD:GUARD + self.rows, :]

    def value(self, n):
        """float64 [B][rows][n]: float(hi) + float(lo) of a pair"""
        v = self.t[..., GUARD:GUARD + self.rows, :n].double()
        return v[0] + v[1] if self.planes else v

    def check(self, n, what, first_row=0):
        """guards untouched (both planes), columns beyond out_cols untouched, pad columns [n, out_cols) of the owned rows zero (both planes)"""
        i, sent = self._ints(), (SENT16 if self.planes else SENT32)
        assert bool((i[..., :GUARD, :] == sent).all()), what + ': rows in FRONT of the result were written'
        assert bool((i[..., GUARD + self.rows:, :] == sent).all()), what + ': rows BEHIND the result were written'
        own = self.owned()[..., first_row:, :]
        assert bool((own[..., self.cols:] == sent).all()), what + ': columns beyond out_cols were written'
        assert bool((own[..., n:self.cols] == 0).all()), what + ': pad columns [N, out_cols) are not zero in every plane'
        assert bool((own[..., :n] != sent).any(dim=-1).all()), what + ': an owned row was not written'


class Conv:
    """One convolution: fp32 data on the CPU, its float64 reference (F.conv1d on the CPU), plane-pair operands on the device."""

    def __init__(self, cin, cout, k, dil, rows_in, B=1, up=1, seed=100):
        _lib, ops, packing = _mods()
        self.cin, self.cout, self.k, self.dil, self.B, self.up = cin, cout, k, dil, B, up
        self.rows_in, self.M, self.cp, self.op = rows_in, rows_in * up, _pad32(cin), _pad32(cout)
        x = _rand(B, cin, rows_in, seed=seed)
        w = _rand(cout, cin, k, seed=seed + 1) / math.sqrt(cin * k)
        b = _rand(cout, seed=seed + 2)
        xu = x.double() if up == 1 else F.interpolate(x.double(), scale_factor=up, mode='nearest')
        self.lin = F.conv1d(F.pad(xu, ((k - 1) * dil, 0)), w.double(), b.double(), dilation=dil).transpose(1, 2).contiguous().to(DEV)     # [B][M][cout] float64
        xr = torch.zeros(B, rows_in, self.cp)
        xr[:, :, :cin] = x.transpose(1, 2)
        self.x32, self.w32 = xr.to(DEV), packing.conv_weight(w).to(DEV)
        self.xp, self.wp = packing.split_planes(self.x32), packing.split_planes(self.w32)         # [2][B][rows_in][cp], [2][cout][k * cp]
        self.b = b.to(DEV)
        self.a1, self.a2 = (_rand(cout, seed=seed + 3).abs() + 0.1).to(DEV), (_rand(cout, seed=seed + 4).abs() + 0.1).to(DEV)
        # residuals live in [.][.][op] buffers like the product's (ldres = Cp), pad columns zero
        self.res, self.res2 = (torch.zeros(B, self.M, self.op, device=DEV) for _ in range(2))
        self.res[..., :cout], self.res2[..., :cout] = _rand(B, self.M, cout, seed=seed + 5).to(DEV), _rand(B, self.M, cout, seed=seed + 6).to(DEV)
        self.r64, self.r264 = self.res[..., :cout].double(), self.res2[..., :cout].double()

    def launch(self, planes=True, **kw):
        _lib, ops, packing = _mods()
        geo = dict(n_out=self.cout, taps=self.k, cin_pad=self.cp, pad_left=(self.k - 1) * self.dil, dil=self.dil, up=self.up, m_out=kw.pop('m_out', self.M))
        if planes:       # a pair is addressed like the fp32 tensor it stands for; lo lies B * rows_in * lda behind hi
            return ops.conv1d(self.xp, self.wp, self.b, a_plane=self.B * self.rows_in * self.cp, w_plane=self.cout * self.k * self.cp, **geo, **kw)
        return ops.conv1d(self.x32, self.w32, self.b, x3=True, **geo, **kw)

    def buf(self, planes, rows=None, ld=None, cols=None):
        return Buf(self.B, self.M if rows is None else rows, self.op if ld is None else ld, planes, cols)


def _err(buf, n, ref):
    return ((buf.value(n) - ref).abs().max() / ref.abs().max()).item()


def run_epilogues(c, tag, pair_out=True):
    """The epilogues resblock() / decode_impl() launch (hvx_hift.hip), each held to float64 and to the guard / pad-column rules.  Returns {name: raw bits} and {name: error}.
    pair_out False: the same launches with fp32 results where the product writes a pair (part B compares the two)."""
    _lib = _mods()[0]
    n, lin = c.cout, c.lin
    raw, errs = {}, {}

    def done(name, bufs_refs):
        for j, (bf, ref) in enumerate(bufs_refs):
            bf.check(n, '%s %s[%d]' % (tag, name, j))
            errs['%s[%d]' % (name, j)] = _err(bf, n, ref)
            raw['%s[%d]' % (name, j)] = bf.owned().clone()
    pk = lambda bf, key: {key: bf.plane} if pair_out else {}
    # 1. convs1: bias + Snake -> out as a pair
    o = c.buf(pair_out)
    c.launch(act=_lib.ACT_SNAKE, act_alpha=c.a1, out=o.view, **pk(o, 'out_plane'))
    done('snake', [(o, _snake(lin, c.a1.double()))])
    # 2. convs2, d < 2: bias + fp32 res -> fp32 out, out2 = Snake(out) as a pair
    o, o2 = c.buf(False), c.buf(pair_out)
    c.launch(res=c.res, out=o.view, out2=o2.view, act2=_lib.ACT_SNAKE, act2_alpha=c.a2, **pk(o2, 'out2_plane'))
    v = lin + c.r64
    done('res+snake2', [(o, v), (o2, _snake(v, c.a2.double()))])
    # 3. last convs2 of a ResBlock: + res + res2 -> fp32 accumulator (middle ResBlocks); (+ res + res2) / 3 -> fp32 and / or LeakyReLU(v) as a pair (last ResBlock)
    o = c.buf(False)
    c.launch(res=c.res, res2=c.res2, out=o.view)
    done('res+res2', [(o, lin + c.r64 + c.r264)])
    v = (lin + c.r64 + c.r264) / 3.0
    lrelu = torch.where(v >= 0, v, v * SLOPE)
    o, o2 = c.buf(False), c.buf(pair_out)
    c.launch(res=c.res, res2=c.res2, div=3.0, out=o.view, out2=o2.view, act2=_lib.ACT_LRELU, act2_param=SLOPE, **pk(o2, 'out2_plane'))
    done('mean3', [(o, v), (o2, lrelu)])
    o2 = c.buf(pair_out)
    c.launch(res=c.res, res2=c.res2, div=3.0, out2=o2.view, act2=_lib.ACT_LRELU, act2_param=SLOPE, **pk(o2, 'out2_plane'))       # out is null
    done('mean3, out null', [(o2, lrelu)])
    # 4. bias only -> fp32 (conv_post: N = 18 into ldo = out_cols = 32)
    o = c.buf(False)
    c.launch(out=o.view)
    done('bias', [(o, lin)])
    worst = max(errs.values())
    print('%-34s %s  worst %.2e' % (tag, ' '.join('%s %.2e' % kv for kv in errs.items()), worst))
    assert worst < BOUND, (tag, errs)
    return raw, errs


def _same(ra, rb):
    return all(torch.equal(ra[k], rb[k]) for k in ra)


def _dist(ra, rb, key='bias[0]'):
    """mutual distance of two fp32 results (raw bits), in units of the result's scale"""
    a, b = ra[key].view(torch.float32).double(), rb[key].view(torch.float32).double()
    return ((a - b).abs().max() / a.abs().max()).item()


def _in_kernel_split(c, tag, raw_pairs):
    """gemm_x3_kernel (fp32 operands split on their way into LDS) on the same fp32 values: within the float64 bound itself; its distance from the plane-pair form is printed"""
    o = c.buf(False)
    c.launch(planes=False, out=o.view)
    o.check(c.cout, tag + ' in-kernel split')
    e = _err(o, c.cout, c.lin)
    print('%-34s in-kernel split (gemm_x3_kernel) %.2e of the scale; distance from the plane-pair form %.2e' % (tag, e, _dist({'bias[0]': o.owned()}, raw_pairs)))
    assert e < BOUND, (tag, e)


# ---- A / D: the 128 x 128 tile forms ------------------------------------------------------------------------------------------------------------------------------

WIDE = [(256, 256, k, d, 45061, 1) for k in (3, 7, 11) for d in (1, 3, 5)] + [(128, 128, k, d, 40003, 1) for k in (3, 7, 11) for d in (1, 3, 5)] + [
    (256, 256, 3, 1, 45056, 1),        # a whole number of 128-row tiles
    (256, 200, 3, 1, 9001, 1),         # a partial column tile (cols 128 .. 199 of the second tile; out_cols = 224)
    (128, 128, 7, 3, 5003, 2), (256, 256, 3, 5, 3001, 2)]      # batch 2: a_bs / out_bs strides


@pytest.mark.parametrize('cin,cout,k,dil,rows,B', WIDE)
def test_wide_convs_8_wave_and_4_wave_tiles(cin, cout, k, dil, rows, B):
    """N > 64 skips (R) and (S).  x3p8 = 1 (default): K and cin_pad are multiples of 64 -> (E) gemm_x3p8_kernel; x3p8 = 0 -> (F) gemm_x3p_kernel<128,128>.
    The 256- / 128-channel ResBlock shapes of the first two stages at 8 T - 3 / 40 T + 3 rows (ragged last row tile), every epilogue, both forms against float64.
    gemm_x3.hip says of the 8-wave form "same (hi, lo) pairs, same k order, same three MFMAs per step: results are bit-identical to the 4-wave form": measured
    here bit-identical on every case and epilogue, so equality is asserted.  The fp32-operand launch of the same shape has >= 256 tiles at the long row counts
    and takes gemm_x3_kernel<128,128>."""
    _lib = _mods()[0]
    c = Conv(cin, cout, k, dil, rows, B=B)
    tag = '%d>%d k%d d%d M%d B%d' % (cin, cout, k, dil, rows, B)
    with _lib.option_scope(x3p8=1):
        r8, _ = run_epilogues(c, tag + ' 8-wave')
    with _lib.option_scope(x3p8=0):
        r4, _ = run_epilogues(c, tag + ' 4-wave')
    same = _same(r8, r4)
    print('%-34s 8-wave vs 4-wave tile: %s' % (tag, 'bit-identical' if same else 'DIFFER, distance %.2e' % _dist(r8, r4)))
    assert same
    if ((rows + 127) // 128) * ((cout + 127) // 128) * B >= 256:
        _in_kernel_split(c, tag, r8)


def test_wide_conv_cin_pad_96_takes_the_4_wave_tile():
    """cin 80 -> cin_pad 96, N = 128: (E) fails on cin_pad % 64 under the DEFAULT options -> (F) gemm_x3p_kernel<128,128>; a K-step of 32 then crosses taps every third step."""
    c = Conv(80, 128, 7, 3, 9001)
    run_epilogues(c, '80>128 k7 d3 M9001 (cin_pad 96)')


# ---- A / D: N <= 64 -----------------------------------------------------------------------------------------------------------------------------------------------

NARROW = [(64, 64, 7, 3, 4001, 1), (64, 64, 11, 5, 1000, 1), (64, 18, 7, 1, 3001, 1), (32, 32, 3, 1, 2500, 1), (32, 32, 11, 5, 4000, 1), (128, 64, 7, 1, 3999, 1),
          (64, 64, 7, 3, 2001, 2), (64, 18, 7, 1, 1501, 2),
          (64, 64, 3, 1, 5003, 2)]             # batch 2 at M >= 4096: (R) needs batch == 1, so this stays on the tiled form


@pytest.mark.parametrize('cin,cout,k,dil,rows,B', NARROW)
def test_narrow_convs_128x64_tile(cin, cout, k, dil, rows, B):
    """N <= 64 and (R) fails (M < 4096, or cin_pad != 64, or batch 2) -> (S) gemm_x3p_kernel<128,64,32,64>: 64 -> 64 and 64 -> 18 (conv_post: 14 pad columns to zero)
    below 4096 rows, cin_pad 32, N = 64 exactly, batch 2 below and above 4096 rows."""
    c = Conv(cin, cout, k, dil, rows, B=B)
    run_epilogues(c, '%d>%d k%d d%d M%d B%d' % (cin, cout, k, dil, rows, B))


C64 = [(64, k, d) for k in (3, 7, 11) for d in (1, 3, 5)] + [(18, 7, 1)]


@pytest.mark.parametrize('rows', [4096, 4097, 120 * 301 + 1, 4095])
@pytest.mark.parametrize('cout,k,dil', C64 + [(64, 11, 7)])
def test_last_stage_convs_resident_rows_vs_tiled(cout, k, dil, rows):
    """cin_pad 64, N <= 64, batch 1: M >= 4096 with a halo of at most 64 rows -> (R) conv64_x3p_kernel<192> (4096 rows: 32 whole tiles; 4097: one row in the last
    tile; 120 T + 1: the product's row count); M = 4095 -> (S); (k 11, dil 7): 128 + 70 > 192 -> (S) at every row count.  conv64_resident = 0 sends all of them to (S):
    the two forms sum the same products in the same order (test_gpu_fullsize.py asserts it for the whole model), so every output of every epilogue is torch.equal.
    fp32 operands with x3 take gemm_x3_kernel<128,64> above 4096 rows."""
    _lib = _mods()[0]
    c = Conv(64, cout, k, dil, rows)
    tag = '64>%d k%d d%d M%d' % (cout, k, dil, rows)
    with _lib.option_scope(conv64_resident=1):
        r1, _ = run_epilogues(c, tag + ' resident')
    with _lib.option_scope(conv64_resident=0):
        r0, _ = run_epilogues(c, tag + ' tiled')
    for key in r1:
        assert torch.equal(r1[key], r0[key]), (tag, key, 'conv64_resident 1 vs 0 differ')
    if rows > 4096:
        _in_kernel_split(c, tag, r1)


# ---- A: up-sampling convolutions ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('cin,cout,k,up,lprev', [(512, 256, 16, 8, 2501), (256, 128, 11, 5, 8003), (128, 64, 7, 3, 12001)])
def test_upsampling_convs_on_planes(cin, cout, k, up, lprev):
    """Nearest up-sampling folded into the A index map (src = idx / up), a_plane = Lprev * Cpp, + fp32 res, as decode_impl launches them: 512 -> 256 and 256 -> 128
    take (E) / (F) with x3p8 1 / 0; 128 -> 64 has N <= 64 but up != 1, so (R) fails -> (S) even at 36 003 rows.  Reference: F.interpolate(nearest), then the causal conv."""
    _lib = _mods()[0]
    c = Conv(cin, cout, k, 1, lprev, up=up)
    tag = '%d>%d k%d up%d M%d' % (cin, cout, k, up, c.M)
    for x3p8 in (1, 0) if cout > 64 else (1,):
        with _lib.option_scope(x3p8=x3p8):
            o = c.buf(False)
            c.launch(res=c.res, out=o.view)
            o.check(cout, tag)
            e = _err(o, cout, c.lin + c.r64)
            print('%-34s x3p8 %d  + res -> fp32 %.2e' % (tag, x3p8, e))
            assert e < BOUND, (tag, e)
            run_epilogues(c, tag + ' x3p8 %d' % x3p8)


def test_last_stage_upsampling_pair_of_launches_with_the_reflection_row():
    """The last stage's up-sampling convolution exactly as decode_impl issues it (128 -> 64, up 3, k 7; (S) for both launches): the full launch with out_row_off =
    res_row_off = 1 writes rows 1 .. Lup, then M = 2 with both offsets -1 writes row 0 = x_up[1] + si[0] and must SKIP its row m = 0 (shifted index -1: the guard in
    front).  The combined [Lup + 1] buffer is held to the float64 value of reflect-pad(1, 0)(x_up) + si."""
    lprev, up = 12001, 3
    c = Conv(128, 64, 7, 1, lprev, up=up)
    L = c.M + 1
    si = torch.zeros(1, L, 64, device=DEV)
    si[:] = _rand(1, L, 64, seed=7).to(DEV)
    o = c.buf(False, rows=L)
    c.launch(res=si, res_row_off=1, out=o.view, out_row_off=1)
    o.check(64, 'full launch, row offset 1', first_row=1)
    assert bool((o.owned()[:, 0] == SENT32).all()), 'row 0 belongs to the second launch'
    c.launch(res=si, res_row_off=-1, out=o.view, out_row_off=-1, m_out=2)
    o.check(64, 'M = 2, row offset -1')
    ref = torch.cat([c.lin[:, 1:2], c.lin], dim=1) + si.double()
    e = _err(o, 64, ref)
    e0 = ((o.value(64)[:, 0] - ref[:, 0]).abs().max() / ref.abs().max()).item()
    print('reflect-pad(1,0)(x_up) + si: %.2e of the scale (row 0 alone %.2e)' % (e, e0))
    assert e < BOUND, e


def test_second_output_at_its_own_row_offset():
    """out2_row_off != out_row_off (GemmArgs keeps one offset per output): convs2's launch with out at offset 0 and the pair out2 two rows down, on (E) and on (R);
    each output's guards and its unwritten first rows stay untouched."""
    _lib = _mods()[0]
    for c, tag in ((Conv(256, 256, 3, 1, 5003), '(E)'), (Conv(64, 64, 7, 3, 5003), '(R)')):
        o, o2 = c.buf(False), c.buf(True, rows=c.M + 2)
        c.launch(res=c.res, out=o.view, out2=o2.view, out2_row_off=2, act2=_lib.ACT_SNAKE, act2_alpha=c.a2, out2_plane=o2.plane)
        o.check(c.cout, tag + ' out')
        o2.check(c.cout, tag + ' out2', first_row=2)
        assert bool((o2.owned()[:, :, :2] == SENT16).all()), 'rows above out2_row_off were written'
        v = c.lin + c.r64
        ref2 = _snake(v, c.a2.double())
        e, e2 = _err(o, c.cout, v), ((o2.value(c.cout)[:, 2:] - ref2).abs().max() / ref2.abs().max()).item()
        print('%s out %.2e, out2 at row offset 2 %.2e' % (tag, e, e2))
        assert e < BOUND and e2 < BOUND, (tag, e, e2)


# ---- B: the plane-pair store is exact by definition -----------------------------------------------------------------------------------------------------------------

def _assert_pair_is_split_of(pair_bits, f32_bits, n, what):
    """bit for bit: hi == bf16(v), lo == bf16(v - float(hi)) (packing.split_planes is the one definition of the format)"""
    packing = _mods()[2]
    want = packing.split_planes(f32_bits.view(torch.float32)[..., :n].contiguous()).view(torch.int16)
    got = pair_bits[..., :n]
    assert torch.equal(got[0], want[0]), what + ': hi plane != bf16(fp32 result)'
    assert torch.equal(got[1], want[1]), what + ': lo plane != bf16(fp32 result - hi)'


@pytest.mark.parametrize('form,cin,cout,k,dil,rows,opts', [
    ('8-wave, lean + vector passes', 256, 256, 3, 1, 5003, {}),
    ('4-wave, lean + vector passes', 256, 256, 3, 1, 5003, {'x3p8': 0}),
    ('8-wave, partial column tile', 256, 200, 3, 1, 3001, {}),
    ('128x64, lean + vector passes', 64, 64, 7, 3, 3001, {}),
    ('128x64, N = 18', 64, 18, 7, 1, 3001, {}),
    ('resident, lean + vector passes', 64, 64, 7, 3, 5003, {}),
    ('resident, N = 18', 64, 18, 7, 1, 5003, {})])
def test_pair_store_equals_split_of_the_fp32_store(form, cin, cout, k, dil, rows, opts):
    """gemm_epilogue.h writes a pair in three places: the lean pass (whole aligned column tiles, one residual: epilogues 1, 2 and the run-time mode), the vector pass
    of do_pass (res2 / div, or a tile the lean conditions refuse) and its element-wise branch (a partial column tile: N = 18, N = 200).  The same launch with fp32
    outputs and with pair outputs must give hi == bf16(out32), lo == bf16(out32 - hi) bit for bit, on (E), (F), (S) and (R)."""
    _lib = _mods()[0]
    c = Conv(cin, cout, k, dil, rows)
    with _lib.option_scope(**opts):
        rp, _ = run_epilogues(c, form + ' pair')
        rf, _ = run_epilogues(c, form + ' fp32', pair_out=False)
    for key in ('snake[0]', 'res+snake2[1]', 'mean3[1]', 'mean3, out null[0]'):
        _assert_pair_is_split_of(rp[key], rf[key], cout, '%s, %s' % (form, key))
    for key in ('res+snake2[0]', 'res+res2[0]', 'mean3[0]', 'bias[0]'):
        assert torch.equal(rp[key], rf[key]), (form, key, 'the fp32 output changed with the form of the other output')


@pytest.mark.parametrize('cin,cout,rows,opts', [(256, 256, 3001, {}), (256, 256, 3001, {'x3p8': 0}), (64, 64, 3001, {}), (64, 64, 5003, {})])
def test_pair_store_scalar_pass_unaligned_leading_dimension(cin, cout, rows, opts):
    """A leading dimension that is not a multiple of 4 elements (ldo = N + 2) fails the 16-byte test of gemm_epilogue.h (`vec`), so every access of the pass is scalar
    and a pair leaves through store_planes1.  launch_gemm accepts such an output; the pair must still be the exact split of the fp32 result, the fp32 result the
    same values as with an aligned ldo, and the two spare columns of every row untouched."""
    _lib = _mods()[0]
    c = Conv(cin, cout, 3, 1, rows)
    with _lib.option_scope(**opts):
        outs = {}
        for pair in (True, False):
            o, o2 = c.buf(False, ld=cout + 2, cols=cout), c.buf(pair, ld=cout + 2, cols=cout)
            c.launch(res=c.res, out=o.view, out2=o2.view, act2=_lib.ACT_SNAKE, act2_alpha=c.a2, **({'out2_plane': o2.plane} if pair else {}))
            o.check(cout, 'scalar pass out')
            o2.check(cout, 'scalar pass out2')
            outs[pair] = (o.owned().clone(), o2.owned().clone())
        al = c.buf(False)
        c.launch(res=c.res, out=al.view)
    v = c.lin + c.r64
    e = ((outs[True][0].view(torch.float32)[..., :cout].double() - v).abs().max() / v.abs().max()).item()
    print('%d>%d M%d %s scalar pass: fp32 out %.2e of the scale' % (cin, cout, rows, opts, e))
    assert e < BOUND
    assert torch.equal(outs[True][0], outs[False][0])
    assert torch.equal(outs[True][0][..., :cout], al.owned()[..., :cout]), 'the scalar and the vector pass store different fp32 values'
    _assert_pair_is_split_of(outs[True][1], outs[False][1], cout, 'scalar pass')


@pytest.mark.parametrize('rows,C', [(36121, 64), (40003, 128), (4507, 256), (1000, 8)])
def test_act_rows_pair_equals_split_of_fp32(rows, C):
    """elementwise.hip: act_rows_planes_kernel (the Snake of x_raw in front of every ResBlock; hvx_op_act_rows with planes) against act_rows_kernel<float> bit for bit
    — Snake with a per-channel alpha, and LeakyReLU — and the fp32 kernel against float64.  cols = C inside rows of Cp elements, as the product calls it."""
    _lib, ops, packing = _mods()
    cp = _pad32(C)
    x = torch.zeros(rows, cp, device=DEV)
    x[:, :C] = (_rand(rows, C, seed=11) * 2.0).to(DEV)
    alpha = (_rand(C, seed=12).abs() + 0.1).to(DEV)
    for act, kw, ref in ((_lib.ACT_SNAKE, dict(alpha=alpha), _snake(x[:, :C].double(), alpha.double())),
                         (_lib.ACT_LRELU, dict(act_param=SLOPE), torch.where(x[:, :C] >= 0, x[:, :C].double(), x[:, :C].double() * SLOPE))):
        o32, op = Buf(1, rows, cp, False, cols=C), Buf(1, rows, cp, True, cols=C)
        ops.act_rows(x[:, :C], act, out=o32.view[0], **kw)
        ops.act_rows(x[:, :C], act, out=op.view[0], plane=op.plane, **kw)
        for bf in (o32, op):                 # (columns [C, Cp) belong to nobody here: cols == out_cols == C)
            bf.check(C, 'act_rows %d' % act)
        e = ((o32.value(C)[0] - ref).abs().max() / ref.abs().max()).item()
        print('act_rows act %d [%d][%d]: fp32 vs float64 %.2e of the scale' % (act, rows, C, e))
        assert e < BOUND
        _assert_pair_is_split_of(op.owned(), o32.owned(), C, 'act_rows act %d' % act)


def test_split_planes_represents_fp32_to_2_pow_minus_17():
    """|x - (hi + lo)| <= 2^-17 |x| over 1 M values spanning 1e-6 .. 1e6 and both signs (the figure csrc/hvx_kernels.h states for the format; measured 7.61e-6 < 2^-17 =
    7.63e-6), for packing.split_planes on the device — the function the product builds its weight planes with."""
    packing = _mods()[2]
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(1 << 20, generator=g) * 2 - 1) * torch.pow(10.0, torch.rand(1 << 20, generator=g) * 12 - 6)
    x = x.float().to(DEV)
    p = packing.split_planes(x)
    assert p.dtype == torch.bfloat16 and p.shape == (2, 1 << 20)
    assert torch.equal(p[0], x.to(torch.bfloat16))
    rel = ((x.double() - (p[0].double() + p[1].double())).abs() / x.double().abs()).max().item()
    print('split_planes: max |x - (hi + lo)| / |x| = %.3e (2^-17 = %.3e)' % (rel, 2.0 ** -17))
    assert rel <= 2.0 ** -17


def test_pair_operands_need_both_operands_as_pairs():
    """launch_gemm_x3 refuses a launch with only one operand as a pair (plane pairs cannot fall back to an fp32 kernel)"""
    _lib, ops, packing = _mods()
    c = Conv(64, 64, 3, 1, 300)
    with pytest.raises(_lib.HvxError, match='both operands must be plane pairs'):
        ops.conv1d(c.xp, c.w32, c.b, n_out=64, taps=3, cin_pad=64, pad_left=2, a_plane=300 * 64)
