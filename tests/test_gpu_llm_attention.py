"""The LM layers' cache attention, launch form by launch form against float64: csrc/attention.hip attn_fwd_kernel in the nine instantiations launch_t picks from
(one / two query tiles, with / without the in-workgroup merge of the key splits' waves, four / eight waves, fragment-order / row-major caches) and
attn_combine_kernel, through ops.llm_attention with the geometry hvx_llm_forward launches — GQA-packed rows r = rh kn + rl (G = 7 query heads per KV head, 2 KV
heads, head_dim 64, scale 0.125), a 4-slot cache of 1024 keys read through kv_slot = [2, 0, 3], per-sequence pos0 / kv_len / n_valid_lo, the strides of
csrc/hvx_llm.hip — and the consumer of its partials, the combining form of gemm_narrow_resid_kernel (csrc/gemm_skinny.hip), through ops.decode_gemm(w_narrow, att_o).
tests/test_gpu_fullsize.py and the oracle parity tests see these kernels through whole models; here every launch is held to the mathematics.

Operands are built on the CPU in bf16 or fp32, the reference is float64 FROM THOSE VALUES: out[b kn + rl, (h G + rh) 64 + d] = softmax_j(scale q . k_j) . v_j over
j < min(kv_len[b], pos0[b] + rl + 1) of slot kv_slot[b]; rows rl >= n_valid_lo[b] are not written.  Caches are laid out with packing.kfrag / vfrag and fragment-order
outputs decoded with packing.unfrag_rows (tests/test_host_cpu.py holds those to the index formulas), never with the kernels' addressing.  Every element is compared;
a sentinel fills all that must not be written; cache positions at and beyond kv_len and the whole unused slot hold +-2^40 (finite: the kernel multiplies padded V
columns by p == 0), so a leaked key shows.  So that ONE wrong key shows as well, the keys pos0 - 1 .. pos0 + kn - 1 of a sequence (the last visible key of every row,
and the first invisible one of every row but the last, whose first invisible key is poison) and four keys at random positions score 4 units above the rest: each
carries percents of its row's weight at any context length.

Visible ends pos0 + kn, mixed over the three sequences of a launch (C = split_chunk, c = sub_chunk; 256 / 64 stand in where a form has no split): kn, 31, 32, 33, 63,
64, 65, c - 1, c, c + 1, C - 1, C, C + 1, 2 C + 17, 1024 — those >= kn, and 2 C + 17 = 1041 does not exist in a 1024-key cache at C = 512; n_valid_lo cycles through
kn, kn - 1, 1; one launch has kv_len < pos0 + kn in two sequences, one has every sequence inside the first split.  With the hvx_llm.hip strides the grid covers all
896 columns of `out`: the sentinel is held in the rows behind the grid (and in the padding rows of a fragment-order `out`).

Bounds (U = 2^-24, UB = 2^-8; per row: n visible keys, s_j the float64 scores, m = max s_j, R = m - min s_j, p_j = exp(s_j - m), ref = sum p v / sum p,
A = sum p |v| / sum p >= |ref|, per element d):
  scores: an fp32 sum of 64 products (exact for bf16 operands: kd = 64 roundings; fp32 operands: kd = 65), times the scale (one rounding, U |s|):
      d_m = max_j (kd U scale sum_d |q_d k_jd| + U |s_j|)                                — also the bound of the stored maximum m of a partial;
  p_j = expf(s_j - m'), m' the running maximum (s_j <= m' <= m): the argument's rounding U (m - s_j), expf 1 ulp = 2 U.  Whenever the maximum moves, at the merge of
  the waves and at the combine of the splits, the state is multiplied by expf(m_old - m_new): the SAME factor on sum p v and sum p, so what it leaves is a relative
  perturbation of the older keys' weights — 2 U (expf) + U (the product), and the arguments' roundings, which add up to U R per chain (walk, merge, combine):
      d_s = max_j (kd U scale sum_d |q_d k_jd| + U |s_j| + U (m - s_j)) + 2 U + 3 U R,        steps = ceil(n / 32) + 1 (walk) + 1 (merge) + 1 (combine)
  a relative perturbation eps_j of the weights moves sum p v / sum p by at most (A + |ref|) max |eps_j| <= 2 A max |eps_j|: hence 2 d_s and c_e = 2 * 3 = 6;
  bf16: P is rounded to bf16 for the PV product ONLY (the row sum adds the unrounded p): UB sum p |v|, c_P = 1;
  the fp32 sums over n keys: (n + 1) U sum p |v| in the numerator (the fp32 form also rounds its products), n U in the row sum, |ref| <= A: c_n n -> 2 n + 2;
  the division by the row sum: 1 / l and a product, or a division: 4 U |ref|;
      eps = [UB] + (2 n + 2) U + 2 d_s + 6 U steps,      e = eps / (1 - eps) A + 4 U |ref|,      |got - ref| <= e (fp32),   UB |ref| + (1 + UB) e (bf16: one last rounding).
  Partials (skip_combine = 1; m_s, l_s, o_s the float64 state over that split's visible keys of the row): |o / l - o_s / l_s| <= e of the split (fp32, no last
  rounding), |l exp(m - m_s) - l_s| <= l_s eps_l / (1 - eps_l) with eps_l = n U + d_s + 3 U steps, |m - m_s| <= d_m.
  The narrow o_proj behind the attention: |x - ref| <= B |W|^T + K U (|a| + B) |W|^T + 2 U |ref|, a the float64 attention rows and B their bound above; its 16-bit copy
  UB |ref| + (1 + UB) that.
test_fp32_emulation_stays_inside_the_bounds (CPU) runs an fp32 emulation of the kernel's arithmetic — 32-key steps with an online maximum, bf16 P, the waves' merge,
then the splits' combine, each in the kernel's order — through the same bounds: they hold without a device, for the seeds used here.

Worst error / bound measured on an MI355X (`out` / partials; 44 form x dtype cases, 6 or 7 launches each, every one inside its bounds; no kernel bug found):
  merge, one tile, 4 waves (fragment cache)      bf16 0.66 / 0.74    fp32 0.020 / 0.072        the same over a row-major cache   bf16 0.66 / 0.74    fp32 0.016 / 0.052
  merge, one tile, 8 waves                       bf16 0.66 / 0.74    fp32 with n_sub = 8 (falls back to 4 waves: merge at c = 128, whole splits at c = 64) 0.020 / 0.072
  merge, two tiles                               bf16 0.79 / 0.85    fp32 0.021 / 0.072        row-major                         bf16 0.69 / 0.85    fp32 0.015 / 0.065
  splits without merge (35 / 56 rows)            bf16 0.75 / 0.73    fp32 0.020 / 0.074        row-major                         bf16 0.75 / 0.73    fp32 0.017 / 0.074
  no split, one tile (84 rows)                   bf16 0.76           fp32 0.025                row-major: the same figures
  no split, two tiles (280 rows)                 bf16 0.79           fp32 0.019                row-major: the same figures
  fragment-order `out` (bf16)                    the figures of the row-major `out` of the same form, store and combine
  o_proj, combining = combine launch + plain     bit-identical in all 12 cases; stream 0.50, 16-bit copy 0.995 (rows that are not active: x0 + bias, one rounding each)
The bf16 figures are the UB term nearly attained where few keys carry a row's weight (the fp32 emulation reaches 0.82 / 0.76 the same way).
"""
import functools
import math

import pytest
import torch

from flowmirror_hydravox_amd import _lib, ops, packing
from flowmirror_hydravox_amd._lib import SK_RESID

gpu = pytest.mark.gpu

G, KVH = 7, 2
QH = G * KVH
Q = QH * 64                      # 896
CTX, NSLOT = 1024, 4
SLOTS = (2, 0, 3)                # three sequences, slot 1 unused (all poison)
SCALE = 0.125
U = 2.0 ** -24
UB = 2.0 ** -8
SENT = -77.0                     # exact in bf16
POISON = 2.0 ** 40
BF, F32 = torch.bfloat16, torch.float32
DT = {'bf16': BF, 'fp32': F32}


# ================================================================================================================================================
# operands, positions, the float64 reference and its bounds
# ================================================================================================================================================
def _poison(shape):
    n = 1
    for s in shape:
        n *= s
    return (POISON * (1.0 - 2.0 * (torch.arange(n) % 2))).view(*shape)


@functools.lru_cache(maxsize=2)
def _base(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(NSLOT, KVH, CTX, 64, generator=g), torch.randn(NSLOT, KVH, CTX, 64, generator=g)


def _position_sets(kn, C, c):
    """[(pos0, kv_len, n_valid_lo)] per launch, three sequences each"""
    ends = sorted(e for e in {kn, 31, 32, 33, 63, 64, 65, c - 1, c, c + 1, C - 1, C, C + 1, 2 * C + 17, CTX} if kn <= e <= CTX)
    while len(ends) % 3:
        ends.insert(len(ends) // 2, ends[len(ends) // 2])
    n = len(ends) // 3
    nv = [kn, max(kn - 1, 1), 1]
    sets = []
    for i in range(n):
        e = [ends[i], ends[i + n], ends[i + 2 * n]]
        e = e[i % 3:] + e[:i % 3]                                            # the long sequence is not always the last
        sets.append(([x - kn for x in e], e, [nv[(i + b) % 3] for b in range(3)]))
    # kv_len the binding limit in sequences 0 and 1
    e = [x for x in (C + 1, 65, min(2 * C + 17, CTX)) if x >= kn + 1] + [CTX] * 3
    e = e[:3]
    sets.append(([x - kn for x in e], [e[0] - 1, max(e[1] // 2, 1), e[2]], [kn, kn, max(kn - 1, 1)]))
    # every sequence short: all splits but the first are dead
    e = [kn, max(33, kn), max(min(c + 1, C), kn)]
    sets.append(([x - kn for x in e], e, [kn, 1, kn]))
    return sets


def _operands(dt, kn, pos0, kv_len, n_valid, slots, seed):
    """q [n_seq][kn][QH][64], K / V caches [NSLOT][KVH][CTX][64] in dt: values below kv_len of every sequence's slot, poison everywhere else"""
    n_seq = len(slots)
    g = torch.Generator().manual_seed(seed)
    K0, V0 = _base(1 + seed % 2)
    q = torch.randn(n_seq, kn, QH, 64, generator=g) + 0.5
    kc, vc = _poison((NSLOT, KVH, CTX, 64)), -_poison((NSLOT, KVH, CTX, 64))
    for b, s in enumerate(slots):
        n = kv_len[b]
        kb = K0[s, :, :n].clone()
        hot = [j for j in range(pos0[b] - 1, pos0[b] + kn) if 0 <= j < n] + [int(j) for j in torch.randint(0, n, (4,), generator=g)]
        kb[:, hot] += 1.0                                                    # q . k grows by 0.5 * 64: 4 score units
        kc[s, :, :n], vc[s, :, :n] = kb, V0[s, :, :n]
        for rl in range(n_valid[b], kn):
            q[b, rl] = _poison((QH, 64))                                     # rows that are not valid are not even read
    return q.to(dt), kc.to(dt), vc.to(dt)


def _state(qd, Kd, Vd, lim, lo, hi, kd):
    """float64 softmax state of rows qd [R][64] over the keys lo <= j < min(hi, lim[r]) of Kd / Vd [n][64]"""
    hi = max(min(hi, Kd.shape[0]), lo)
    j = torch.arange(lo, hi)
    vis = j[None, :] < lim[:, None]
    Ks, Vs = Kd[lo:hi], Vd[lo:hi]
    s = SCALE * (qd @ Ks.t())
    mag = SCALE * (qd.abs() @ Ks.abs().t())
    ninf, zero = torch.full_like(s, -math.inf), torch.zeros_like(s)
    n = vis.sum(1)
    m = torch.where(vis, s, ninf).amax(1) if hi > lo else torch.full((qd.shape[0],), -math.inf, dtype=torch.float64)
    ms = torch.where(n > 0, m, torch.zeros_like(m))
    p = torch.where(vis, (s - ms[:, None]).exp(), zero)
    smin = torch.where(vis, s, -ninf).amin(1) if hi > lo else ms
    R = torch.where(n > 0, ms - smin, torch.zeros_like(ms))
    ds_j = torch.where(vis, kd * U * mag + U * s.abs(), zero)
    d_m = ds_j.amax(1) if hi > lo else torch.zeros_like(ms)
    d_s = (torch.where(vis, ds_j + U * (ms[:, None] - s), zero).amax(1) if hi > lo else torch.zeros_like(ms)) + 2 * U + 3 * U * R
    return dict(n=n, m=m, l=p.sum(1), o=p @ Vs, oa=p @ Vs.abs(), d_m=d_m, d_s=d_s)


def _err(st, bf, final):
    """-> (ref, bound of the normalised output, eps_l) of a state; final: the bound of the value rounded to the output type, else of the fp32 quotient"""
    n = st['n'].double()
    steps = torch.ceil(n / 32) + 3
    live = st['n'] > 0
    l = torch.where(live, st['l'], torch.ones_like(st['l']))[:, None]
    ref, A = st['o'] / l, st['oa'] / l
    eps = ((UB if bf else 0.0) + (2 * n + 2) * U + 2 * st['d_s'] + 6 * U * steps)[:, None]
    e = eps / (1 - eps) * A + 4 * U * ref.abs()
    if final and bf:
        e = UB * ref.abs() + (1 + UB) * e
    return ref, e, n * U + st['d_s'] + 3 * U * steps


class Case:
    """one launch: controls, operands, the float64 reference of `out` and of every split's partial"""

    def __init__(self, dt, kn, pos0, kv_len, n_valid, C, merge, slots=SLOTS, seed=0):
        self.dt, self.kn, self.n_seq, self.slots = dt, kn, len(slots), slots
        self.pos0, self.kv_len, self.n_valid = pos0, kv_len, n_valid
        self.n_rows, self.C, self.S = G * kn, C, (CTX // C if C else 1)
        self.npad = 32 if self.n_rows <= 32 else max(64, self.n_rows)               # (hvx_llm_bind's att_rows_pad: 32 or 64; no partials beyond 64 rows)
        self.q, self.kc, self.vc = _operands(dt, kn, pos0, kv_len, n_valid, slots, seed)
        bf, kd = dt == BF, 64 if dt == BF else 65
        M, R, S = self.n_seq * kn, self.n_rows, self.S
        self.ref, self.bound, self.mask = torch.zeros(M, Q, dtype=torch.float64), torch.zeros(M, Q, dtype=torch.float64), torch.zeros(M, Q, dtype=torch.bool)
        z = lambda *t: torch.zeros(self.n_seq, KVH, S, self.npad, *t, dtype=torch.float64)
        self.p_ref, self.p_e, self.p_m, self.p_dm, self.p_l, self.p_el = z(64), z(64), z(), z(), z(), z()
        self.p_state = torch.zeros(self.n_seq, KVH, S, self.npad, dtype=torch.int8)          # 0 not asserted on, 1 value, 2 sentinel
        self.p_state[:, :, :, R:] = 2
        r = torch.arange(R)
        rh, rl = r // kn, r % kn
        for b, slot in enumerate(slots):
            lim = torch.minimum(torch.tensor(kv_len[b]), pos0[b] + rl + 1)
            ok = rl < n_valid[b]
            for h in range(KVH):
                qd = self.q[b, rl, h * G + rh].double()
                Kd, Vd = self.kc[slot, h, :kv_len[b]].double(), self.vc[slot, h, :kv_len[b]].double()
                ref, e, _ = _err(_state(qd, Kd, Vd, lim, 0, CTX, kd), bf, True)
                rows, cols = (b * kn + rl)[ok], ((h * G + rh)[ok, None] * 64 + torch.arange(64)[None, :])
                self.ref[rows[:, None], cols], self.bound[rows[:, None], cols], self.mask[rows[:, None], cols] = ref[ok], e[ok], True
                self.p_state[b, h, :, :R][:, ~ok] = 2
                for s in range(S if S > 1 else 0):
                    if merge and s * C >= min(kv_len[b], pos0[b] + kn):
                        self.p_state[b, h, s] = 2                                # a dead workgroup of the merge forms leaves at once
                        continue
                    st = _state(qd, Kd, Vd, lim, s * C, (s + 1) * C, kd)
                    pr, pe, el = _err(st, bf, False)
                    live = ok & (st['n'] > 0)
                    self.p_state[b, h, s, :R][live] = 1
                    self.p_ref[b, h, s, :R], self.p_e[b, h, s, :R], self.p_el[b, h, s, :R] = pr, pe, el
                    self.p_m[b, h, s, :R], self.p_dm[b, h, s, :R], self.p_l[b, h, s, :R] = torch.where(live, st['m'], torch.zeros_like(st['l'])), st['d_m'], st['l']

    def controls(self):
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device='cuda')
        return dict(kv_slot=i32(self.slots), kv_len=i32(self.kv_len), pos0=i32(self.pos0), n_valid_lo=i32(self.n_valid))


WORST = {}


def _ratio(form, what, err, bound):
    form = form + (' bf16' if ' bf16 ' in what + ' ' else ' fp32' if ' fp32 ' in what + ' ' else '')
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    WORST[form] = max(WORST.get(form, 0.0), worst)
    bad = int((~(err <= bound)).sum())                                       # (NaN fails)
    print('%s: %d elements, worst error / bound %.3f' % (what, err.numel(), worst))
    assert err.numel() > 0 and bad == 0, '%s: %d of %d elements outside the bound, worst error / bound %.3f' % (what, bad, err.numel(), worst)


def _check_out(form, what, got, case):
    """got [rows >= n_seq kn][Q]: every written element inside its bound, the sentinel everywhere else"""
    got = got.double()
    M = case.n_seq * case.kn
    mask = torch.cat([case.mask, torch.zeros(got.shape[0] - M, Q, dtype=torch.bool)])
    rest = got[~mask]
    assert bool((rest == SENT).all()), '%s: %d elements outside the result were written' % (what, int((rest != SENT).sum()))
    _ratio(form, what, (got[:M] - case.ref).abs()[case.mask], case.bound[case.mask])


def _check_partials(form, what, po, pm, case):
    po, pm = po.double().cpu().view(case.n_seq, KVH, case.S, case.npad, 64), pm.double().cpu().view(case.n_seq, KVH, case.S, case.npad, 2)
    dead, live = case.p_state == 2, case.p_state == 1
    assert bool((po[dead] == SENT).all()) and bool((pm[dead] == SENT).all()), '%s: partials of dead splits / rows were written' % what
    m, l = pm[..., 0][live], pm[..., 1][live]
    _ratio(form, what + ' o/l', (po[live] / l[:, None] - case.p_ref[live]).abs(), case.p_e[live])
    el = case.p_el[live]
    _ratio(form, what + ' l', (l * (m - case.p_m[live]).exp() - case.p_l[live]).abs(), case.p_l[live] * el / (1 - el))
    _ratio(form, what + ' m', (m - case.p_m[live]).abs(), case.p_dm[live])


def _launch(case, *, frag, c=0, n_sub=4, skip=False, ofrag=False, out=None, po=None, pm=None, **over):
    """one ops.llm_attention launch with the strides of csrc/hvx_llm.hip -> (out [rows][Q] decoded on the CPU, part_o, part_ml)"""
    dt, kn, n_seq = case.dt, case.kn, case.n_seq
    M = n_seq * kn
    rows = ((M + 15) // 16 * 16 + 16) if ofrag else M + 3
    kc, vT = case.kc, case.vc.transpose(-1, -2).contiguous()
    kd, vd = (packing.kfrag(kc), packing.vfrag(vT)) if frag else (kc, vT)
    sent = lambda n, t: torch.full((n,), SENT, dtype=t, device='cuda')
    if out is None:
        out = sent(rows * Q, dt)
    rows = out.numel() // Q
    if case.S > 1:
        po = sent(n_seq * KVH * case.S * case.npad * 64, F32) if po is None else po
        pm = sent(n_seq * KVH * case.S * case.npad * 2, F32) if pm is None else pm
    kw = dict(batch=n_seq, heads=KVH, n_rows=case.n_rows, kn=kn, q_strides=(kn * Q, G * 64, 64, Q), k_strides=(KVH * CTX * 64, CTX * 64),
              v_strides=(KVH * CTX * 64, 64 * CTX), v_ld=CTX, o_strides=(kn * Q, G * 64, 64, Q), causal=True, scale=SCALE, n_splits=case.S, split_chunk=case.C,
              n_sub=n_sub, sub_chunk=c, part_o=po, part_ml=pm, n_rows_pad=case.npad if case.S > 1 else 0, skip_combine=skip, kv_frag=frag,
              o_frag_kt=Q // 32 if ofrag else 0, **case.controls())
    kw.update(over)
    ops.llm_attention(case.q.cuda().contiguous(), kd.contiguous().cuda(), vd.contiguous().cuda(), out, **kw)
    torch.cuda.synchronize()
    o = out.cpu()
    return (packing.unfrag_rows(o, rows, Q) if ofrag else o.view(rows, Q)), po, pm


# form id -> (kn, fragment-order cache, split_chunk, sub_chunk, n_sub, merge form, fragment-order out, dtypes)
BOTH = ('bf16', 'fp32')
FORMS = {}
for _kn in (1, 2):
    for _C, _c in ((256, 64), (512, 128)):
        FORMS['merge-1tile-frag-kn%d-C%d-c%d' % (_kn, _C, _c)] = (_kn, True, _C, _c, 4, True, False, BOTH)
    FORMS['merge-1tile-8waves-frag-kn%d-C512-c64' % _kn] = (_kn, True, 512, 64, 8, True, False, ('bf16',))
    # fp32 with n_sub = 8: launch_attention falls back to four waves — 4 x 128 is the split again (the merge form), 4 x 64 is not (the waves then own whole splits)
    FORMS['fp32-nsub8-falls-back-frag-kn%d-C512-c128' % _kn] = (_kn, True, 512, 128, 8, True, False, ('fp32',))
    FORMS['fp32-nsub8-falls-back-frag-kn%d-C512-c64' % _kn] = (_kn, True, 512, 64, 8, False, False, ('fp32',))
for _kn in (3, 4):
    for _C, _c in ((256, 64), (512, 128)):
        FORMS['merge-2tile-frag-kn%d-C%d-c%d' % (_kn, _C, _c)] = (_kn, True, _C, _c, 4, True, False, BOTH)
for _kn in (5, 8):
    FORMS['split-nomerge-1tile-frag-kn%d-C256' % _kn] = (_kn, True, 256, 64, 4, False, False, BOTH)
FORMS['nosplit-1tile-frag-kn12'] = (12, True, 0, 0, 4, False, False, BOTH)
FORMS['nosplit-2tile-frag-kn40'] = (40, True, 0, 0, 4, False, False, BOTH)
FORMS['merge-1tile-rowmajor-kn2-C256-c64'] = (2, False, 256, 64, 4, True, False, BOTH)
FORMS['merge-2tile-rowmajor-kn4-C256-c64'] = (4, False, 256, 64, 4, True, False, BOTH)
FORMS['split-nomerge-1tile-rowmajor-kn5-C256'] = (5, False, 256, 64, 4, False, False, BOTH)
FORMS['nosplit-1tile-rowmajor-kn12'] = (12, False, 0, 0, 4, False, False, BOTH)
FORMS['nosplit-2tile-rowmajor-kn40'] = (40, False, 0, 0, 4, False, False, BOTH)
FORMS['ofrag-nosplit-1tile-frag-kn12'] = (12, True, 0, 0, 4, False, True, ('bf16',))
FORMS['ofrag-nosplit-2tile-frag-kn40'] = (40, True, 0, 0, 4, False, True, ('bf16',))
FORMS['ofrag-combine-merge-1tile-frag-kn2-C256-c64'] = (2, True, 256, 64, 4, True, True, ('bf16',))
FORMS['ofrag-combine-split-nomerge-frag-kn5-C256'] = (5, True, 256, 64, 4, False, True, ('bf16',))
PARAMS = [pytest.param(f, d, id='%s-%s' % (f, d)) for f, v in FORMS.items() for d in v[7]]


@gpu
@pytest.mark.parametrize('form,dtype', PARAMS)
def test_llm_attention_form_against_float64(form, dtype):
    """Every launch form at every position set of the module docstring: `out` element by element inside its bound, then — forms with key splits — the same launch with
    skip_combine: `out` untouched, every live partial inside its bounds, bit-identical partials in both launches; the sentinel in all that must stay unwritten."""
    kn, frag, C, c, n_sub, merge, ofrag, _ = FORMS[form]
    dt = DT[dtype]
    for i, (pos0, kv_len, n_valid) in enumerate(_position_sets(kn, C or 256, c or 64)):
        case = Case(dt, kn, pos0, kv_len, n_valid, C, merge, seed=100 * kn + i)
        what = '%s %s pos0=%s kv_len=%s n_valid=%s' % (form, dtype, pos0, kv_len, n_valid)
        out, po, pm = _launch(case, frag=frag, c=c, n_sub=n_sub, ofrag=ofrag)
        _check_out(form, what, out, case)
        if case.S > 1:
            out2, po2, pm2 = _launch(case, frag=frag, c=c, n_sub=n_sub, ofrag=ofrag, skip=True)
            assert bool((out2 == SENT).all()), what + ': skip_combine wrote `out`'
            _check_partials(form, what + ' partial', po2, pm2, case)
            assert torch.equal(po, po2) and torch.equal(pm, pm2), what + ': the partials differ between the two launches'
    print('%s %s: worst error / bound over all launches %.3f' % (form, dtype, WORST['%s %s' % (form, dtype)]))


@gpu
def test_llm_attention_refuses_what_it_cannot_launch():
    kn = 2
    pos0, kv_len, n_valid = _position_sets(kn, 256, 64)[0]
    case = Case(F32, kn, pos0, kv_len, n_valid, 0, False)
    with pytest.raises(_lib.HvxError, match='fragment-order output is 16-bit only'):
        _launch(case, frag=True, ofrag=True)
    with pytest.raises(_lib.HvxError, match='fragment-order caches serve the causal LLM calls only'):
        _launch(case, frag=True, causal=False)
    with pytest.raises(_lib.HvxError, match='fragment-order caches serve the causal LLM calls only'):
        _launch(case, frag=True, chunk=16)
    q, k = case.q.cuda(), case.kc.cuda()
    out = torch.full((kn * 3 * Q,), SENT, device='cuda')
    kw = dict(batch=3, heads=KVH, n_rows=G * kn, kn=kn, q_strides=(kn * Q, G * 64, 64, Q), k_strides=(KVH * CTX * 64, CTX * 64), v_strides=(KVH * CTX * 64, 64 * CTX),
              v_ld=CTX, o_strides=(kn * Q, G * 64, 64, Q), kv_len_const=8)
    for bad in ((None, k, k, out), (q, None, k, out), (q, k, None, out), (q, k, k, None)):
        with pytest.raises(_lib.HvxError, match='null'):
            ops.llm_attention(*bad, **kw)
    with pytest.raises(_lib.HvxError, match='null out'):                     # skip_combine alone does not excuse a null `out`: one split stores there
        ops.llm_attention(q, k, k, None, skip_combine=True, n_splits=1, **kw)
    h = lambda t: t.to(torch.float16)
    with pytest.raises(_lib.HvxError, match='fp32 .0. or bf16 .1. only'):
        ops.llm_attention(h(q), h(k), h(k), h(out), **kw)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


# ================================================================================================================================================
# the narrow residual projection that combines the partials itself (csrc/gemm_skinny.hip: gemm_narrow_resid_kernel<COMB>, combined_pair)
# ================================================================================================================================================
H = 896


@gpu
@pytest.mark.parametrize('dtype', BOTH)
@pytest.mark.parametrize('kn,slots,ends,n_new', [(1, (2,), [200], [1]), (1, (3,), [1000], [1]), (1, SLOTS, [300, 1000, 600], [1, 0, 1]),
                                                 (2, (0,), [513], [1]), (2, SLOTS, [300, 1024, 600], [2, 0, 1]), (2, SLOTS, [257, 40, 800], [1, 2, 2])])
def test_combining_o_proj_is_the_combine_launch_and_the_plain_o_proj_bit_for_bit(kn, slots, ends, n_new, dtype):
    """attention with skip_combine -> decode_gemm(w_narrow, att_o) against attention + attn_combine_kernel -> decode_gemm(w_narrow) on a second copy of the stream:
    the fp32 streams and the 16-bit copies bit-identical (the claim above combined_pair), and each inside the float64 bound of attention followed by projection.
    1 and 3 sequences, ragged n_new (0: the whole sequence inactive), 1 to 4 live 256-key splits."""
    dt, C, n_seq = DT[dtype], 256, len(slots)
    pos0 = [e - kn for e in ends]
    case = Case(dt, kn, pos0, ends, n_new, C, True, slots=slots, seed=7 * kn + n_seq)
    M = n_seq * kn
    g = torch.Generator().manual_seed(40 + M)
    W = (torch.randn(H, Q, generator=g) * Q ** -0.5).to(dt)
    bias, x0 = torch.randn(H, generator=g) * 0.5, torch.randn(M, H, generator=g) * 2.0
    a, B = case.ref, case.bound                                              # rows that are not valid: 0 in both (the combining form builds zeros, the plain one reads them)
    wd = W.double()
    ref = x0.double() + (a @ wd.t() + bias.double())
    e = B @ wd.abs().t() + Q * U * ((a.abs() + B) @ wd.abs().t()) + 2 * U * ref.abs()
    Wn, bd = packing.pack_narrow4(W).cuda(), bias.cuda()
    ctl = case.controls()
    ldo, ldo2 = H + 4, H + 8
    streams = []
    for fused in (True, False):
        attn = torch.zeros(M * Q, dtype=dt, device='cuda')
        _, po, pm = _launch(case, frag=True, c=64, skip=fused, out=attn)
        x = torch.full((M + 2, ldo), SENT, dtype=F32, device='cuda')
        x[:M, :H] = x0.cuda()
        x2 = torch.full((M + 2, ldo2), SENT, dtype=dt, device='cuda')
        if fused:
            assert bool((attn == 0).all())
            ops.decode_gemm(0, SK_RESID, M, H, Q, None, Wn, lda=Q, bias=bd, out=x, ldo=ldo, out2=x2, ldo2=ldo2, w_narrow=True, att_o=po, att_ml=pm, att_kvlen=ctl['kv_len'],
                            att_splits=case.S, att_chunk=C, att_rows_pad=case.npad, kn=kn, q_heads=QH, kv_heads=KVH, pos0=ctl['pos0'], n_new=ctl['n_valid_lo'])
        else:
            ops.decode_gemm(0, SK_RESID, M, H, Q, attn, Wn, lda=Q, bias=bd, out=x, ldo=ldo, out2=x2, ldo2=ldo2, w_narrow=True)
        torch.cuda.synchronize()
        streams.append((x.cpu(), x2.cpu()))
        tag = 'o_proj %s kn=%d ends=%s n_new=%s %s ' % (dtype, kn, ends, n_new, 'combining' if fused else 'plain')
        for name, got, ld, bnd in (('stream', x, ldo, e), ('copy', x2, ldo2, UB * ref.abs() + (1 + UB) * e if dt == BF else e)):
            got = got.double().cpu()
            assert bool((got[M:] == SENT).all()) and bool((got[:, H:] == SENT).all()), tag + name + ': written outside the result'
            _ratio('o_proj-' + ('combining' if fused else 'plain'), tag + name, (got[:M, :H] - ref).abs(), bnd)
    assert torch.equal(streams[0][0], streams[1][0]), 'the fp32 streams differ in %d elements' % int((streams[0][0] != streams[1][0]).sum())
    assert torch.equal(streams[0][1], streams[1][1]), 'the copies differ in %d elements' % int((streams[0][1] != streams[1][1]).sum())


@gpu
def test_combining_o_proj_refuses_more_than_1024_columns():
    f = lambda n, t=F32: torch.full((n,), SENT, dtype=t, device='cuda')
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device='cuda')
    x = f(H)
    with pytest.raises(_lib.HvxError, match='K = q_heads . 64 <= 1024'):
        ops.decode_gemm(0, SK_RESID, 1, H, 18 * 64, None, f(H * 18 * 64, BF), lda=18 * 64, out=x, ldo=H, w_narrow=True, att_o=f(2 * 4 * 32 * 64), att_ml=f(2 * 4 * 32 * 2),
                        att_kvlen=i32([5]), att_splits=4, att_chunk=256, att_rows_pad=32, kn=1, q_heads=18, kv_heads=2, pos0=i32([4]), n_new=i32([1]))
    with pytest.raises(_lib.HvxError, match='belong to form 0'):
        ops.decode_gemm(1, SK_RESID, 64, H, Q, f(64 * Q, BF), f(H * Q, BF), lda=Q, out=f(64 * H), ldo=H, w_narrow=True)
    torch.cuda.synchronize()
    assert bool((x == SENT).all())


# ================================================================================================================================================
# the bounds hold for an fp32 emulation of the kernel's arithmetic (no device)
# ================================================================================================================================================
def _emu_walk(q, K, V, lim, lo, hi, bf):
    """attn_fwd_kernel's loop in fp32: 32-key steps, online maximum, P rounded to bf16 for the PV product only -> (m, l, o)"""
    R = q.shape[0]
    m, l, o = torch.full((R,), -math.inf), torch.zeros(R), torch.zeros(R, 64)
    hi = min(hi, K.shape[0], int(lim.max()))
    for k0 in range(lo, hi, 32):
        k1 = min(k0 + 32, K.shape[0])
        s = (q @ K[k0:k1].t()) * SCALE
        vis = (torch.arange(k0, k1)[None, :] < lim[:, None]) & (torch.arange(k0, k1)[None, :] < hi)
        s = torch.where(vis, s, torch.full_like(s, -math.inf))
        m_new = torch.maximum(m, s.amax(1))
        m_safe = torch.where(m_new == -math.inf, torch.zeros_like(m_new), m_new)
        alpha = torch.where(m == -math.inf, torch.zeros_like(m), (m - m_safe).exp())
        p = torch.where(vis, (s - m_safe[:, None]).exp(), torch.zeros_like(s))
        l = l * alpha + p.sum(1)
        o = o * alpha[:, None] + (p.to(BF).float() if bf else p) @ V[k0:k1]
        m = m_new
    return m, l, o


def _emu_merge(states):
    """the LDS merge of the waves / the combine of the splits: fixed order, weights expf(m_w - m)"""
    m = functools.reduce(torch.maximum, [s[0] for s in states])
    l, o = torch.zeros_like(states[0][1]), torch.zeros_like(states[0][2])
    for mw, lw, ow in states:
        wgt = torch.where(mw == -math.inf, torch.zeros_like(mw), (mw - m).exp())
        o = o + wgt[:, None] * ow
        l = l + wgt * lw
    return m, l, o


@pytest.mark.parametrize('dtype', BOTH)
@pytest.mark.parametrize('kn,C,c,n_sub', [(2, 256, 64, 4), (1, 512, 64, 8), (4, 512, 128, 4), (12, 0, 0, 1)])
def test_fp32_emulation_stays_inside_the_bounds(kn, C, c, n_sub, dtype):
    dt = DT[dtype]
    bf = dt == BF
    for i, (pos0, kv_len, n_valid) in enumerate(_position_sets(kn, C or 256, c or 64)):
        case = Case(dt, kn, pos0, kv_len, n_valid, C, True, seed=100 * kn + i)
        out = torch.full((case.n_seq * kn, Q), SENT, dtype=torch.float64)
        po, pm = torch.full(case.p_ref.shape, SENT, dtype=torch.float64), torch.full(case.p_ref.shape[:-1] + (2,), SENT, dtype=torch.float64)
        r = torch.arange(case.n_rows)
        rh, rl = r // kn, r % kn
        for b, slot in enumerate(SLOTS):
            lim = torch.minimum(torch.tensor(kv_len[b]), pos0[b] + rl + 1)
            ok = rl < n_valid[b]
            for h in range(KVH):
                q, K, V = case.q[b, rl, h * G + rh].float(), case.kc[slot, h, :kv_len[b]].float(), case.vc[slot, h, :kv_len[b]].float()
                if C:
                    parts = []
                    for s in range(case.S):
                        if s * C >= min(kv_len[b], pos0[b] + kn):
                            continue
                        st = _emu_merge([_emu_walk(q, K, V, lim, s * C + w * c, min((s + 1) * C, s * C + (w + 1) * c), bf) for w in range(n_sub)])
                        parts.append(st)
                        po[b, h, s, :case.n_rows][ok], pm[b, h, s, :case.n_rows, 0][ok], pm[b, h, s, :case.n_rows, 1][ok] = st[2][ok].double(), st[0][ok].double(), st[1][ok].double()
                    live = torch.minimum(torch.tensor(len(parts)), (lim + C - 1) // C)            # attn_combine_kernel: n_live per row
                    m, l, o = _emu_merge([(torch.where(live > s, st[0], torch.full_like(st[0], -math.inf)), st[1], st[2]) for s, st in enumerate(parts)])
                    res = o / l[:, None]
                else:
                    m, l, o = _emu_walk(q, K, V, lim, 0, CTX, bf)
                    res = o * (1.0 / l)[:, None]
                rows, cols = (b * kn + rl)[ok], ((h * G + rh)[ok, None] * 64 + torch.arange(64)[None, :])
                out[rows[:, None], cols] = res.to(dt).double()[ok]
        what = 'emulation kn=%d C=%d c=%d waves=%d %s set %d' % (kn, C, c, n_sub, dtype, i)
        _check_out('emulation', what, out, case)
        if C:
            _check_partials('emulation', what + ' partial', po, pm, case)
