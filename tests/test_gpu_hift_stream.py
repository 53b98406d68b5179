"""The streaming vocoder on the device: the pieces of `HiftStream` against the pieces of the whole-cache path (`HvxHift.inference` over the cache, cut at
the samples already handed out) on the same handle, stage by stage against the CPU oracle, and the context check (a longer context changes nothing,
context 0 does).

Bounds: F0 2e-3 Hz and source 2e-4 (test_hift_stages_vs_reference), decode 1e-3 relative to the oracle on the oracle's source (the same test), end to end
2e-2 absolute (the F0 -> phase amplification).  Every figure is printed before it is asserted (pytest -s shows them)."""
import numpy as np
import pytest
import torch

from conftest import load_golden, state_checksum

pytestmark = pytest.mark.gpu
DEV = 'cuda'
FILLS = [(12, False), (37, False), (38, False), (90, False), (160, True)]
T = 160


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)


@pytest.fixture(scope='module')
def setup(tiny_cfg):
    """one handle, one random mel of 160 frames and, computed once, the oracle at every fill: (f0, source, wav) of hift_ref.hift_inference"""
    from flowmirror_hydravox_amd import weights as W
    from flowmirror_hydravox_amd.hift import HvxHift
    from oracle import hift_ref
    g = load_golden('hift_tiny.npz')
    c = tiny_cfg.hift
    sd = W.make_hift_state(c, seed=int(g['weight_seed']), init='fan_in')
    assert state_checksum(sd) == str(g['weight_sha'])
    tables = hift_ref.make_tables(c, seed=int(g['table_seed']))
    hift = HvxHift(c, sd, tables=tables)
    mel = torch.randn(1, 80, T, generator=torch.Generator().manual_seed(21))
    oracle = {}
    for fill, final in FILLS:
        taps = {}
        wav, s = hift_ref.hift_inference(mel[:, :, :fill], sd, c, tables, taps, finalize=final)
        oracle[(fill, final)] = dict(f0=taps['f0'][0], source=s.reshape(-1), wav=wav[0])
    cache = torch.full((80, T + 7), float('nan'), device=DEV)                 # a cache plane wider than the utterance: the row stride is not the fill
    cache[:, :T] = mel[0].to(DEV)
    return dict(hift=hift, mel=mel, cache=cache, oracle=oracle, cfg=c, sd=sd, tables=tables)


def _whole_pieces(hift, mel, fills):
    """today's path: inference over the cache so far, cut at the samples already handed out"""
    out, handed = [], 0
    for fill, final in fills:
        wav, _ = hift.inference(speech_feat=mel[:, :, :fill].to(DEV), finalize=final)
        out.append(wav[0, handed:].clone())
        handed = wav.shape[1]
    return out


def _stream_pieces(st, cache, fills):
    return [st.piece(cache, fill, final)[0].clone() for fill, final in fills]


def test_context_and_lengths_on_the_device(tiny_cfg, setup):
    from flowmirror_hydravox_amd.hift import hift_left_context
    import ctypes as C
    hift = setup['hift']
    a, b = C.c_int32(), C.c_int32()
    assert hift.lib.hvx_hift_left_context(hift._h, C.byref(a), C.byref(b)) == 0
    assert (a.value, b.value) == hift_left_context(tiny_cfg.hift) == (8, 29)


def test_pieces_equal_the_whole_cache_path(setup):
    """lengths exactly, samples within the end-to-end bound; the first piece (a window that starts at frame 0) bit for bit; frames_vocoded"""
    from flowmirror_hydravox_amd.hift import hift_left_context
    hift, c = setup['hift'], setup['cfg']
    whole = _whole_pieces(hift, setup['mel'], FILLS)
    st = hift.stream(T)
    got = _stream_pieces(st, setup['cache'], FILLS)
    torch.cuda.synchronize()
    assert [p.numel() for p in got] == [p.numel() for p in whole] == [480 * n for n in (4, 25, 1, 52, 78)]
    assert [p.numel() for p in got] == [hift.piece_samples(a, f, fin) for a, (f, fin) in zip([0] + [f for f, _ in FILLS], FILLS)]
    assert torch.equal(got[0], whole[0])                                          # the launches of today's pass
    err = [float((a - b).abs().max()) for a, b in zip(got, whole)]
    print('pieces vs whole-cache pieces, max abs per piece:', err)
    assert max(err) < 2e-2, err
    assert torch.isfinite(torch.cat(got)).all()
    # frames through the decode: the new frames once, plus per piece the left context and the frames a non-final pass holds back behind conv_pre
    # (conv_pre_look_right and the one dropped frame); the whole-cache path decodes every fill again
    decode_frames = hift_left_context(c)[1]
    n = st.frames_vocoded
    print('frames_vocoded', n, 'whole-cache', sum(f for f, _ in FILLS))
    assert T <= n <= T + len(FILLS) * (decode_frames + c.conv_pre_look_right + 1)
    assert n < sum(f for f, _ in FILLS) == 337
    # the state's F0 (assembled from the windows) and the whole-cache F0, each against the oracle
    f0_o = setup['oracle'][(T, True)]['f0']
    e_state = float((st.f0.cpu() - f0_o).abs().max())
    e_whole = float((hift.f0(setup['mel'][0]).cpu() - f0_o).abs().max())
    print('F0 [Hz] vs oracle: state %.3e, whole-cache %.3e' % (e_state, e_whole))
    assert st.f0.numel() == T and e_state < 2e-3 and e_whole < 2e-3
    for fill, final in FILLS[:-1]:
        f0 = hift.f0(setup['mel'][0, :, :fill])[:fill - 3].cpu()
        assert float((f0 - setup['oracle'][(fill, final)]['f0']).abs().max()) < 2e-3, fill
    st.close()
    assert hift.live_streams == 0


def test_refusals_and_reset_on_the_device(setup):
    from flowmirror_hydravox_amd._lib import HvxError
    hift, cache = setup['hift'], setup['cache']
    st = hift.stream(T)
    first = st.piece(cache, 37, False).clone()
    with pytest.raises(HvxError, match='smaller than the previous'):
        st.piece(cache, 36, False)
    assert st.piece(cache, 37, False).numel() == 0                                # no new frame: nothing is launched, nothing comes back
    st.piece(cache, 90, True)
    with pytest.raises(HvxError, match='reset the stream'):
        st.piece(cache, 90, True)
    with pytest.raises(HvxError, match='reset the stream'):
        st.piece(cache, 160, False)
    before = st.frames_vocoded
    st.reset()
    assert torch.equal(st.piece(cache, 37, False), first)                         # a new utterance in the same memory
    assert st.frames_vocoded == before + 34                                       # the counter runs over the object's calls
    st.close()


def test_short_utterance_and_a_final_call_without_a_new_frame(setup):
    """T = 9, shorter than the context: the one non-final call that is allowed (9 frames: one frame out), then the final call on the same 9 frames; and
    one final call alone"""
    hift, mel, cache = setup['hift'], setup['mel'], setup['cache']
    fills = [(9, False), (9, True)]
    whole = _whole_pieces(hift, mel, fills)
    st = hift.stream(16)
    got = _stream_pieces(st, cache, fills)
    assert [p.numel() for p in got] == [p.numel() for p in whole] == [480, 8 * 480]
    assert torch.equal(got[0], whole[0]) and torch.equal(got[1], whole[1])       # both windows start at frame 0: today's launches
    st.reset()
    alone = st.piece(cache, 9, True)[0]
    ref, _ = hift.inference(speech_feat=mel[:, :, :9].to(DEV), finalize=True)
    assert torch.equal(alone, ref[0])
    st.close()
    # the same at the end of the long utterance: the final call adds no frame to the cache
    fills = [(f, False) for f, _ in FILLS] + [(T, True)]
    whole = _whole_pieces(hift, mel, fills)
    st = hift.stream(T)
    got = _stream_pieces(st, cache, fills)
    assert [p.numel() for p in got] == [p.numel() for p in whole] and got[-1].numel() == 8 * 480
    err = [float((a - b).abs().max()) for a, b in zip(got, whole)]
    print('final call without a new frame, max abs per piece:', err)
    assert max(err) < 2e-2, err
    st.close()


def test_source_on_the_same_f0(setup):
    """both source stages on the oracle's F0: the stream's (phase scan continued from the carried sums, absolute table index) against hvx_hift_source over
    the frames so far.  Samples that are not bit-equal are counted: the two scans add the same doubles in another association, which moves a sum by
    <= 1e-16 relative before it is rounded to fp32 — a flip needs a sum within that of a rounding boundary (2^-24 relative apart), odds of a few 1e-9 per
    frame and harmonic, so the count over these 160 x 9 phase rows is expected to be 0."""
    hift, cache = setup['hift'], setup['cache']
    f0 = setup['oracle'][(T, True)]['f0']
    st = hift.stream(T)
    st.set_inputs(f0=f0)
    worst, unequal, total = 0.0, 0, 0
    for fill, final in FILLS:
        st.piece(cache, fill, final)
        start, got = st.last_source()
        n = fill if final else fill - 3
        ref = hift.source(f0[:n])[start:]
        assert got.numel() == ref.numel() > 0
        worst = max(worst, float((got - ref).abs().max()))
        unequal += int((got.view(torch.int32) != ref.view(torch.int32)).sum())
        total += got.numel()
    print('source: max abs %.3e, samples not bit-equal %d of %d' % (worst, unequal, total))
    assert worst < 2e-4
    assert unequal == 0
    # ... and the source the oracle computes from that F0
    start, got = st.last_source()
    assert float((got.cpu() - setup['oracle'][(T, True)]['source'][start:]).abs().max()) < 2e-4
    st.close()
    # Up to 256 frames hift_phase_kernel gives every thread one frame and both scans are the same sequential sum, so the 0 above holds by construction.
    # 300 frames: the whole-cache scan runs in 256 partial sums of 2 frames, the continued one per piece — the re-association described above.  The count is
    # recorded; the bound is the source bound.
    gen = torch.Generator().manual_seed(22)
    f0 = torch.rand(300, generator=gen) * 400.0
    long_cache = torch.randn(80, 300, generator=gen).to(DEV)
    st = hift.stream(300)
    st.set_inputs(f0=f0)
    worst, unequal, total = 0.0, 0, 0
    for fill, final in ((200, False), (290, False), (300, True)):
        st.piece(long_cache, fill, final)
        start, got = st.last_source()
        ref = hift.source(f0[:fill if final else fill - 3])[start:]
        worst = max(worst, float((got - ref).abs().max()))
        unequal += int((got.view(torch.int32) != ref.view(torch.int32)).sum())
        total += got.numel()
    print('source over 300 frames: max abs %.3e, samples not bit-equal %d of %d' % (worst, unequal, total))
    assert worst < 2e-4
    st.close()


def _decode_pieces(setup, context=None, source_of=None):
    """the windowed path's pieces with the oracle's F0 and source in place of the two stages (source_of: which oracle pass's source a fill uses)"""
    hift = setup['hift']
    st = hift.stream(T, context=context)
    out = []
    for fill, final in FILLS:
        o = setup['oracle'][source_of(fill, final)]
        s = torch.zeros(T * 480)
        s[:o['source'].numel()] = o['source']
        st.set_inputs(f0=setup['oracle'][(T, True)]['f0'], source=s)
        out.append(st.piece(setup['cache'], fill, final)[0].clone())
    st.close()
    return out


def test_decode_on_the_oracles_source(setup):
    """both paths decode the oracle's source of the same pass; distances are max abs over the utterance's pieces, relative to the oracle's peak"""
    hift, mel = setup['hift'], setup['mel']
    win = torch.cat(_decode_pieces(setup, source_of=lambda fill, final: (fill, final))).cpu()
    whole, ref, handed = [], [], 0
    for fill, final in FILLS:
        o = setup['oracle'][(fill, final)]
        n = fill if final else fill - 3
        wav = hift.decode(mel[0, :, :n], o['source']) if final else hift.decode_chunk(mel[0, :, :n], o['source'])
        assert wav.numel() == o['wav'].numel()
        whole.append(wav[handed:].cpu())
        ref.append(o['wav'][handed:])
        handed = wav.numel()
    whole, ref = torch.cat(whole), torch.cat(ref)
    assert win.shape == whole.shape == ref.shape == (T * 480,)
    d_win, d_whole, d_paths = _rel(win, ref), _rel(whole, ref), _rel(win, whole) * float(whole.abs().max()) / float(ref.abs().max())
    print('decode vs oracle: windowed %.3e, whole-cache %.3e, ratio %.3f; windowed vs whole-cache %.3e' % (d_win, d_whole, d_win / d_whole, d_paths))
    assert d_win < 1e-3 and d_whole < 1e-3
    assert d_win <= 1.25 * d_whole
    assert d_paths < d_whole


def test_a_longer_context_changes_nothing_and_none_does(tiny_cfg, setup):
    """the decode on fixed inputs (the oracle's F0 and final source), with the derived context, with 8 frames more and with none: the comparison can see a
    context that is too short"""
    from flowmirror_hydravox_amd.hift import hift_left_context
    f0_frames, decode_frames = hift_left_context(tiny_cfg.hift)
    final_source = lambda fill, final: (T, True)
    base = torch.cat(_decode_pieces(setup, source_of=final_source)).cpu()
    more = torch.cat(_decode_pieces(setup, context=(f0_frames + 8, decode_frames + 8), source_of=final_source)).cpu()
    none = torch.cat(_decode_pieces(setup, context=(0, 0), source_of=final_source)).cpu()
    d_more, d_none = _rel(more, base), _rel(none, base)
    print('context + 8 vs derived %.3e; context 0 vs derived %.3e' % (d_more, d_none))
    assert d_more < 1e-3
    assert d_none > 1e-3                                                          # outside the bound the other two agree within
    # and end to end (own F0, own source): the F0 windows of a longer context give the same F0 to the predictor's accuracy
    hift = setup['hift']
    a, b = hift.stream(T), hift.stream(T, context=(f0_frames + 8, decode_frames + 8))
    pa, pb = torch.cat(_stream_pieces(a, setup['cache'], FILLS)), torch.cat(_stream_pieces(b, setup['cache'], FILLS))
    assert float((a.f0 - b.f0).abs().max()) < 2e-3 and float((pa - pb).abs().max()) < 2e-2
    z = hift.stream(T, context=(0, decode_frames))
    _stream_pieces(z, setup['cache'], FILLS)
    print('F0 with no F0 context vs derived [Hz]: %.3e' % float((a.f0 - z.f0).abs().max()))
    assert float((a.f0 - z.f0).abs().max()) > 2e-3
    for s in (a, b, z):
        s.close()
