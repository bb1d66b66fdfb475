"""Direct GPU checks of the kernels of csrc/mel_loss.hip against the float64 model tests/_mel_loss_ref.py, one entry point
at a time.  Geometry 64 / 16 / 64 with B = 3, S = 1000 (F = 63: two frame tiles of 32, the second partial), 70 mels (two
channel tiles of 64, ldn = 72 with two pad columns), cutoff = 33 (ldm = 36: three pad columns; lds = 68: two), lens
[1000, 333, 33]: a multiple of nothing, and h + 1 where a sample has both mirrors.

NaN stands wherever a kernel must not read: samples past lens[b], rows past an item's frames, columns past cutoff and
n_mel, target frames past n[b].  Every buffer lies between canaries that are checked after every launch.

Bars (u = 2^-24, the unit roundoff of fp32; every bar is per element, against the model run in float64 on the same fp32
inputs) are derived from the fp32 operations a kernel performs, in the test that uses them."""
import numpy as np
import pytest
import torch

import _mel_loss_ref as K

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24
CANARY = 12345.0
GUARD = 64


class Buf:
    """a device buffer between two canary zones"""

    def __init__(self, data=None, shape=None, dtype=torch.float32, fill=float("nan")):
        if data is not None:
            data = np.ascontiguousarray(data)
            shape, dtype = data.shape, torch.from_numpy(data).dtype
        n = int(np.prod(shape))
        self.whole = torch.full((n + 2 * GUARD,), CANARY if dtype.is_floating_point else 12345, device=DEV, dtype=dtype)
        self.t = self.whole[GUARD:GUARD + n].view(*shape)
        if data is not None:
            self.t.copy_(torch.from_numpy(data))
        elif dtype.is_floating_point:
            self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        w = self.whole.cpu()
        return bool((w[:GUARD] == 12345).all() and (w[-GUARD:] == 12345).all())

    def np(self):
        return self.t.cpu().numpy()


def _call(fn, *args):
    from rad_mmm_amd._lib import check, ptr, stream
    check(fn(*[ptr(a.t) if isinstance(a, Buf) else a for a in args], stream()), fn.__name__)
    torch.cuda.synchronize()
    for a in args:
        assert not isinstance(a, Buf) or a.intact(), "a canary was overwritten"


@pytest.fixture(scope="module")
def L():
    from rad_mmm_amd._lib import lib
    return lib


G = K.Geometry(64, 16, 64, 70, 3, 1000)
LENS = np.array([1000, 333, 33])
NFX = 1 + LENS // 16                                              # 63, 21, 3
FT = G.F - 3
FRAMES = np.array([70, 20, 2])                                    # read clamped into [0, min(F, Ft)] = [0, 60]
NL = np.minimum(np.minimum(NFX, FT), np.clip(FRAMES, 0, FT))      # 60, 20, 2
assert list(K.loss_frames(LENS, FRAMES, G, FT)) == list(NL)


def _lens(v=LENS):
    return Buf(np.asarray(v, dtype=np.int32))


def _rows_mask(nf):
    return K.valid_rows(nf, G)


def _assert_within(got, want, bar, what):
    """|got - want| <= bar per element; prints the worst measured / bar"""
    got, want, bar = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(bar, dtype=np.float64)
    assert np.isfinite(got).all(), what
    err = np.abs(got - want)
    ratio = np.where(bar > 0, err / np.where(bar > 0, bar, 1), np.where(err > 0, np.inf, 0.0))
    print(f"{what}: worst measured / bar {ratio.max():.3f}")
    assert ratio.max() <= 1.0, (what, float(ratio.max()))


def test_frame_is_bit_equal_to_the_model(L):
    rng = np.random.RandomState(0)
    x = rng.randn(G.B, G.S + 8).astype(np.float32)                 # ldx > S
    for b, n in enumerate(LENS):
        x[b, n:] = np.nan
    xb, A, lens = Buf(x), Buf(shape=(G.rows, G.n_fft)), _lens()
    _call(L.radmmm_melloss_frame, xb, G.S + 8, lens, A, G.B, G.S, G.F, G.n_fft, G.hop)
    want = K.frame(np.nan_to_num(x[:, :G.S]), LENS, G)
    assert np.array_equal(A.np(), want)
    assert not A.np()[~_rows_mask(NFX)].any()
    full = np.nan_to_num(x)
    A2 = Buf(shape=(G.rows, G.n_fft))
    _call(L.radmmm_melloss_frame, Buf(full), G.S + 8, None, A2, G.B, G.S, G.F, G.n_fft, G.hop)
    assert np.array_equal(A2.np(), K.frame(full[:, :G.S], None, G))


def test_unframe_is_exact_on_integers_with_both_mirrors_and_accum(L):
    rng = np.random.RandomState(1)
    dA = rng.randint(-8, 9, size=(G.rows, G.n_fft)).astype(np.float32)
    dA[~_rows_mask(NFX)] = np.nan
    want = K.unframe(np.nan_to_num(dA), LENS, G)
    assert np.array_equal(want, K.unframe_fast(np.nan_to_num(dA), LENS, G))
    ldd = G.S + 4
    dAb, lens, dx = Buf(dA), _lens(), Buf(shape=(G.B, ldd))
    _call(L.radmmm_melloss_unframe, dAb, lens, dx, ldd, G.B, G.S, G.F, G.n_fft, G.hop, 0)
    got = dx.np()
    assert np.array_equal(got[:, :G.S], want) and np.isnan(got[:, G.S:]).all()
    for b, n in enumerate(LENS):
        assert not got[b, n:G.S].any()
    assert LENS[2] == G.h + 1 and want[2, 1:LENS[2] - 1].any()
    pre = rng.randint(-8, 9, size=(G.B, ldd)).astype(np.float32)
    acc = Buf(pre)
    _call(L.radmmm_melloss_unframe, dAb, lens, acc, ldd, G.B, G.S, G.F, G.n_fft, G.hop, 1)
    exp = pre.copy()
    exp[:, :G.S] += want.astype(np.float32)
    assert np.array_equal(acc.np(), exp)
    again = Buf(shape=(G.B, ldd))
    _call(L.radmmm_melloss_unframe, dAb, lens, again, ldd, G.B, G.S, G.F, G.n_fft, G.hop, 0)
    assert np.array_equal(again.np()[:, :G.S], got[:, :G.S])


def _spec(seed):
    rng = np.random.RandomState(seed)
    spec = rng.randn(G.rows, G.lds).astype(np.float32) * np.exp(rng.uniform(-6, 3, size=(G.rows, 1))).astype(np.float32)
    spec[5, :] = 0                                                 # a silent frame: re = im = 0 in every bin
    spec[7, 3] = spec[7, G.cutoff + 3] = 0                         # one silent bin
    spec[:, 2 * G.cutoff:] = np.nan
    spec[~_rows_mask(NFX)] = np.nan
    return spec


def test_mag(L):
    """p = fl(fl(re^2) + fl(im^2)) carries at most 2u relative (three roundings of positive terms, the sum's on top of the
    larger square's); sqrt halves that and rounds once more: 2u relative in all.  Bar 2.5u |mag|."""
    spec = _spec(2)
    out = Buf(shape=(G.rows, G.ldm))
    _call(L.radmmm_melloss_mag, Buf(spec), G.lds, _lens(), out, G.ldm, G.B, G.S, G.F, G.hop, G.cutoff)
    want = K.mag(np.nan_to_num(spec).astype(np.float64), LENS, G)
    got = out.np()
    _assert_within(got, want, 2.5 * U * np.abs(want), "mag")
    assert not got[:, G.cutoff:].any() and not got[~_rows_mask(NFX)].any() and not got[5].any() and got[7, 3] == 0


def _melp(seed):
    """positive values on both sides of the clip (none in [0.5, 2], where |log| is small against the partials' bar)"""
    rng = np.random.RandomState(seed)
    lo = np.exp(rng.uniform(np.log(1e-7), np.log(0.5), size=(G.rows, G.ldn)))
    hi = np.exp(rng.uniform(np.log(2.0), np.log(20.0), size=(G.rows, G.ldn)))
    melp = np.where(rng.rand(G.rows, G.ldn) < 0.5, lo, hi).astype(np.float32)
    melp[3, 4] = np.float32(K.CLIP)                                # exactly at the clip: passes
    melp[:, G.n_mel:] = np.nan
    melp[~_rows_mask(NFX)] = np.nan
    return melp


def _terms_inputs(L):
    """melp, the GPU's own mel of it, and a target that differs from that mel by at least 1e-3 except where it is made
    equal on purpose (sign(0) = 0)"""
    melp = _melp(3)
    mel_out = Buf(shape=(G.B, G.n_mel, G.F))
    _call(L.radmmm_melloss_terms, Buf(melp), G.ldn, _lens(), None, None, 0, mel_out, None, G.B, G.S, G.F, G.hop, G.n_mel, K.CLIP)
    mel = mel_out.np()
    rng = np.random.RandomState(4)
    delta = rng.uniform(1e-3, 2.0, size=(G.B, G.n_mel, FT)) * rng.choice([-1.0, 1.0], size=(G.B, G.n_mel, FT))
    delta[:, ::7, ::5] = 0
    target = (mel[:, :, :FT] + delta).astype(np.float32)
    for b in range(G.B):
        target[b, :, NL[b]:] = np.nan
    return melp, mel, target


def test_terms_mel_and_partials(L):
    """mel: the kernel takes the log in double and rounds once (fmaxf is exact): half an ulp, at most u |mel|, plus the
    double log's own error, far below; bar 1.01u |mel|.  part: every term |mel - t| carries that and the subtraction's
    u |d|; lane l adds at most two terms and the butterfly six levels, each addition within u of the running sum: at most
    8u sum |d| on top.  Bar per row: sum_c 1.01u |mel_c| + 9u sum_c |d_c|."""
    melp, mel, target = _terms_inputs(L)
    want_rows = K.log_mel(np.nan_to_num(melp).astype(np.float64), LENS, G, K.CLIP32)
    want = K.to_layout(want_rows, G)
    _assert_within(mel, want, 1.01 * U * np.abs(want), "terms mel_out")
    for b in range(G.B):
        assert not mel[b, :, NFX[b]:].any()
    part, mel2 = Buf(shape=(G.rows,)), Buf(shape=(G.B, G.n_mel, G.F))
    _call(L.radmmm_melloss_terms, Buf(melp), G.ldn, _lens(), _lens(FRAMES), Buf(target), FT, mel2, part, G.B, G.S, G.F, G.hop,
          G.n_mel, K.CLIP)
    assert np.array_equal(mel2.np(), mel)
    t_rows = K.from_layout(np.nan_to_num(target).astype(np.float64), G, FT)
    d = np.abs(want_rows - t_rows)
    ok = _rows_mask(NL)
    want_part = np.where(ok, d.sum(1), 0.0)
    bar = np.where(ok, 1.01 * U * np.abs(want_rows).sum(1) + 9 * U * d.sum(1), 0.0)
    _assert_within(part.np(), want_part, bar, "terms part")
    only = Buf(shape=(G.rows,))
    _call(L.radmmm_melloss_terms, Buf(melp), G.ldn, _lens(), _lens(FRAMES), Buf(target), FT, None, only, G.B, G.S, G.F, G.hop,
          G.n_mel, K.CLIP)
    assert np.array_equal(only.np(), part.np())


def test_finish(L):
    """fp64 sums of at most 189 fp32 partials (relative error far below u), one rounding to fp32: bar 1.01u |loss|; the
    normaliser is an exact integer; no frames: loss 0"""
    rng = np.random.RandomState(5)
    part = rng.uniform(0.5, 200.0, size=G.rows).astype(np.float32)
    part[~_rows_mask(NL)] = np.nan
    out, norm = Buf(shape=(1,)), Buf(shape=(1,), dtype=torch.float64)
    _call(L.radmmm_melloss_finish, Buf(part), _lens(), _lens(FRAMES), out, norm, G.B, G.S, G.F, FT, G.hop, G.n_mel)
    want = np.nan_to_num(part).astype(np.float64).sum() / (G.n_mel * NL.sum())
    _assert_within(out.np(), [want], [1.01 * U * want], "finish loss")
    assert float(norm.np()[0]) == float(NL.sum())
    _call(L.radmmm_melloss_finish, Buf(part), _lens(), _lens([0, -4, 0]), out, norm, G.B, G.S, G.F, FT, G.hop, G.n_mel)
    assert float(out.np()[0]) == 0.0 and float(norm.np()[0]) == 0.0
    _call(L.radmmm_melloss_finish, Buf(np.nan_to_num(part)), None, None, out, norm, G.B, G.S, G.F, FT, G.hop, G.n_mel)
    assert float(norm.np()[0]) == G.B * FT


def test_bwd_fused_and_plain(L):
    """fused: coef = fl(g / (n_mel * sum n)) (fp64, rounded once: u), divided by melp (u): bar 2.1u |value|; the sign is
    exact because every non-zero |mel - target| is at least 1e-3, and 0 where the target equals the mel.  plain:
    fl(dmel / melp): bar 1.01u |value|.  Exact zeros below the clip, in rows past n[b] (or the item's frames) and in the pad
    columns."""
    melp, mel, target = _terms_inputs(L)
    g = np.array([0.7], dtype=np.float32)
    norm = np.array([float(NL.sum())])
    out = Buf(shape=(G.rows, G.ldn))
    _call(L.radmmm_melloss_bwd, Buf(melp), G.ldn, _lens(), _lens(FRAMES), Buf(target), FT, Buf(norm), Buf(g), None, out, G.B, G.S,
          G.F, G.hop, G.n_mel, K.CLIP)
    mp = np.nan_to_num(melp).astype(np.float64)
    mel_rows = K.from_layout(mel.astype(np.float64), G, G.F)
    t_rows = K.from_layout(np.nan_to_num(target).astype(np.float64), G, FT)
    want = K.loss_bwd(mp, mel_rows, t_rows, NL, G, grad=float(g[0]), clip=K.CLIP32)
    got = out.np()
    _assert_within(got, want, 2.1 * U * np.abs(want), "bwd fused")
    assert not got[:, G.n_mel:].any() and not got[~_rows_mask(NL)].any()
    zero_d = (mel_rows == t_rows) & _rows_mask(NL)[:, None]
    assert zero_d.sum() > 50 and not got[:, :G.n_mel][zero_d].any()
    below = (mp[:, :G.n_mel] < K.CLIP32) & _rows_mask(NL)[:, None]
    assert below.sum() > 100 and not got[:, :G.n_mel][below].any() and got[3, 4] != 0
    _call(L.radmmm_melloss_bwd, Buf(melp), G.ldn, _lens(), _lens(FRAMES), Buf(target), FT, Buf(np.zeros(1)), Buf(g), None, out,
          G.B, G.S, G.F, G.hop, G.n_mel, K.CLIP)
    assert not out.np().any()                                      # no frames: gradient 0, not NaN
    dmel = np.random.RandomState(6).randn(G.B, G.n_mel, G.F).astype(np.float32)
    for b in range(G.B):
        dmel[b, :, NFX[b]:] = np.nan
    _call(L.radmmm_melloss_bwd, Buf(melp), G.ldn, _lens(), None, None, 0, None, None, Buf(dmel), out, G.B, G.S, G.F, G.hop,
          G.n_mel, K.CLIP)
    want = K.plain_bwd(mp, np.nan_to_num(dmel), LENS, G, K.CLIP32)
    got = out.np()
    _assert_within(got, want, 1.01 * U * np.abs(want), "bwd plain")
    assert not got[:, G.n_mel:].any() and not got[~_rows_mask(NFX)].any()


def test_dspec(L):
    """mag carries 2u (test_mag), s = fl(dmag / mag) another u, fl(s * re) another: bar 4.5u |value|; exact zeros where
    re = im = 0, in rows past an item's frames and in the pad columns"""
    spec = _spec(7)
    dmag = np.random.RandomState(8).randn(G.rows, G.ldm).astype(np.float32)
    dmag[:, G.cutoff:] = np.nan
    dmag[~_rows_mask(NFX)] = np.nan
    out = Buf(shape=(G.rows, G.lds))
    _call(L.radmmm_melloss_dspec, Buf(dmag), G.ldm, Buf(spec), G.lds, _lens(), out, G.B, G.S, G.F, G.hop, G.cutoff)
    s64, d64 = np.nan_to_num(spec).astype(np.float64), np.nan_to_num(dmag).astype(np.float64)
    re, im = s64[:, :G.cutoff], s64[:, G.cutoff:2 * G.cutoff]
    m = np.sqrt(re * re + im * im)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(m > 0, d64[:, :G.cutoff] / m, 0.0)
    want = np.zeros((G.rows, G.lds))
    want[:, :G.cutoff], want[:, G.cutoff:2 * G.cutoff] = s * re, s * im
    want[~_rows_mask(NFX)] = 0
    got = out.np()
    _assert_within(got, want, 4.5 * U * np.abs(want), "dspec")
    assert not got[:, 2 * G.cutoff:].any() and not got[~_rows_mask(NFX)].any() and not got[5].any()
    assert got[7, 3] == 0 and got[7, G.cutoff + 3] == 0


def test_lens_at_or_below_h_stay_inside_every_buffer(L):
    """lens[b] <= h, 0, negative and above S: every launch returns 0, every output is finite and every canary is intact
    (the kernels clamp lens into [1, S] and every reflected index into the item).  A bounds check: nothing here can read or
    write outside a buffer."""
    rng = np.random.RandomState(9)
    lens_v = np.array([G.h, 0, G.S + 100])
    x = rng.randn(G.B, G.S).astype(np.float32)
    lens = _lens(lens_v)
    A = Buf(shape=(G.rows, G.n_fft))
    _call(L.radmmm_melloss_frame, Buf(x), G.S, lens, A, G.B, G.S, G.F, G.n_fft, G.hop)
    assert np.isfinite(A.np()).all()
    assert np.array_equal(A.np(), K.frame(x, lens_v, G))
    spec = rng.randn(G.rows, G.lds).astype(np.float32)
    mag = Buf(shape=(G.rows, G.ldm))
    _call(L.radmmm_melloss_mag, Buf(spec), G.lds, lens, mag, G.ldm, G.B, G.S, G.F, G.hop, G.cutoff)
    melp = np.abs(rng.randn(G.rows, G.ldn)).astype(np.float32)
    target = rng.randn(G.B, G.n_mel, FT).astype(np.float32)
    mel, part = Buf(shape=(G.B, G.n_mel, G.F)), Buf(shape=(G.rows,))
    for fr in (None, _lens([-1, 2 ** 31 - 1, 1])):
        _call(L.radmmm_melloss_terms, Buf(melp), G.ldn, lens, fr, Buf(target), FT, mel, part, G.B, G.S, G.F, G.hop, G.n_mel, K.CLIP)
        out, norm = Buf(shape=(1,)), Buf(shape=(1,), dtype=torch.float64)
        _call(L.radmmm_melloss_finish, part, lens, fr, out, norm, G.B, G.S, G.F, FT, G.hop, G.n_mel)
        dmelp = Buf(shape=(G.rows, G.ldn))
        _call(L.radmmm_melloss_bwd, Buf(melp), G.ldn, lens, fr, Buf(target), FT, norm, Buf(np.ones(1, dtype=np.float32)), None,
              dmelp, G.B, G.S, G.F, G.hop, G.n_mel, K.CLIP)
        for o in (mel, part, out, norm, dmelp):
            assert np.isfinite(o.np()).all()
    dspec = Buf(shape=(G.rows, G.lds))
    _call(L.radmmm_melloss_dspec, Buf(rng.randn(G.rows, G.ldm).astype(np.float32)), G.ldm, Buf(spec), G.lds, lens, dspec, G.B, G.S,
          G.F, G.hop, G.cutoff)
    dA = rng.randint(-8, 9, size=(G.rows, G.n_fft)).astype(np.float32)
    dx = Buf(shape=(G.B, G.S))
    _call(L.radmmm_melloss_unframe, Buf(dA), lens, dx, G.S, G.B, G.S, G.F, G.n_fft, G.hop, 0)
    for o in (mag, dspec, dx):
        assert np.isfinite(o.np()).all()
