"""The entry points of csrc/mpd.hip (include/radmmm_hip.h, "multi-period discriminator"), each alone against a float64 /
integer model written here from the header's formulas.  Copies (fold_frame, frame, repad) are held bit for bit, the
adjoints (unframe, unfold_audio) are exact on small integers, reductions stay within n * 2^-24 * sum |terms| (n terms
added in fp32 in some order, each rounding at most 2^-24 of the running sum, which sum |terms| bounds), and NaN is planted
wherever a kernel must not read: pad columns, pad rows of an upstream gradient, rows past a count, the other half.

Shapes: every period at T = k p, k p + 1, k p + p - 1, the widest legal reflect n_pad = T - 1 once per odd period
(T = (p + 1) / 2; period 2 never pads more than one sample), H % 3 in {0, 1, 2}, H' = 1, B = 1, widths 4 and 32."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PERIODS = (2, 3, 5, 7, 11)
EPS = 2.0 ** -24


def _lib():
    from rad_mmm_amd._lib import check, lib, ptr, stream
    return check, lib, ptr, stream


_KEEP = []


def _dev(a):
    """device copy, kept alive until the test ends (a temporary would be freed, and its memory reused, before the launch)"""
    t = torch.as_tensor(np.ascontiguousarray(a)).to(DEV)
    _KEEP.append(t)
    return t


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.synchronize()
    del _KEEP[:]


def _cases():
    out = []
    for p in PERIODS:
        ts = {4 * p, 4 * p + 1, 4 * p + p - 1, 7 * p + 1, 9 * p}       # H = 4, 5, 5, 8, 9: H % 3 = 1, 2, 2, 2, 0
        if p % 2:
            ts.add((p + 1) // 2)                                        # n_pad = T - 1, H = 1
        out += [(p, T, B) for T in sorted(ts) for B in ((1, 2) if T == 4 * p + 1 else (2,))]
    return out


def _fold(audio, p):
    """[B, T] -> [B, H, p] with the reflect tail"""
    B, T = audio.shape
    H = -(-T // p)
    t = np.arange(H * p)
    t = np.where(t >= T, 2 * (T - 1) - t, t)
    return audio[:, t].reshape(B, H, p)


def _sequences(y, yh, p):
    """[S, H]: sequence s = (sig * B + b) * p + w"""
    x = np.concatenate([_fold(y, p), _fold(yh, p)])                     # [2B, H, p]
    return x.transpose(0, 2, 1).reshape(-1, x.shape[1])


def _windows(x, st, Ho):
    """x [S, H, C] -> frames [S, Ho, 5, C] of a 5-tap, pad-2 conv of stride st"""
    S, H, C = x.shape
    xp = np.zeros((S, H + 4, C), x.dtype)
    xp[:, 2:2 + H] = x
    return np.stack([xp[:, st * h:st * h + 5] for h in range(Ho)], 1)


@pytest.mark.parametrize("p,T,B", _cases())
def test_fold_frame_is_a_copy_and_unfold_audio_its_adjoint(p, T, B):
    check, lib, ptr, stream = _lib()
    rng = np.random.RandomState(p * 1000 + T)
    H, ldy = -(-T // p), T + 3
    H1 = (H - 1) // 3 + 1
    y = np.full((B, ldy), np.nan, np.float32)
    yh = np.full((B, ldy), np.nan, np.float32)
    y[:, :T], yh[:, :T] = rng.randn(B, T), rng.randn(B, T)
    F = torch.full((2 * B * p * H1, 8), float("nan"), device=DEV)
    check(lib.radmmm_mpd_fold_frame(ptr(_dev(y)), ptr(_dev(yh)), ldy, ptr(F), B, T, p, H, H1, stream()), "fold_frame")
    seq = _sequences(y[:, :T], yh[:, :T], p)
    want = np.zeros((seq.shape[0], H1, 8), np.float32)
    want[:, :, :5] = _windows(seq[:, :, None], 3, H1)[..., 0]
    assert np.array_equal(F.cpu().numpy().reshape(want.shape), want)
    # the adjoint on small integers: <fold_frame(e_t), dF> for every sample t
    dF = rng.randint(-8, 9, size=want.shape).astype(np.float32)
    dF[:, :, 5:] = np.nan                                               # the pad columns are never read
    for sig in range(2):
        g = torch.full((B, ldy), float("nan"), device=DEV)
        check(lib.radmmm_mpd_unfold_audio(ptr(_dev(dF)), ptr(g), ldy, B, T, p, H, H1, sig, stream()), "unfold_audio")
        g = g.cpu().numpy()
        assert np.isnan(g[:, T:]).all()
        wantg = np.zeros((B, T))
        for b in range(B):
            for t in range(T):
                e = np.zeros((B, T), np.float32)
                e[b, t] = 1
                z = np.zeros((B, T), np.float32)
                fr = _windows(_sequences(*((e, z) if sig == 0 else (z, e)), p)[:, :, None], 3, H1)[..., 0]
                wantg[b, t] = (fr * dF[:, :, :5]).sum()
        assert np.array_equal(g[:, :T], wantg.astype(np.float32))


SHAPES = [(6, 4, 4, 3), (6, 5, 4, 3), (6, 9, 32, 3), (2, 1, 4, 3), (2, 2, 32, 3), (6, 4, 4, 1), (3, 1, 32, 1), (22, 7, 8, 3)]


@pytest.mark.parametrize("S,H,C,st", SHAPES)
def test_repad_frame_and_unframe(S, H, C, st):
    from rad_mmm_amd._lib import rowgemm_plan
    check, lib, ptr, stream = _lib()
    rng = np.random.RandomState(S * 100 + H * 10 + C + st)
    Ho = (H - 1) // st + 1
    ldz = C + 4
    Z = np.full((S * H, ldz), np.nan, np.float32)
    Z[:, :C] = rng.randn(S * H, C)
    Z[0, 0] = 0.0                                                       # at the kink: the output is 0, the derivative the slope
    X = torch.full((S, H + 4, C), float("nan"), device=DEV)
    check(lib.radmmm_mpd_repad(ptr(_dev(Z)), ldz, ptr(X), S, H, C, 0.1, stream()), "repad")
    z = Z[:, :C].reshape(S, H, C)
    wantX = np.zeros((S, H + 4, C), np.float32)
    wantX[:, 2:2 + H] = np.where(z > 0, z, np.float32(0.1) * z)
    assert np.array_equal(X.cpu().numpy(), wantX)
    Fr = torch.full((S * Ho, 5 * C), float("nan"), device=DEV)
    check(lib.radmmm_mpd_frame(ptr(X), ptr(Fr), S, H, C, Ho, st, stream()), "frame")
    assert np.array_equal(Fr.cpu().numpy().reshape(S, Ho, 5, C), _windows(wantX[:, 2:2 + H], st, Ho))
    # the framed descriptor of this layer reaches a kernel the plan accepts (host only, before any launch)
    a = 0x10000
    for Cout in (4, 32):
        assert rowgemm_plan(A=a, lda=st * C, a_item_stride=(H + 4) * C, B=a, ldb=5 * C, C=a, ldc=Cout, M=S * Ho, N=Cout,
                            K=5 * C, T=Ho, bias=a) > 0
        assert rowgemm_plan(A=a, lda=Cout, B=a, ldb=5 * C, b_layout=1, C=a, ldc=5 * C, M=S * Ho, N=5 * C, K=Cout, T=Ho) > 0
    # unframe: small integers and slope 0.5 are exact; the pad rows of `add` are never read
    dF = rng.randint(-8, 9, size=(S, Ho, 5, C)).astype(np.float32)
    add = np.full((S, H + 4, C), np.nan, np.float32)
    add[:, 2:2 + H] = rng.randint(-8, 9, size=(S, H, C))
    want = np.zeros((S, H + 4, C))
    for h in range(Ho):
        want[:, st * h:st * h + 5] += dF[:, h]
    for with_add in (True, False):
        dZ = torch.full((S * H, C), float("nan"), device=DEV)
        check(lib.radmmm_mpd_unframe(ptr(_dev(dF)), ptr(_dev(add)) if with_add else None, ptr(X), ptr(dZ), S, H, C, Ho, st, 0.5,
                                     stream()), "unframe")
        w = (want[:, 2:2 + H] + (add[:, 2:2 + H] if with_add else 0)) * np.where(wantX[:, 2:2 + H] > 0, 1.0, 0.5)
        assert np.array_equal(dZ.cpu().numpy().reshape(S, H, C), w.astype(np.float32))


@pytest.mark.parametrize("B2,p,H,C", [(2, 2, 1, 4), (4, 3, 5, 32), (2, 11, 3, 4), (6, 5, 70, 8), (2, 7, 2, 1024)])
def test_conv_post_forward_and_gradients(B2, p, H, C):
    check, lib, ptr, stream = _lib()
    rng = np.random.RandomState(B2 + p + H + C)
    S = B2 * p
    x = rng.randn(S, H, C).astype(np.float32)
    Xp = np.zeros((S, H + 4, C), np.float32)
    Xp[:, 2:2 + H] = x
    Xp[:, 0], Xp[:, H + 3] = np.nan, np.nan                             # only the inner pad row on either side is read
    W, bias = rng.randn(3, C).astype(np.float32), rng.randn(1).astype(np.float32)
    out = torch.full((B2, H, p), float("nan"), device=DEV)
    check(lib.radmmm_mpd_conv_post(ptr(_dev(Xp)), ptr(_dev(W)), ptr(_dev(bias)), ptr(out), B2, p, H, C, stream()), "conv_post")
    x64 = np.zeros((S, H + 2, C))
    x64[:, 1:1 + H] = x
    terms = np.stack([x64[:, k:k + H] * W[k].astype(np.float64) for k in range(3)], -1)      # [S, H, C, 3]
    want = terms.sum((2, 3)) + float(bias[0])                                                  # [S, H]
    bar = (3 * C + 1) * EPS * (np.abs(terms).sum((2, 3)) + abs(float(bias[0])))
    got = out.cpu().numpy().reshape(B2, H, p).transpose(0, 2, 1).reshape(S, H)
    print(f"conv_post: largest error / bar {float((np.abs(got - want) / bar).max()):.3f}")
    assert (np.abs(got - want) <= bar).all()
    # data gradient: exact on small integers with slope 0.5
    dO = rng.randint(-4, 5, size=(B2, H, p)).astype(np.float32)
    Wi = rng.randint(-4, 5, size=(3, C)).astype(np.float32)
    add = np.full((S, H + 4, C), np.nan, np.float32)
    add[:, 2:2 + H] = rng.randint(-4, 5, size=(S, H, C))
    dZ = torch.full((S * H, C), float("nan"), device=DEV)
    check(lib.radmmm_mpd_conv_post_dgrad(ptr(_dev(dO)), ptr(_dev(Wi)), ptr(_dev(add)), ptr(_dev(Xp)), ptr(dZ), B2, p, H, C, 0.5,
                                         stream()), "conv_post_dgrad")
    dos = np.zeros((S, H + 2))
    dos[:, 1:1 + H] = dO.transpose(0, 2, 1).reshape(S, H)
    wantz = sum(dos[:, 2 - k:2 - k + H, None] * Wi[k][None, None, :] for k in range(3)) + add[:, 2:2 + H]
    wantz = wantz * np.where(x > 0, 1.0, 0.5)
    assert np.array_equal(dZ.cpu().numpy().reshape(S, H, C), wantz.astype(np.float32))
    # weight and bias gradient: partial rows + radmmm_colsum_final
    dOr = rng.randn(B2, H, p).astype(np.float32)
    n = int(lib.radmmm_mpd_conv_post_wgrad_parts(B2, p, H))
    part = torch.full((n, 3 * C + 1), float("nan"), device=DEV)
    dw = torch.full((3 * C + 1,), float("nan"), device=DEV)
    check(lib.radmmm_mpd_conv_post_wgrad(ptr(_dev(dOr)), ptr(_dev(Xp)), ptr(part), B2, p, H, C, stream()), "conv_post_wgrad")
    check(lib.radmmm_colsum_final(ptr(part), ptr(dw), n, 3 * C + 1, stream()), "colsum_final")
    d64 = dOr.transpose(0, 2, 1).reshape(S, H).astype(np.float64)
    tw = np.stack([d64[:, :, None] * x64[:, k:k + H] for k in range(3)])                       # [3, S, H, C]
    wantw, barw = tw.sum((1, 2)), (S * H) * EPS * np.abs(tw).sum((1, 2))
    got = dw.cpu().numpy()
    assert (np.abs(got[:3 * C].reshape(3, C) - wantw) <= barw).all()
    assert abs(got[3 * C] - d64.sum()) <= (S * H) * EPS * np.abs(d64).sum()


def _counts(rng, B, sizes, ragged):
    if not ragged:
        return None
    c = np.stack([rng.randint(0, s + 1, size=B) for s in sizes]).astype(np.int32)
    c[:, 0] = sizes                                                     # one full item
    if B > 1:
        c[0, 1], c[6, 1] = -3, sizes[6] + 5                             # read clamped to [0, size]
    return c


@pytest.mark.parametrize("B,p,Hs,Cs,ragged", [(3, 3, (11, 4, 2, 1, 1), (4, 8, 16, 16, 16), True), (1, 2, (5, 2, 1, 1, 1), (32, 4, 4, 8, 4), True),
                                              (2, 11, (3, 1, 1, 1, 1), (4, 4, 4, 4, 32), False), (2, 5, (400, 134, 45, 15, 15), (32, 4, 4, 4, 4), True)])
def test_loss_terms_finish_and_loss_gradients(B, p, Hs, Cs, ragged):
    check, lib, ptr, stream = _lib()
    rng = np.random.RandomState(B * 10 + p)
    Hs, Cs = list(Hs) + [Hs[4]], list(Cs) + [1]
    sizes = Hs + [Hs[4] * p]
    cnt = _counts(rng, B, sizes, ragged)
    eff = np.stack([np.clip(cnt[l], 0, sizes[l]) if ragged else np.full(B, sizes[l]) for l in range(7)])
    cnt_d = _dev(cnt) if ragged else None
    maps, parts, offs = [], [], [0]
    for l in range(6):
        x = rng.randn(2, B, p, Hs[l], Cs[l]).astype(np.float32)
        x[1, :, :, :, 0] = x[0, :, :, :, 0]                             # r == g: sign(0) = 0
        maps.append(x)
        offs.append(offs[-1] + int(lib.radmmm_mpd_fm_terms_parts(B, p, Hs[l], Cs[l])))
    part = torch.full((offs[-1],), float("nan"), device=DEV)
    bufs = []
    for l in range(5):
        buf = np.full((2, B, p, Hs[l] + 4, Cs[l]), np.nan, np.float32)   # the pad rows and the rows past a count are not read
        for b in range(B):
            buf[:, b, :, 2:2 + eff[l, b]] = maps[l][:, b, :, :eff[l, b]]
        bufs.append(_dev(buf))
    out = maps[5][..., 0].transpose(0, 1, 3, 2).copy()                   # [2, B, H, p]
    outn = out.copy()
    for b in range(B):
        outn[:, b, eff[5, b]:] = np.nan if eff[6, b] <= eff[5, b] * p else outn[:, b, eff[5, b]:]
    # (the output's rows past cnt[5] still count for the adversarial terms when cnt[6] reaches them: NaN only where neither reads)
    out_d = _dev(outn)
    for l in range(6):
        src = bufs[l] if l < 5 else out_d
        check(lib.radmmm_mpd_fm_terms(ptr(src), ptr(cnt_d[l]) if ragged else None, ptr(part[offs[l]:]), B, p, Hs[l], Cs[l], int(l < 5),
                                      stream()), "fm_terms")
    res = torch.full((4,), float("nan"), device=DEV)
    norm = torch.full((8,), float("nan"), device=DEV, dtype=torch.float64)
    i32 = ctypes.c_int32
    check(lib.radmmm_mpd_finish(ptr(part), (i32 * 7)(*offs), (i32 * 6)(*Cs), (i32 * 6)(*Hs), ptr(out_d), ptr(cnt_d), ptr(res), ptr(norm),
                                B, p, stream()), "finish")
    fm, fm_bar = 0.0, 0.0
    for l in range(6):
        m = (np.arange(Hs[l])[None, :] < eff[l][:, None])[:, None, :, None]
        d = np.abs(maps[l][0].astype(np.float64) - maps[l][1]) * m
        nl = eff[l].sum() * Cs[l] * p
        assert float(norm[l]) == nl
        fm += d.sum() / nl
        fm_bar += d.size * EPS * d.sum() / nl
    mf = (np.arange(sizes[6])[None, :] < eff[6][:, None])
    dr, dg = out[0].reshape(B, -1).astype(np.float64), out[1].reshape(B, -1).astype(np.float64)
    n6 = eff[6].sum()
    assert float(norm[6]) == n6
    want = np.array([fm, (((1 - dr) ** 2) * mf).sum() / n6, ((dg ** 2) * mf).sum() / n6, (((1 - dg) ** 2) * mf).sum() / n6])
    got = res.cpu().numpy().astype(np.float64)
    bars = np.array([fm_bar + EPS * fm] + [2 * EPS * w for w in want[1:]])          # fp64 sums rounded once to fp32
    print("finish: error / bar", np.abs(got - want) / bars)
    assert (np.abs(got - want) <= bars).all()
    # the gradients: coefficients formed in fp64 and rounded once, signs exact
    up = rng.rand(4).astype(np.float32) + 0.5
    up_d = _dev(up)
    for l in range(5):
        G = torch.full(tuple(bufs[l].shape), float("nan"), device=DEV)
        check(lib.radmmm_mpd_fm_grad(ptr(bufs[l]), ptr(cnt_d[l]) if ragged else None, ptr(norm[l:]), ptr(up_d), ptr(G), B, p, Hs[l], Cs[l],
                                     stream()), "fm_grad")
        G = G.cpu().numpy()
        assert np.isnan(G[:, :, :, :2]).all() and np.isnan(G[:, :, :, Hs[l] + 2:]).all()
        m = (np.arange(Hs[l])[None, :] < eff[l][:, None])[:, None, :, None]
        coef = np.float32(np.float64(up[0]) / float(norm[l]))
        w = (coef * np.sign(maps[l][0] - maps[l][1]) * m).astype(np.float32)
        assert np.array_equal(G[0, :, :, 2:2 + Hs[l]], w) and np.array_equal(G[1, :, :, 2:2 + Hs[l]], -w)
    dO = torch.full((2, B, Hs[4], p), float("nan"), device=DEV)
    check(lib.radmmm_mpd_out_grad(ptr(out_d), ptr(cnt_d), ptr(norm), ptr(up_d), ptr(dO), B, p, Hs[4], stream()), "out_grad")
    dO = dO.cpu().numpy().reshape(2, B, -1).astype(np.float64)
    mh = np.repeat(np.arange(Hs[4])[None, :] < eff[5][:, None], p, axis=1)
    cf = np.where(mh, np.float64(up[0]) / float(norm[5]) * np.sign(np.where(mh, dr - dg, 0.0)), 0.0)
    want_r = np.where(mf, -2 * (1 - np.where(mf, dr, 0)) * up[1] / n6, 0.0) + cf
    want_g = np.where(mf, (2 * np.where(mf, dg, 0) * up[2] - 2 * (1 - np.where(mf, dg, 0)) * up[3]) / n6, 0.0) - cf
    tol = 8 * EPS * (np.abs(want_r).max() + np.abs(want_g).max() + np.abs(cf).max())
    assert np.abs(dO[0] - want_r).max() <= tol and np.abs(dO[1] - want_g).max() <= tol
