"""The entry points of csrc/msd.hip (include/radmmm_hip.h, "grouped strided 1-d convolution"), each alone against a float64 /
integer model written here from the header's formulas.

With small integer operands (inputs in [-4, 4], weights and gradients in [-2, 2]) every product and every partial sum is an
integer far below 2^24 (at most 41 * 64 * 8 = 20 992 per forward element, 3 * 131 * 8 per weight-gradient element), so any
summation order gives the same bits and the results are held BIT FOR BIT, the zero pad rows of the output buffer included.
The same cases with realistic values stay within n * 2^-23 * sum |a||b| per element (n terms, as test_hip_gemm_f32_direct
does).  NaN is planted wherever a kernel must not read or write: a sequence past the last one, the pad rows of an upstream
gradient, a partial-sum block past the last split.

Shapes: the reference's five (G, Cin_g, Cout_g, stride) with 41 taps, two narrow ones (4 and 8 wide: masked edges of an
MFMA tile), two with other tap counts whose widths (12, 20) leave a partial second tile, the widest accepted corner
(64 channels per group at stride 4 and 41 taps: the forward's largest LDS carve-up) and two with fewer taps than the stride
(phases of the data gradient that meet no tap: only the map's own gradient times the derivative).  S = 3; input lengths 1, 7 and
131 (five row tiles, the last partial; at stride 4 two tiles; uneven split ranges)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
S = 3
SLOPE = 0.1
#        G, Cin_g, Cout_g, stride, k
SHAPES = [(4, 32, 32, 2, 41), (16, 8, 16, 2, 41), (16, 16, 32, 4, 41), (16, 32, 64, 4, 41), (16, 64, 64, 1, 41),
          (2, 4, 4, 2, 41), (4, 4, 8, 4, 41), (3, 12, 20, 1, 5), (2, 20, 12, 2, 3),
          (1, 64, 64, 4, 41),         # the widest accepted corner: the forward's largest LDS carve-up (62 800 bytes)
          (2, 4, 4, 4, 3), (2, 8, 4, 2, 1)]   # fewer taps than the stride: the data gradient's phases without a tap
LENGTHS = (1, 7, 131)
CASES = [(*sh, H) for sh in SHAPES for H in LENGTHS]


def _lib():
    from rad_mmm_amd._lib import check, lib, ptr, stream
    return check, lib, ptr, stream


def _data(shape, integers, seed, H):
    """X [S, Hin + k - 1, Cin] (pad rows zero), W [G, Cout_g, k, Cin_g], bias [Cout], dZ [S, Hout, Cout], add like X with NaN pad rows"""
    G, ci, co, st, k = shape
    rng = np.random.RandomState(seed)
    Ho, pin = (H - 1) // st + 1, k // 2

    def draw(lim, *dims):
        return (rng.randint(-lim, lim + 1, dims) if integers else rng.randn(*dims) * lim / 2).astype(np.float32)

    X = np.zeros((S, H + 2 * pin, G * ci), np.float32)
    X[:, pin:pin + H] = draw(4, S, H, G * ci)
    W = draw(2, G, co, k, ci) if integers else (draw(2, G, co, k, ci) / np.sqrt(k * ci)).astype(np.float32)
    add = np.full_like(X, np.nan)
    add[:, pin:pin + H] = draw(2, S, H, G * ci)
    return X, W, draw(2, G * co), draw(2, S, Ho, G * co), add, Ho, pin


def _conv(X, W, st, Ho):
    """float64 [S, Ho, Cout]: sum_kk X[s][st h' + tap][g Cin_g + ci] W[g][co][tap][ci]"""
    G, co, k, ci = W.shape
    X, W = X.astype(np.float64), W.astype(np.float64)
    out = np.zeros((X.shape[0], Ho, G * co))
    for g in range(G):
        for tap in range(k):
            out[:, :, g * co:(g + 1) * co] += X[:, tap:tap + st * (Ho - 1) + 1:st, g * ci:(g + 1) * ci] @ W[g, :, tap].T
    return out


def _conv_adjoint(dZ, W, st, Hp):
    """float64 [S, Hp, Cin]: the gradient of _conv with respect to its padded input"""
    G, co, k, ci = W.shape
    dZ, W = dZ.astype(np.float64), W.astype(np.float64)
    Ho = dZ.shape[1]
    out = np.zeros((dZ.shape[0], Hp, G * ci))
    for g in range(G):
        for tap in range(k):
            out[:, tap:tap + st * (Ho - 1) + 1:st, g * ci:(g + 1) * ci] += dZ[:, :, g * co:(g + 1) * co] @ W[g, :, tap]
    return out


def _wgrad(dZ, X, shape, rows=None):
    """float64 [G, Cout_g, k, Cin_g] over the (s, h') pairs in rows (all when None)"""
    G, ci, co, st, k = shape
    dZ, X = dZ.astype(np.float64), X.astype(np.float64)
    Ho = dZ.shape[1]
    if rows is not None:
        keep = np.zeros((dZ.shape[0], Ho, 1))
        for s, h in rows:
            keep[s, h] = 1.0
        dZ = dZ * keep
    out = np.zeros((G, co, k, ci))
    for g in range(G):
        zg = dZ[:, :, g * co:(g + 1) * co].reshape(-1, co)
        for tap in range(k):
            out[g, :, tap] = zg.T @ X[:, tap:tap + st * (Ho - 1) + 1:st, g * ci:(g + 1) * ci].reshape(-1, ci)
    return out


def _lrelu(v):
    return np.where(v > 0, v, SLOPE * v)


def _with_nan_tail(a):
    """device copy with one more leading block of NaN behind it: what lies past the last sequence must not be read"""
    t = torch.full((a.shape[0] + 1, *a.shape[1:]), float("nan"), device=DEV)
    t[:-1] = torch.as_tensor(a)
    return t


@pytest.mark.parametrize("integers", (True, False), ids=("integers", "realistic"))
@pytest.mark.parametrize("G,ci,co,st,k,H", CASES)
def test_forward(G, ci, co, st, k, H, integers):
    check, lib, ptr, stream = _lib()
    shape = (G, ci, co, st, k)
    X, W, bias, _, _, Ho, pin = _data(shape, integers, 7 * H + k + G, H)
    for po in (20, 2, 0):
        Xd, Wd, bd = _with_nan_tail(X), _with_nan_tail(W.reshape(1, -1)), torch.as_tensor(bias).to(DEV)
        Y = torch.full((S + 1, Ho + 2 * po, G * co), float("nan"), device=DEV)
        check(lib.radmmm_msd_gconv_fwd(ptr(Xd), ptr(Wd), ptr(bd), ptr(Y), S, H, Ho, G, ci, co, k, st, po, SLOPE, stream()), "fwd")
        got = Y.cpu().numpy()
        assert np.isnan(got[S]).all()
        pre = _conv(X, W, st, Ho) + bias.astype(np.float64)
        want = np.zeros((S, Ho + 2 * po, G * co))
        want[:, po:po + Ho] = _lrelu(pre)
        if integers:
            # slope * v is one fp32 multiplication of an exact integer: the model rounds the same product once
            want[:, po:po + Ho] = np.where(pre > 0, pre, (np.float32(SLOPE) * pre.astype(np.float32)).astype(np.float64))
            assert np.array_equal(got[:S], want.astype(np.float32))
        else:
            assert np.array_equal(got[:S, :po], want[:, :po]) and np.array_equal(got[:S, po + Ho:], want[:, po + Ho:])
            bound = (k * ci + 2) * 2.0 ** -23 * (_conv(np.abs(X), np.abs(W), st, Ho) + np.abs(bias))
            err = np.abs(got[:S, po:po + Ho] - want[:, po:po + Ho])
            assert (err <= bound).all(), float((err / bound).max())


@pytest.mark.parametrize("integers", (True, False), ids=("integers", "realistic"))
@pytest.mark.parametrize("G,ci,co,st,k,H", CASES)
def test_data_gradient(G, ci, co, st, k, H, integers):
    check, lib, ptr, stream = _lib()
    shape = (G, ci, co, st, k)
    X, W, _, dZ, add, Ho, pin = _data(shape, integers, 11 * H + k + G, H)
    Xd, Wd, Zd = _with_nan_tail(X), _with_nan_tail(W.reshape(1, -1)), _with_nan_tail(dZ)
    deriv = np.where(X[:, pin:pin + H] > 0, 1.0, np.float64(np.float32(SLOPE)))
    base = _conv_adjoint(dZ, W, st, H + 2 * pin)[:, pin:pin + H]
    for with_add in (True, False):
        dX = torch.full((S + 1, H, G * ci), float("nan"), device=DEV)
        Ad = _with_nan_tail(add) if with_add else None
        check(lib.radmmm_msd_gconv_dgrad(ptr(Zd), ptr(Wd), ptr(Ad), ptr(Xd), ptr(dX), S, H, Ho, G, ci, co, k, st, SLOPE, stream()),
              "dgrad")
        got = dX.cpu().numpy()
        assert np.isnan(got[S]).all()
        summed = base + (add[:, pin:pin + H] if with_add else 0.0)
        if integers:
            want = (summed.astype(np.float32) * deriv.astype(np.float32))          # one fp32 product of an exact integer
            assert np.array_equal(got[:S], want)
        else:
            terms = _conv_adjoint(np.abs(dZ), np.abs(W), st, H + 2 * pin)[:, pin:pin + H] + (np.abs(add[:, pin:pin + H]) if with_add else 0.0)
            n = ((k - 1) // st + 1) * co + 2
            err = np.abs(got[:S] - summed * deriv)
            assert (err <= n * 2.0 ** -23 * terms).all(), float((err / (n * 2.0 ** -23 * terms + 1e-300)).max())


@pytest.mark.parametrize("integers", (True, False), ids=("integers", "realistic"))
@pytest.mark.parametrize("G,ci,co,st,k,H", CASES)
def test_weight_gradient(G, ci, co, st, k, H, integers):
    check, lib, ptr, stream = _lib()
    shape = (G, ci, co, st, k)
    X, W, _, dZ, _, Ho, pin = _data(shape, integers, 13 * H + k + G, H)
    Xd, Zd = _with_nan_tail(X), _with_nan_tail(dZ)
    n = int(lib.radmmm_msd_gconv_wgrad_splits(S, Ho, G, k))
    nch = -(-Ho // 32)
    units = S * nch
    assert 1 <= n <= min(units, 64)
    cols = G * co * k * ci
    P = torch.full((n + 1, cols), float("nan"), device=DEV)
    check(lib.radmmm_msd_gconv_wgrad(ptr(Zd), ptr(Xd), ptr(P), S, H, Ho, G, ci, co, k, st, stream()), "wgrad")
    dW = torch.full((2, cols), float("nan"), device=DEV)
    check(lib.radmmm_colsum_final(ptr(P), ptr(dW), n, cols, stream()), "colsum_final")
    got_p, got = P.cpu().numpy(), dW.cpu().numpy()
    assert np.isnan(got_p[n]).all() and np.isnan(got[1]).all()
    want = _wgrad(dZ, X, shape).reshape(-1)
    if integers:
        assert np.array_equal(got[0], want.astype(np.float32))
        for i in range(n):            # split i takes units [i U / n, (i + 1) U / n), a unit = 32 windows of one sequence
            rows = [(u // nch, h) for u in range(units * i // n, units * (i + 1) // n)
                    for h in range(32 * (u % nch), min(32 * (u % nch) + 32, Ho))]
            assert np.array_equal(got_p[i], _wgrad(dZ, X, shape, rows).reshape(-1).astype(np.float32)), i
    else:
        bound = (S * Ho + n) * 2.0 ** -23 * _wgrad(np.abs(dZ), np.abs(X), shape).reshape(-1)
        err = np.abs(got[0] - want)
        assert (err <= bound).all(), float((err / (bound + 1e-300)).max())


# ---- what surrounds the grouped convolutions: pools, the first conv's frames, repad, the eight-map loss kernels -----------
EPS = 2.0 ** -24


def _pool_matrix(T):
    """[To, T]: AvgPool1d(4, 2, padding 2) with the zero pad counted, To = T // 2 + 1"""
    To = T // 2 + 1
    P = np.zeros((To, T))
    for j in range(To):
        for t in range(2 * j - 2, 2 * j + 2):
            if 0 <= t < T:
                P[j, t] = 0.25
    return P


@pytest.mark.parametrize("T", (1, 2, 3, 8, 97, 1030))
def test_avgpool_and_its_adjoint(T):
    """integers that are multiples of 4: every window sum and its quarter are exact, so both directions are bit for bit"""
    check, lib, ptr, stream = _lib()
    rng = np.random.RandomState(T)
    B, ld, To = 3, T + 5, T // 2 + 1
    y = np.full((B, ld), np.nan, np.float32)
    yh = np.full((B, ld), np.nan, np.float32)
    y[:, :T], yh[:, :T] = 4 * rng.randint(-8, 9, (B, T)), 4 * rng.randint(-8, 9, (B, T))
    out = torch.full((2 * B + 1, To), float("nan"), device=DEV)
    yd, yhd = torch.as_tensor(y).to(DEV), torch.as_tensor(yh).to(DEV)
    check(lib.radmmm_msd_avgpool(ptr(yd), ptr(yhd), ld, ptr(out), B, T, stream()), "avgpool")
    P = _pool_matrix(T)
    got = out.cpu().numpy()
    assert np.isnan(got[2 * B]).all()
    assert np.array_equal(got[:2 * B], np.concatenate([y[:, :T] @ P.T, yh[:, :T] @ P.T]).astype(np.float32))
    g = (4 * rng.randint(-8, 9, (B, To))).astype(np.float32)
    gx = torch.full((B + 1, ld), float("nan"), device=DEV)
    gd = torch.as_tensor(g).to(DEV)
    check(lib.radmmm_msd_avgpool_bwd(ptr(gd), ptr(gx), ld, B, T, stream()), "avgpool_bwd")
    got = gx.cpu().numpy()
    assert np.isnan(got[B]).all() and np.isnan(got[:B, T:]).all()
    assert np.array_equal(got[:B, :T], (g @ P).astype(np.float32))


@pytest.mark.parametrize("T", (1, 7, 8, 15, 97))
def test_frame15_is_a_copy_and_unframe15_its_adjoint(T):
    check, lib, ptr, stream = _lib()
    rng = np.random.RandomState(T)
    B, ld = 2, T + 3
    y = np.full((B, ld), np.nan, np.float32)
    yh = np.full((B, ld), np.nan, np.float32)
    y[:, :T], yh[:, :T] = rng.randn(B, T), rng.randn(B, T)
    F = torch.full((2 * B * T + 1, 16), float("nan"), device=DEV)
    yd, yhd = torch.as_tensor(y).to(DEV), torch.as_tensor(yh).to(DEV)
    check(lib.radmmm_msd_frame15(ptr(yd), ptr(yhd), ld, ptr(F), B, T, stream()), "frame15")
    x = np.concatenate([y[:, :T], yh[:, :T]])
    xp = np.zeros((2 * B, T + 14), np.float32)
    xp[:, 7:7 + T] = x
    want = np.zeros((2 * B, T, 16), np.float32)
    for j in range(15):
        want[:, :, j] = xp[:, j:j + T]
    got = F.cpu().numpy()
    assert np.isnan(got[2 * B * T]).all() and np.array_equal(got[:2 * B * T].reshape(want.shape), want)
    dF = rng.randint(-4, 5, (2 * B, T, 16)).astype(np.float32)
    dFn = dF.copy()
    dFn[:, :, 15] = np.nan                            # the pad column is never read
    g = torch.full((2 * B + 1, ld), float("nan"), device=DEV)
    dd = torch.as_tensor(dFn).to(DEV)
    check(lib.radmmm_msd_unframe15(ptr(dd), ptr(g), ld, 2 * B, T, stream()), "unframe15")
    wantg = np.zeros((2 * B, T + 14))
    for j in range(15):
        wantg[:, j:j + T] += dF[:, :, j]
    got = g.cpu().numpy()
    assert np.isnan(got[2 * B]).all() and np.isnan(got[:2 * B, T:]).all()
    assert np.array_equal(got[:2 * B, :T], wantg[:, 7:7 + T].astype(np.float32))


@pytest.mark.parametrize("pad", (0, 1, 2, 20))
@pytest.mark.parametrize("H,C", ((1, 4), (7, 8), (33, 128)))
def test_repad(H, C, pad):
    check, lib, ptr, stream = _lib()
    rng = np.random.RandomState(H + C + pad)
    ldz = C + 4
    Z = np.full((S * H, ldz), np.nan, np.float32)
    Z[:, :C] = rng.randn(S * H, C)
    X = torch.full((S + 1, H + 2 * pad, C), float("nan"), device=DEV)
    Zd = torch.as_tensor(Z).to(DEV)
    check(lib.radmmm_msd_repad(ptr(Zd), ldz, ptr(X), S, H, C, pad, SLOPE, stream()), "repad")
    want = np.zeros((S, H + 2 * pad, C), np.float32)
    z = Z[:, :C].reshape(S, H, C)
    want[:, pad:pad + H] = np.where(z > 0, z, np.float32(SLOPE) * z)
    got = X.cpu().numpy()
    assert np.isnan(got[S]).all() and np.array_equal(got[:S], want)


@pytest.mark.parametrize("B,ratios", ((2, (1.0, 0.7)), (3, (1.0, 0.7, 0.5)), (2, None)))
def test_eight_map_loss_terms_finish_and_gradients(B, ratios):
    """msd_fm_terms / msd_finish / msd_fm_grad / msd_out_grad on eight maps of the multi-scale geometry (pads 20 and 2, the
    dense output), NaN in every pad row: the four terms and the normalisers against float64 within n * 2^-24 * sum |terms|,
    the gradients against the formulas (one fp32 product each: 4 ulp)"""
    import ctypes
    check, lib, ptr, stream = _lib()
    rng = np.random.RandomState(B)
    Cs, Hs, pads = [8, 8, 16, 16, 32, 32, 16, 1], [97, 49, 25, 7, 2, 2, 2, 2], [20, 20, 20, 20, 20, 2, 2, -1]
    maps, dev_maps = [], []
    for C, H, pad in zip(Cs, Hs, pads):
        m = rng.randn(2 * B, H, C).astype(np.float32)
        eq = rng.rand(B, H, C) < 0.1
        m[B:][eq] = m[:B][eq]                                                          # r == g: sign(0) = 0
        maps.append(m)
        if pad >= 0:
            buf = np.full((2 * B, H + 2 * pad, C), np.nan, np.float32)
            buf[:, pad:pad + H] = m
        else:
            buf = m.reshape(2 * B, H)
        dev_maps.append(torch.as_tensor(buf).to(DEV))
    if ratios is None:
        cnt, cnt_d = None, None
        counts = [[H] * B for H in Hs] + [[Hs[7]] * B]
    else:
        counts = [[int(np.ceil(np.float32(r) * np.float32(H))) for r in ratios] for H in Hs + [Hs[7]]]
        counts[3][1] = Hs[3] + 5                                                       # read clamped to the map's rows
        counts[4][0] = -3
        cnt = np.asarray(counts, np.int32)
        cnt_d = torch.as_tensor(cnt).to(DEV)
        counts = [[min(max(c, 0), H) for c in row] for row, H in zip(counts, Hs + [Hs[7]])]
    offs = [0]
    for C, H in zip(Cs, Hs):
        offs.append(offs[-1] + int(lib.radmmm_mpd_fm_terms_parts(B, 1, H, C)))
    part = torch.full((offs[-1] + 1,), float("nan"), device=DEV)
    for l in range(8):
        check(lib.radmmm_msd_fm_terms(ptr(dev_maps[l]), ptr(cnt_d[l]) if cnt_d is not None else None, ptr(part[offs[l]:]), B, Hs[l],
                                      Cs[l], pads[l], stream()), "fm_terms")
    res = torch.full((5,), float("nan"), device=DEV)
    norm = torch.full((10,), float("nan"), device=DEV, dtype=torch.float64)
    i32 = ctypes.c_int32
    check(lib.radmmm_msd_finish(ptr(part), (i32 * 9)(*offs), (i32 * 8)(*Cs), (i32 * 8)(*Hs), ptr(dev_maps[7]), ptr(cnt_d), ptr(res),
                                ptr(norm), B, stream()), "finish")
    fm, fm_abs, want_norm = 0.0, 0.0, []
    for l in range(8):
        mask = (np.arange(Hs[l])[None, :] < np.asarray(counts[l])[:, None]).astype(np.float64)
        d = np.abs(maps[l][:B].astype(np.float64) - maps[l][B:].astype(np.float64)) * mask[:, :, None]
        want_norm.append(mask.sum() * Cs[l])
        fm += d.sum() / want_norm[-1]
        fm_abs += (Hs[l] * Cs[l] * B + 64) * EPS * d.sum() / want_norm[-1]
    mo = (np.arange(Hs[7])[None, :] < np.asarray(counts[8])[:, None]).astype(np.float64)
    want_norm.append(mo.sum())
    dr, dg = maps[7][:B, :, 0].astype(np.float64), maps[7][B:, :, 0].astype(np.float64)
    want = [fm, ((1 - dr) ** 2 * mo).sum() / mo.sum(), (dg ** 2 * mo).sum() / mo.sum(), ((1 - dg) ** 2 * mo).sum() / mo.sum()]
    got, gn = res.cpu().numpy(), norm.cpu().numpy()
    assert np.isnan(got[4]) and np.isnan(gn[9]) and np.isnan(part.cpu().numpy()[-1])
    assert np.array_equal(gn[:9], np.asarray(want_norm))
    assert abs(got[0] - want[0]) <= fm_abs + EPS * abs(want[0])
    for j in range(1, 4):
        assert abs(got[j] - want[j]) <= 2 * EPS * abs(want[j]), j
    up = np.asarray([0.75, -1.5, 0.5, 2.0], np.float32)
    up_d = torch.as_tensor(up).to(DEV)
    for l in range(7):
        G = torch.full_like(dev_maps[l], float("nan"))
        check(lib.radmmm_msd_fm_grad(ptr(dev_maps[l]), ptr(cnt_d[l]) if cnt_d is not None else None, ptr(norm[l:]), ptr(up_d), ptr(G), B,
                                     Hs[l], Cs[l], pads[l], stream()), "fm_grad")
        mask = (np.arange(Hs[l])[None, :] < np.asarray(counts[l])[:, None])[:, :, None]
        coef = np.float32(np.float64(up[0]) / want_norm[l])
        wantg = coef * np.sign(maps[l][:B] - maps[l][B:]) * mask
        got = G.cpu().numpy()
        pad = pads[l]
        assert np.isnan(got[:, :pad]).all() and np.isnan(got[:, pad + Hs[l]:]).all()             # pad rows are not written
        assert np.array_equal(got[:B, pad:pad + Hs[l]], wantg.astype(np.float32))
        assert np.array_equal(got[B:, pad:pad + Hs[l]], -wantg.astype(np.float32))
    dOut = torch.full((2 * B + 1, Hs[7]), float("nan"), device=DEV)
    check(lib.radmmm_msd_out_grad(ptr(dev_maps[7]), ptr(cnt_d), ptr(norm), ptr(up_d), ptr(dOut), B, Hs[7], stream()), "out_grad")
    mh = np.arange(Hs[7])[None, :] < np.asarray(counts[7])[:, None]
    cf = np.float64(up[0]) / want_norm[7] * np.sign(dr - dg) * mh
    inv = 1.0 / want_norm[8]
    want_r = -2.0 * up[1] * inv * (1 - dr) * mo + cf
    want_g = (2.0 * up[2] * inv * dg - 2.0 * up[3] * inv * (1 - dg)) * mo - cf
    got = dOut.cpu().numpy()
    assert np.isnan(got[2 * B]).all()
    scale = 4 * EPS * (np.abs(want_r).max() + np.abs(want_g).max() + 1)
    assert np.abs(got[:B] - want_r).max() <= scale and np.abs(got[B:2 * B] - want_g).max() <= scale
