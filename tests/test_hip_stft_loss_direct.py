"""The five kernels of csrc/stft_loss.hip through the C ABI, each against the numpy model tests/_stft_loss_ref.py.
Outputs are pre-filled with NaN, and NaN is planted wherever a kernel must not read: past T in a wider signal, in items
without valid frames, in invalid rows and in the pad columns of the matrices.

Bars.  frame is a copy and unframe sums small integers: both are compared for equality.  A partial of terms is a sum of n
bins evaluated in fp32: |got - want| <= n * 2^-23 * sum |terms| (want: float64 from the same fp32 spectra).  finish adds in
fp64: the same bar over the rows.  An element of bwd is dmag * re / mag with dmag a sum of at most three products of
rounded factors: 16 * 2^-24 times the sum of the absolute values of those products (with ym + xm for |ym - xm|, whose
rounding error scales with the magnitudes), times |re| / mag."""
import numpy as np
import pytest
import torch

import _stft_loss_ref as K

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN = float("nan")


def _lib():
    from rad_mmm_amd._lib import check, lib, ptr, stream
    return lib, check, ptr, stream


def _dev(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


# (B, T, ldx, n_fft, hop, win, frames): hop 1 / 5 / 12 / 50, win == n_fft, an odd left pad (13) and an uneven one (39 of
# 64), ldx > T, T = n_fft/2 + 1 (samples with both mirrors), frame counts 0, 1 and F
def _cases():
    out = []
    for B, T, ldx, n_fft, hop, win, frames in (
            (3, 100, 100, 32, 1, 32, "F10"), (3, 77, 80, 64, 5, 39, "F10"), (2, 600, 600, 64, 12, 38, None),
            (3, 300, 301, 128, 50, 100, "3F0"), (3, 33, 40, 64, 5, 64, "F01"), (3, 17, 17, 32, 1, 7, "F10")):
        F = 1 + T // hop
        fr = None if frames is None else np.array([{"F": F, "1": 1, "0": 0, "3": 3}[c] for c in frames], dtype=np.int32)
        out.append(pytest.param(B, T, ldx, n_fft, hop, win, fr, id=f"T{T}-fft{n_fft}-hop{hop}-win{win}-{frames}"))
    return out


def _frame_gpu(x, ldx, frames, B, T, n_fft, hop, win, ldk):
    lib, check, ptr, stream = _lib()
    F = 1 + T // hop
    A = torch.full((B * F, ldk), NAN, device=DEV)
    check(lib.radmmm_stftloss_frame(ptr(x), ldx, ptr(frames), ptr(A), ldk, B, T, F, n_fft, hop, win, stream()), "frame")
    return A


@pytest.mark.parametrize("B,T,ldx,n_fft,hop,win,frames", _cases())
def test_frame_is_bit_equal_to_the_model(B, T, ldx, n_fft, hop, win, frames):
    x = np.random.RandomState(T + hop).randn(B, ldx).astype(np.float32)
    want = K.frame(x[:, :T], frames, n_fft, hop, win, ldk=(win + 3) // 4 * 4)
    x[:, T:] = NAN
    if frames is not None:
        x[frames == 0] = NAN                                       # an item without valid frames is not read
    got = _frame_gpu(_dev(x), ldx, _dev(frames), B, T, n_fft, hop, win, want.shape[1])
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_frame_grid_stride_loop_wraps():
    """8 x 40001 rows of 8 float4 groups: more than the 8192 x 256 threads of the capped grid"""
    B, T, n_fft, hop, win = 8, 40000, 32, 1, 32
    x = np.random.RandomState(3).randn(B, T).astype(np.float32)
    frames = np.array([T + 1, 1, 0, 40000, 77, T + 1, 2, 12345], dtype=np.int32)
    assert B * (T + 1) * (win // 4) > 8192 * 256
    got = _frame_gpu(_dev(x), T, _dev(frames), B, T, n_fft, hop, win, win)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), K.frame(x, frames, n_fft, hop, win).view(np.uint32))


def _unframe_gpu(dA, ldk, frames, B, T, lddx, n_fft, hop, win, prefill=None):
    lib, check, ptr, stream = _lib()
    F = 1 + T // hop
    dx = torch.full((B, lddx), NAN, device=DEV) if prefill is None else prefill.clone()
    check(lib.radmmm_stftloss_unframe(ptr(dA), ldk, ptr(frames), ptr(dx), lddx, B, T, F, n_fft, hop, win,
                                      int(prefill is not None), stream()), "unframe")
    return dx


@pytest.mark.parametrize("B,T,ldx,n_fft,hop,win,frames", _cases())
def test_unframe_is_exactly_the_model_on_integers(B, T, ldx, n_fft, hop, win, frames):
    rng = np.random.RandomState(T + win)
    F = 1 + T // hop
    ldk = (win + 3) // 4 * 4
    dA = rng.randint(-8, 9, size=(B, F, ldk)).astype(np.float32)
    want = K.unframe(dA.reshape(B * F, ldk), frames, T, n_fft, hop, win)
    assert np.array_equal(want, K.unframe_fast(dA.reshape(B * F, ldk), frames, T, n_fft, hop, win))
    dA[:, :, win:] = NAN
    if frames is not None:
        dA[np.arange(F)[None, :] >= frames[:, None]] = NAN
    got = _unframe_gpu(_dev(dA), ldk, _dev(frames), B, T, ldx, n_fft, hop, win).cpu().numpy()
    assert np.array_equal(got[:, :T].astype(np.float64), want) and np.isnan(got[:, T:]).all()
    if T == n_fft // 2 + 1:                                       # every inner sample has both mirrors
        assert not np.array_equal(want, K.unframe(dA.reshape(B * F, ldk), frames, T, n_fft, hop, win, bug="drop_mirror"))
    pre = rng.randint(-8, 9, size=(B, ldx)).astype(np.float32)
    acc = _unframe_gpu(_dev(dA), ldk, _dev(frames), B, T, ldx, n_fft, hop, win, prefill=_dev(pre)).cpu().numpy()
    assert np.array_equal(acc[:, :T].astype(np.float64), want + pre[:, :T]) and np.array_equal(acc[:, T:], pre[:, T:])


def test_unframe_grid_stride_loop_wraps():
    B, T, n_fft, hop, win = 64, 40000, 32, 50, 32
    F = 1 + T // hop
    assert B * T > 8192 * 256
    rng = np.random.RandomState(5)
    dA = rng.randint(-8, 9, size=(B * F, win)).astype(np.float32)
    frames = rng.randint(0, F + 1, size=B).astype(np.int32)
    got = _unframe_gpu(_dev(dA), win, _dev(frames), B, T, T, n_fft, hop, win).cpu().numpy()
    assert np.array_equal(got.astype(np.float64), K.unframe_fast(dA, frames, T, n_fft, hop, win))


def _spectra(cutoff, B, F, frames, seed):
    """fp32 spectra [B*F, lds] of two signals with a few bins below the clamp in x only; NaN in invalid rows and in the
    pad columns"""
    rng = np.random.RandomState(seed)
    lds = (2 * cutoff + 3) // 4 * 4
    sx = rng.randn(B * F, lds).astype(np.float32)
    sy = (sx + 0.5 * rng.randn(B * F, lds)).astype(np.float32)
    sx[:, 3] *= 1e-5
    sx[:, cutoff + 3] *= 1e-5                                     # bin 3 of x: power ~1e-10, below the clamp
    sx[0, 5] = sx[0, cutoff + 5] = 0.0                            # and one exact zero
    nf = np.full(B, F) if frames is None else frames
    valid = (np.arange(F)[None, :] < nf[:, None]).reshape(-1)
    for s in (sx, sy):
        s[~valid] = NAN
        s[:, 2 * cutoff:] = NAN
    return sx, sy, lds, valid


def _model_terms(sx, sy, cutoff, valid, a_w):
    f = lambda a: np.nan_to_num(a.astype(np.float64))             # noqa: E731
    part, xm, ym, dl = K.terms(f(sx[:, :cutoff]), f(sx[:, cutoff:2 * cutoff]), f(sy[:, :cutoff]), f(sy[:, cutoff:2 * cutoff]),
                               valid.astype(np.float64), a_w)
    return part, xm, ym, dl


@pytest.mark.parametrize("a_w", [False, True])
@pytest.mark.parametrize("ragged", [True, False])
@pytest.mark.parametrize("cutoff", [17, 33, 65, 1025])
def test_terms_and_finish_within_the_summation_bar(cutoff, ragged, a_w):
    """17 bins: fewer than a wave's lanes; 1025: more than a workgroup's threads"""
    lib, check, ptr, stream = _lib()
    B, F = 3, 7
    frames = np.array([7, 3, 0], dtype=np.int32) if ragged else None
    sx, sy, lds, valid = _spectra(cutoff, B, F, frames, cutoff)
    want, xm, ym, dl = _model_terms(sx, sy, cutoff, valid, a_w)
    dsx, dsy, dfr = _dev(sx), _dev(sy), _dev(frames)
    part = torch.full((B * F, 4), NAN, device=DEV)
    check(lib.radmmm_stftloss_terms(ptr(dsx), ptr(dsy), lds, ptr(dfr), ptr(part), B, F, cutoff, int(a_w), stream()), "terms")
    got = part.cpu().numpy()
    assert not got[:, 3].any() and not got[~valid].any()
    sums = np.stack([((ym - xm) ** 2).sum(-1), (ym ** 2).sum(-1), np.abs(dl).sum(-1)], -1) * valid[:, None]
    bar = cutoff * 2.0 ** -23 * sums
    err = np.abs(got[:, :3].astype(np.float64) - want)
    print(f"terms cutoff {cutoff}: worst measured / bar {np.max(err[valid] / bar[valid]):.3f}")
    assert (err <= bar).all()
    # finish, from the kernel's own partials
    out = torch.full((2,), NAN, device=DEV)
    norm = torch.full((4,), NAN, device=DEV, dtype=torch.float64)
    check(lib.radmmm_stftloss_finish(ptr(part), ptr(dfr), ptr(out), ptr(norm), B, F, cutoff, stream()), "finish")
    p = got.astype(np.float64)
    S = float(valid.sum())
    D, N, L = p[valid, 0], p[valid, 1], p[valid, 2]
    sc = (np.sqrt(D) / np.sqrt(N)).sum() / S if ragged else np.sqrt(D.sum()) / np.sqrt(N.sum())
    sc_terms = (np.sqrt(D) / np.sqrt(N)).sum() / S if ragged else sc
    mag = L.sum() / (S * cutoff)
    o, n = out.cpu().numpy().astype(np.float64), norm.cpu().numpy()
    rows = B * F
    assert abs(o[0] - sc) <= rows * 2.0 ** -23 * sc_terms and abs(o[1] - mag) <= rows * 2.0 ** -23 * mag
    assert n[0] == S and n[3] == 0.0
    assert abs(n[1] - D.sum()) <= rows * 2.0 ** -52 * D.sum() and abs(n[2] - N.sum()) <= rows * 2.0 ** -52 * N.sum()


@pytest.mark.parametrize("a_w", [False, True])
@pytest.mark.parametrize("ragged", [True, False])
@pytest.mark.parametrize("cutoff", [17, 65, 1025])
def test_bwd_within_the_derived_bar_and_exact_zeros(cutoff, ragged, a_w):
    lib, check, ptr, stream = _lib()
    B, F = 3, 7
    frames = np.array([7, 3, 0], dtype=np.int32) if ragged else None
    sx, sy, lds, valid = _spectra(cutoff, B, F, frames, 100 + cutoff)
    part64, xm, ym, dl = _model_terms(sx, sy, cutoff, valid, a_w)
    live = valid[:, None] & ~((xm <= np.sqrt(K.CLAMP)) & (ym <= np.sqrt(K.CLAMP)))
    assert np.abs(dl[live]).min() > 1e-5                          # no bin near the |dlog| kink
    dsx, dsy, dfr = _dev(sx), _dev(sy), _dev(frames)
    part = torch.full((B * F, 4), NAN, device=DEV)
    out = torch.empty(2, device=DEV)
    norm = torch.empty(4, device=DEV, dtype=torch.float64)
    check(lib.radmmm_stftloss_terms(ptr(dsx), ptr(dsy), lds, ptr(dfr), ptr(part), B, F, cutoff, int(a_w), stream()), "terms")
    check(lib.radmmm_stftloss_finish(ptr(part), ptr(dfr), ptr(out), ptr(norm), B, F, cutoff, stream()), "finish")
    g_sc, g_mag, scale = 0.7, -1.3, 1.0 / 3.0
    dg_sc, dg_mag = torch.tensor(g_sc, device=DEV), torch.tensor(g_mag, device=DEV)

    def run(want_x, want_y):
        d = [torch.full((B * F, lds), NAN, device=DEV) if w else None for w in (want_x, want_y)]
        check(lib.radmmm_stftloss_bwd(ptr(dsx), ptr(dsy), lds, ptr(part), ptr(norm), ptr(dfr), ptr(dg_sc), ptr(dg_mag),
                                      scale, ptr(d[0]), ptr(d[1]), B, F, cutoff, int(a_w), stream()), "bwd")
        return [None if t is None else t.cpu().numpy() for t in d]

    gx, gy = run(True, True)
    assert np.array_equal(run(True, False)[0], gx) and np.array_equal(run(False, True)[1], gy)
    # the model, in float64, from the kernel's own partials and normalisers
    p, n = part.cpu().numpy().astype(np.float64), norm.cpu().numpy()
    S = n[0]
    D, N = (p[:, 0], np.where(valid, p[:, 1], 1.0)) if ragged else (np.full(B * F, n[1]), np.full(B * F, n[2]))
    csc = np.float32(g_sc) * np.float64(np.float32(scale)) / (S if ragged else 1.0)
    c_diff = np.where(D > 0, csc / np.where(D > 0, np.sqrt(D * N), 1.0), 0.0)[:, None]
    c_y = (csc * np.sqrt(D) / (N * np.sqrt(N)))[:, None]
    c_log = np.float32(g_mag) * np.float64(np.float32(scale)) / (S * cutoff)
    ox, oy = (xm + 1, ym + 1) if a_w else (xm, ym)
    sg = np.sign(dl) * c_log
    e = ym - xm
    dm = {"x": (-c_diff * e - sg / ox, np.abs(c_diff) * (ym + xm) + np.abs(c_log) / ox),
          "y": (c_diff * e - c_y * ym + sg / oy, np.abs(c_diff) * (ym + xm) + np.abs(c_y) * ym + np.abs(c_log) / oy)}
    f = lambda a: np.nan_to_num(a.astype(np.float64))             # noqa: E731
    for name, got, s, m in (("x", gx, sx, xm), ("y", gy, sy, ym)):
        assert not got[~valid].any() and not got[:, 2 * cutoff:].any() and np.isfinite(got).all()
        re, im = f(s[:, :cutoff]), f(s[:, cutoff:2 * cutoff])
        passes = (re * re + im * im >= K.CLAMP) & valid[:, None]
        below = ~passes & valid[:, None]
        assert below.any() == (name == "x") and not got[:, :cutoff][below].any() and not got[:, cutoff:2 * cutoff][below].any()
        worst = 0.0
        for comp, col0 in ((re, 0), (im, cutoff)):
            want = dm[name][0] * comp / m * passes
            bar = 16 * 2.0 ** -24 * dm[name][1] * np.abs(comp) / m
            err = np.abs(got[:, col0:col0 + cutoff] - want)
            assert (err[passes] <= bar[passes]).all(), (name, float((err[passes] / np.maximum(bar[passes], 1e-300)).max()))
            worst = max(worst, float((err[passes] / np.maximum(bar[passes], 1e-300)).max()))
        print(f"bwd d{name} cutoff {cutoff}: worst measured / bar {worst:.3f}")
