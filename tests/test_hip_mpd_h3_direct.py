"""The producers of the multi-period discriminator's precision "h3" (csrc/mpd_h3.hip; include/radmmm_hip.h), each alone
through the C ABI.

The fp16 pair of every producer is held BIT FOR BIT to the host model of the split formats, tests/_split_ref.py (which
tests/test_split_ref_cpu.py holds to the header), applied to the fp32 value the pass forms.  That value itself is modelled in
numpy float32 where the pass only moves, adds and multiplies by 1 or the slope (repad, frame, unframe: bit for bit), and in
float64 with a rounding bound where it multiplies and adds (conv_post_dgrad: three products per element, which the compiler
may fuse), and it is compared with the fp32 twin kernel's output, which the header promises bit for bit.

Shapes: S in {1, 3} sequences, H in {1, 2, 33} rows, C in {32, 96} channels, stride in {1, 3}, pitches larger than the
columns.  NaN lies in every row and column a kernel must not read (the columns of Z behind C, the pad rows of `add` and of
the saved map, one block behind every input); every output starts as a sentinel, has one more row than the kernel may write
and columns behind the matrix, and all of those must keep the sentinel; the pad rows of the padded outputs and the rows up
to rows_pad must come back as zeros.  The saturation word is raised exactly when the model clamps (cases with and without
one element beyond 60000 / scale)."""
import numpy as np
import pytest
import torch

import _split_ref as SR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SLOPE = np.float32(0.1)
SCALE = 64.0
ROWS_PAD = 32
SHAPES = [(S, H, C) for S in (1, 3) for H in (1, 2, 33) for C in (32, 96)]
STRIDES = (1, 3)


def _lib():
    from rad_mmm_amd._lib import check, lib, ptr, stream
    return check, lib, ptr, stream


def _with_nan_tail(a):
    """device copy with one more leading block of NaN behind it: what lies past the last block must not be read"""
    t = torch.full((a.shape[0] + 1, *a.shape[1:]), float("nan"), device=DEV)
    t[:-1] = torch.as_tensor(a)
    return t


def _pair(rows, ld):
    """two half arrays of rows + 1 rows filled with the sentinel pattern"""
    mk = lambda: torch.full((rows + 1, ld), SR.FILL16, dtype=torch.int16, device=DEV)
    return mk(), mk()


def _check_pair(what, pair, value, rows, cols, scale):
    """pair rows [0, value.shape[0]) = the model's split of value, rows up to `rows` zero, the extra row and the columns from
    `cols` on untouched -> the model's amax"""
    want = SR.split_ref(torch.as_tensor(np.ascontiguousarray(value, dtype=np.float32)), scale)
    n = value.shape[0]
    for name, got, w in (("hi", pair[0], want.hi), ("lo", pair[1], want.lo)):
        got = got.cpu()
        assert torch.equal(got[:n, :cols], w.view(torch.int16)), f"{what}: {name} differs from the host model"
        assert bool((got[n:rows, :cols] == 0).all()), f"{what}: {name} rows up to rows_pad must be zeros"
        assert bool((got[rows:] == SR.FILL16).all()) and bool((got[:, cols:] == SR.FILL16).all()), f"{what}: {name} written out of bounds"
    return want.amax


def _check_flag(what, flag, amax):
    assert int(flag.item()) == (1 if amax > SR.F16_CLAMP else 0), (what, int(flag.item()), amax)


def _maybe_clamp(a, clamp, scale=SCALE):
    """one element just beyond the fp16 clamp (in the last row: a tail wave sees it), or none"""
    if clamp:
        a.reshape(-1)[-3] = np.float32(61000.0 / scale)
    return a


def _lrelu(v):
    return np.where(v > 0, v, SLOPE * v).astype(np.float32)


@pytest.mark.parametrize("clamp", (False, True), ids=("plain", "clamps"))
@pytest.mark.parametrize("S,H,C", SHAPES)
def test_repad(S, H, C, clamp):
    check, lib, ptr, stream = _lib()
    rng = np.random.RandomState(S * 1000 + H * 10 + C)
    ldz = C + 4
    Z = np.full((S * H, ldz), np.nan, np.float32)
    Z[:, :C] = _maybe_clamp(rng.randn(S * H, C).astype(np.float32) * 3, clamp)
    Zd = _with_nan_tail(Z)
    X = torch.full((S + 1, H + 4, C), 7.0, device=DEV)
    twin = torch.full((S, H + 4, C), 7.0, device=DEV)
    pair = _pair(S * (H + 4), C)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    check(lib.radmmm_mpdh3_repad(ptr(Zd), ldz, ptr(X), ptr(pair[0]), ptr(pair[1]), S, H, C, float(SLOPE), SCALE, ptr(flag), stream()),
          "mpdh3_repad")
    check(lib.radmmm_mpd_repad(ptr(Zd), ldz, ptr(twin), S, H, C, float(SLOPE), stream()), "mpd_repad")
    want = np.zeros((S, H + 4, C), np.float32)
    want[:, 2:2 + H] = _lrelu(Z[:, :C]).reshape(S, H, C)
    got = X.cpu().numpy()
    assert np.array_equal(got[:S].view(np.int32), want.view(np.int32)) and (got[S] == 7.0).all()
    assert torch.equal(X[:S], twin)
    amax = _check_pair("repad", pair, want.reshape(S * (H + 4), C), S * (H + 4), C, SCALE)
    _check_flag("repad", flag, amax)
    assert (amax > SR.F16_CLAMP) == clamp


@pytest.mark.parametrize("clamp", (False, True), ids=("plain", "clamps"))
@pytest.mark.parametrize("st", STRIDES)
@pytest.mark.parametrize("S,H,C", SHAPES)
def test_frame(S, H, C, st, clamp):
    check, lib, ptr, stream = _lib()
    rng = np.random.RandomState(S * 1000 + H * 10 + C + st)
    Ho = (H - 1) // st + 1
    X = _maybe_clamp(rng.randn(S, H + 4, C).astype(np.float32) * 3, clamp and st * (Ho - 1) + 5 == H + 4)
    if clamp and st * (Ho - 1) + 5 != H + 4:                      # the last rows lie in no window: plant it in row 0 instead
        X[-1, 0, 5] = np.float32(61000.0 / SCALE)
    rows, ldf = S * Ho, 5 * C + 8
    rows_tot = max(rows, ROWS_PAD)
    pair = _pair(rows_tot, ldf)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    check(lib.radmmm_mpdh3_frame(ptr(_with_nan_tail(X)), ptr(pair[0]), ptr(pair[1]), ldf, S, H, C, Ho, st, ROWS_PAD, SCALE, ptr(flag),
                                 stream()), "mpdh3_frame")
    want = np.stack([X[s].reshape(-1)[st * h * C: st * h * C + 5 * C] for s in range(S) for h in range(Ho)])
    amax = _check_pair("frame", pair, want, rows_tot, 5 * C, SCALE)
    _check_flag("frame", flag, amax)
    assert (amax > SR.F16_CLAMP) == clamp


def _unframe_inputs(S, H, C, st, seed):
    rng = np.random.RandomState(seed)
    Ho = (H - 1) // st + 1
    dF = rng.randn(S * Ho, 5 * C).astype(np.float32)
    add = np.full((S, H + 4, C), np.nan, np.float32)
    add[:, 2:2 + H] = rng.randn(S, H, C).astype(np.float32)
    X = np.full((S, H + 4, C), np.nan, np.float32)
    X[:, 2:2 + H] = rng.randn(S, H, C).astype(np.float32)
    X[0, 2, :4] = (0.0, -0.0, 1e-30, -1e-30)                      # the derivative at and next to the kink: x > 0 ? 1 : slope
    return Ho, dF, add, X


def _unframe_model(dF, add, X, S, H, C, Ho, st):
    """float32, the kernel's order: the windows ascending, then add, then the derivative -> dense [S * H][C]"""
    dF = dF.reshape(S, Ho, 5, C)
    out = np.zeros((S, H, C), np.float32)
    for h in range(H):
        u = h + 2
        g = np.zeros((S, C), np.float32)
        for h1 in range(Ho):
            if st * h1 <= u <= st * h1 + 4:
                g = g + dF[:, h1, u - st * h1]
        if add is not None:
            g = g + add[:, u]
        out[:, h] = g * np.where(X[:, u] > 0, np.float32(1), SLOPE)
    return out.reshape(S * H, C)


@pytest.mark.parametrize("clamp", (False, True), ids=("plain", "clamps"))
@pytest.mark.parametrize("st", STRIDES)
@pytest.mark.parametrize("S,H,C", SHAPES)
def test_unframe(S, H, C, st, clamp):
    check, lib, ptr, stream = _lib()
    Ho, dF, add, X = _unframe_inputs(S, H, C, st, S * 1000 + H * 10 + C + st)
    scale = 2.0 ** 16 if clamp else 2.0 ** 8                       # a value of 1 already clamps at 2^16; sums of a few N(0, 1) do not at 2^8
    rows, ldh = S * H, C + 8
    rows_tot = max(rows, ROWS_PAD)
    dFd, addd, Xd = _with_nan_tail(dF), _with_nan_tail(add), _with_nan_tail(X)
    for with_add in (True, False):
        want = _unframe_model(dF, add if with_add else None, X, S, H, C, Ho, st)
        for with_dz in (True, False):
            dZ = torch.full((rows + 1, C), 7.0, device=DEV)
            twin = torch.empty(rows, C, device=DEV)
            pair = _pair(rows_tot, ldh)
            flag = torch.zeros(1, dtype=torch.int32, device=DEV)
            check(lib.radmmm_mpdh3_unframe(ptr(dFd), ptr(addd) if with_add else None, ptr(Xd), ptr(dZ) if with_dz else None,
                                           ptr(pair[0]), ptr(pair[1]), ldh, S, H, C, Ho, st, float(SLOPE), ROWS_PAD, scale, ptr(flag),
                                           stream()), "mpdh3_unframe")
            if with_dz:
                check(lib.radmmm_mpd_unframe(ptr(dFd), ptr(addd) if with_add else None, ptr(Xd), ptr(twin), S, H, C, Ho, st,
                                             float(SLOPE), stream()), "mpd_unframe")
                got = dZ.cpu().numpy()
                assert np.array_equal(got[:rows].view(np.int32), want.view(np.int32)) and (got[rows] == 7.0).all()
                assert torch.equal(dZ[:rows], twin)
            else:
                assert bool((dZ == 7.0).all())
            amax = _check_pair("unframe", pair, want, rows_tot, C, scale)
            _check_flag("unframe", flag, amax)
    if clamp:
        assert amax > SR.F16_CLAMP


@pytest.mark.parametrize("clamp", (False, True), ids=("plain", "clamps"))
@pytest.mark.parametrize("S,H,C", SHAPES)
def test_conv_post_dgrad(S, H, C, clamp):
    """S = 1 * p sequences of one signal row: dOut [1][H][p]"""
    check, lib, ptr, stream = _lib()
    rng = np.random.RandomState(S * 1000 + H * 10 + C)
    p = S
    dOut = rng.randn(1, H, p).astype(np.float32)
    W = rng.randn(3, C).astype(np.float32)
    _, _, add, X = _unframe_inputs(S, H, C, 1, S + H + C)
    scale = 2.0 ** 16 if clamp else 2.0 ** 8
    rows, ldh = S * H, C + 8
    rows_tot = max(rows, ROWS_PAD)
    # float64: dZ[s][h][c] = (sum_k dOut[h + 1 - k][w = s] W[k][c] + add) * lrelu'(X)
    g = np.zeros((S, H, C))
    mag = np.zeros((S, H, C))
    for k in range(3):
        for h in range(H):
            if 0 <= h + 1 - k < H:
                t = dOut[0, h + 1 - k, :, None].astype(np.float64) * W[k][None, :]
                g[:, h] += t
                mag[:, h] += np.abs(t)
    g += add[:, 2:2 + H]
    mag += np.abs(add[:, 2:2 + H])
    d = np.where(X[:, 2:2 + H] > 0, 1.0, float(SLOPE))
    want64, bound = (g * d).reshape(rows, C), (6 * 2.0 ** -24 * mag * d).reshape(rows, C)
    dOd, Wd, addd, Xd = _with_nan_tail(dOut), _with_nan_tail(W), _with_nan_tail(add), _with_nan_tail(X)
    ref_pair = None
    for with_dz in (True, False):
        dZ = torch.full((rows + 1, C), 7.0, device=DEV)
        twin = torch.empty(rows, C, device=DEV)
        pair = _pair(rows_tot, ldh)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        check(lib.radmmm_mpdh3_conv_post_dgrad(ptr(dOd), ptr(Wd), ptr(addd), ptr(Xd), ptr(dZ) if with_dz else None, ptr(pair[0]),
                                               ptr(pair[1]), ldh, 1, p, H, C, float(SLOPE), ROWS_PAD, scale, ptr(flag), stream()),
              "mpdh3_conv_post_dgrad")
        if with_dz:
            check(lib.radmmm_mpd_conv_post_dgrad(ptr(dOd), ptr(Wd), ptr(addd), ptr(Xd), ptr(twin), 1, p, H, C, float(SLOPE), stream()),
                  "mpd_conv_post_dgrad")
            got = dZ.cpu().numpy()
            assert (np.abs(got[:rows] - want64) <= bound).all() and (got[rows] == 7.0).all()
            assert torch.equal(dZ[:rows], twin)
            amax = _check_pair("conv_post_dgrad", pair, got[:rows], rows_tot, C, scale)
            ref_pair = (pair[0].clone(), pair[1].clone())
        else:
            assert bool((dZ == 7.0).all())
            assert torch.equal(pair[0], ref_pair[0]) and torch.equal(pair[1], ref_pair[1])
        _check_flag("conv_post_dgrad", flag, amax)
    if clamp:
        assert amax > SR.F16_CLAMP


def test_bad_arguments_return_before_any_launch():
    _, lib, _, _ = _lib()
    a = 0x10000                                                   # never dereferenced
    err = lambda: lib.radmmm_last_error().decode()
    assert lib.radmmm_mpdh3_repad(a, 36, a, a, a, 3, 2, 36, 0.1, 1.0, None, None) == -1 and "multiple of 8" in err()
    assert lib.radmmm_mpdh3_repad(a, 32, a, None, a, 3, 2, 32, 0.1, 1.0, None, None) == -1 and "pair" in err()
    assert lib.radmmm_mpdh3_repad(a, 32, a, a, a, 3, 2, 32, 0.1, 0.0, None, None) == -1 and "scale" in err()
    assert lib.radmmm_mpdh3_frame(a, a, a, 160, 4, 7, 32, 4, 3, 32, 1.0, None, None) == -1 and "leave the" in err()
    assert lib.radmmm_mpdh3_frame(a, a, a, 152, 4, 7, 32, 3, 3, 32, 1.0, None, None) == -1 and "pitch" in err()
    assert lib.radmmm_mpdh3_unframe(a, None, a, None, a, a + 2, 32, 4, 7, 32, 3, 3, 0.1, 32, 1.0, None, None) == -1 and "aligned" in err()
    assert lib.radmmm_mpdh3_unframe(None, None, a, None, a, a, 32, 4, 7, 32, 3, 3, 0.1, 32, 1.0, None, None) == -1 and "null" in err()
    assert lib.radmmm_mpdh3_conv_post_dgrad(a, a, None, a, None, a, a, 32, 0, 3, 7, 32, 0.1, 32, 1.0, None, None) == -1 and "bad dims" in err()
    assert lib.radmmm_mpdh3_conv_post_dgrad(a, a, None, a, None, a, a, 24, 2, 3, 7, 32, 0.1, 32, 1.0, None, None) == -1 and "pitch" in err()


@pytest.mark.parametrize("env,family", [({"RADMMM_H3_TILE": "128"}, 1), ({"RADMMM_H3_TILE": "256", "RADMMM_H3W_MB": "4", "RADMMM_ONE": "0"}, 2),
                                        ({"RADMMM_H3_TILE": "256", "RADMMM_H3W_MB": "7"}, 4)], ids=("narrow", "h3d", "one"))
def test_framed_split_gemm_equals_the_gemm_on_explicit_frames(monkeypatch, env, family):
    """radmmm_rowgemm_h3 with a_item_stride (halves) reads the padded pair's windows in place: in each kernel family that
    takes one-tap launches the result has the bits of the same launch on the frame matrix cut out by radmmm_mpdh3_frame.
    S = 5 sequences of 70 rows, stride 3 (24 windows: 120 rows, a partial row tile at every tile height), C = 64 (K = 320:
    ten K steps, an even count as the one-tap kernel wants), N = 96 with a bias."""
    from rad_mmm_amd import ops
    from rad_mmm_amd._lib import h3_kernel_code, rowgemm_h3, rowgemm_h3_last_kernel
    check, lib, ptr, stream = _lib()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    S, H, C, st, N = 5, 70, 64, 3, 96
    Ho = (H - 1) // st + 1
    rng = np.random.RandomState(3)
    X = np.zeros((S, H + 4, C), np.float32)
    X[:, 2:2 + H] = rng.randn(S, H, C)
    Xd = torch.as_tensor(X).to(DEV)
    hi, lo = ops.split_f16(Xd.view(-1, C), C, SCALE, C)
    Fh, Fl = torch.empty(S * Ho, 5 * C, dtype=torch.float16, device=DEV), torch.empty(S * Ho, 5 * C, dtype=torch.float16, device=DEV)
    check(lib.radmmm_mpdh3_frame(ptr(Xd), ptr(Fh), ptr(Fl), 5 * C, S, H, C, Ho, st, 0, SCALE, None, stream()), "mpdh3_frame")
    Wh, Wl = ops.split_f16(torch.as_tensor(rng.randn(N, 5 * C).astype(np.float32) * 0.05).to(DEV), 5 * C, ops.W_SCALE, 5 * C)
    bias = torch.as_tensor(rng.randn(N).astype(np.float32)).to(DEV)
    out = [torch.full((S * Ho + 1, N), 7.0, device=DEV) for _ in range(2)]
    common = dict(Bh=Wh, Bl=Wl, ldb_h=5 * C, ldc=N, M=S * Ho, N=N, K=5 * C, T=Ho, bias=bias, nprod=3, acc_scale=1.0 / (SCALE * ops.W_SCALE))
    rowgemm_h3(Ah=Fh, Al=Fl, lda_h=5 * C, C=out[0], **common)
    plain = rowgemm_h3_last_kernel()
    rowgemm_h3(Ah=hi, Al=lo, lda_h=st * C, a_item_stride=(H + 4) * C, C=out[1], **common)
    assert rowgemm_h3_last_kernel() == plain and plain // 1000 == family, (plain, h3_kernel_code(family, 3, 0, 0))
    assert torch.equal(out[0], out[1]) and bool((out[1][-1] == 7.0).all())
    want = torch.as_tensor(np.stack([X[s].reshape(-1)[st * h * C: st * h * C + 5 * C] for s in range(S) for h in range(Ho)])).double() @ \
        (Wh.double() + Wl.double()).cpu().t() / ops.W_SCALE + bias.cpu().double()
    assert float((out[1][:-1].cpu().double() - want).abs().max()) <= 1e-4
