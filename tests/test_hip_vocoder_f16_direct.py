"""radmmm_voc_conv_f16 (csrc/vocoder_f16.hip) called directly, against the float64 model of its contract
(tests/_vocoder_f16_ref.conv_f16_ref), at every instantiation's edges: one tile plus a remainder, lengths around the tap
reach and around the tile boundary, pitches above C, every epilogue option.

Bars.  With exactly summable operands (small integers, power-of-two scales: every product and partial sum is an integer
below 2^24) the result is exact whatever the summation order, so the output must equal the model bit for bit.  With
realistic values the fp16 products are exact in fp32 and only the n = taps * C additions of the accumulation round, each by
at most 2^-24 of a partial sum that sum |a| |w| bounds: n * 2^-24 * sum |a| |w| covers any order, and the bar is twice that,
n * 2^-23 * sum |a| |w|, plus the epilogue's three roundings (the scale, the bias, the residual: 2^-24 of |v| + |bias| + |add|
each)."""
import numpy as np
import pytest
import torch

from _vocoder_f16_ref import conv_f16_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

WIDTHS = {16: (1, 4), 32: (1, 4), 48: (2, 2), 128: (4, 1), 256: (8, 1)}          # C -> (ntc, mi): the instantiation the case is about
CASES = [(C, k, d) for C in WIDTHS for k, d in ((3, 1), (7, 5), (11, 5), (7, 12))]
PAD = 12345.0                                                        # sentinel of the columns past C


def _geometry(C, taps, dil):
    tm = 128 * WIDTHS[C][1]
    return tm, tm + 37, (taps // 2) * dil


def _launch(C, taps, dil, B, T, X, Wh, bias, lens, add=None, Y2=None, y2_accum=0, Y=None, **scales):
    """asserts the plan's instantiation, launches, asserts the launch took it; -> (Y, Y2) on the host"""
    import rad_mmm_amd._lib as L
    Y = torch.full((B * T, C + 4), PAD, device=DEV) if Y is None else Y
    kw = dict(X=X, ldx=X.shape[1], Wh=Wh, ldw=Wh.shape[2], Y=Y, ldy=Y.shape[1], B=B, T=T, C=C, taps=taps, dil=dil,
              lens=lens, bias=bias, **scales)
    if add is not None:
        kw.update(add=add, ldadd=add.shape[1])
    if Y2 is not None:
        kw.update(Y2=Y2, ldy2=Y2.shape[1], y2_accum=y2_accum)
    want = L.voc_f16_kernel_code(*WIDTHS[C])
    assert L.voc_conv_f16_plan(**kw) == want
    L.voc_conv_f16(**kw)
    assert L.voc_conv_f16_last_kernel() == want
    torch.cuda.synchronize()
    return Y.cpu().numpy(), None if Y2 is None else Y2.cpu().numpy()


def _poison(t, T, lens):
    t = t.clone()
    for b, n in enumerate(lens):
        t[b * T + n:(b + 1) * T] = float("nan")
    return t


@pytest.mark.parametrize("C,taps,dil", CASES)
def test_exactly_summable_operands_bit_for_bit(C, taps, dil):
    tm, T, reach = _geometry(C, taps, dil)
    B = 3
    g = torch.Generator().manual_seed(1000 * C + 10 * taps + dil)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()
    Wh = ri(-3, 3, taps, C, C + 8).half()
    bias = ri(-5, 5, C)
    scales = dict(in_scale=2.0, in_slope=0.5, acc_scale=0.25)
    for n in (reach, reach + 1, tm - 1, tm, tm + 1):
        lens = [T, 1, max(1, n)]
        X = _poison(2.0 * ri(-2, 2, B * T, C + 4), T, lens)          # even: in_scale * in_slope * x stays an integer
        add = _poison(ri(-9, 9, B * T, C + 8), T, lens)
        y2_before = ri(-9, 9, B * T, C + 4)
        ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
        args = (C, taps, dil, B, T, X.to(DEV), Wh.to(DEV), bias.to(DEV), ld)
        ref = conv_f16_ref(X.numpy(), Wh.numpy(), bias.numpy(), B, T, C, taps, dil, lens=lens, add=add.numpy(),
                           Y2=y2_before.numpy(), y2_accum=True, **scales)
        assert np.abs(ref["mag"]).max() * 4 < 2 ** 24 and np.array_equal(ref["y"], np.round(ref["y"] * 4) / 4)
        y, y2 = _launch(*args, add=add.to(DEV), Y2=y2_before.clone().to(DEV), y2_accum=1, **scales)
        assert np.isfinite(y).all() and np.isfinite(y2).all()       # no NaN from at or past a length
        assert np.array_equal(y[:, :C], ref["y"].astype(np.float32)), (n, np.abs(y[:, :C] - ref["y"]).max())
        assert np.array_equal(y2[:, :C], ref["y2"].astype(np.float32))
        assert (y[:, C:] == PAD).all() and np.array_equal(y2[:, C:], y2_before.numpy()[:, C:])   # pad columns untouched
        for b, m in enumerate(lens):
            assert not y[b * T + m:(b + 1) * T, :C].any()            # zeros written at and past the lengths
            assert y[b * T:b * T + m, :C].any()
        ys, y2s = _launch(*args, add=add.to(DEV), Y2=torch.full((B * T, C), 7.0, device=DEV), y2_accum=0, **scales)
        assert np.array_equal(ys, y) and np.array_equal(y2s, y[:, :C])   # the Y2 store; and a repeat launch: the same bits


@pytest.mark.parametrize("C,taps,dil", CASES)
@pytest.mark.parametrize("option", ["plain", "add", "y2", "add_y2_accum"])
def test_realistic_values_within_the_formats_bound(C, taps, dil, option):
    tm, T, reach = _geometry(C, taps, dil)
    B = 3
    lens = [T, 1, tm + 1 if option in ("plain", "y2") else reach + 1]
    g = torch.Generator().manual_seed(7 * C + taps + dil)
    X = _poison(2.0 * torch.randn(B * T, C + 4, generator=g), T, lens)
    Wh = (256.0 * 0.05 * torch.randn(taps, C, C + 8, generator=g)).half()
    bias = 0.1 * torch.randn(C, generator=g)
    add = _poison(torch.randn(B * T, C + 8, generator=g), T, lens) if "add" in option else None
    y2_before = torch.randn(B * T, C + 4, generator=g) if "y2" in option else None
    accum = option == "add_y2_accum"
    scales = dict(in_scale=0.75, in_slope=0.1, acc_scale=1.0 / 256.0)
    ref = conv_f16_ref(X.numpy(), Wh.numpy(), bias.numpy(), B, T, C, taps, dil, lens=lens,
                       add=None if add is None else add.numpy(), Y2=None if y2_before is None else y2_before.numpy(),
                       y2_accum=accum, **scales)
    y, y2 = _launch(C, taps, dil, B, T, X.to(DEV), Wh.to(DEV), bias.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV),
                    add=None if add is None else add.to(DEV), Y2=None if y2_before is None else y2_before.clone().to(DEV),
                    y2_accum=int(accum), **scales)
    n = taps * C
    absadd = 0.0 if add is None else np.nan_to_num(np.abs(add.numpy()[:, :C].astype(np.float64)))
    tol = n * 2.0 ** -23 * ref["mag"] + 3 * 2.0 ** -24 * (ref["mag"] + np.abs(bias.numpy().astype(np.float64)) + absadd)
    err = np.abs(y[:, :C].astype(np.float64) - ref["y"])
    worst = float((err / np.maximum(tol, 1e-300)).max())
    print(f"C {C} taps {taps} dil {dil} {option}: max-abs {err.max():.3e}, worst error / bound {worst:.3f} "
          f"(|y| max {np.abs(ref['y']).max():.2f})")
    assert np.isfinite(y).all() and (err <= tol).all()
    assert (y[:, C:] == PAD).all()
    for b, m in enumerate(lens):
        assert not y[b * T + m:(b + 1) * T, :C].any()
    if y2 is not None:                                              # Y2 = (Y2 +) y, from the y the kernel wrote: one more rounding
        want = y[:, :C].astype(np.float64) + (y2_before.numpy()[:, :C] if accum else 0.0)
        assert (np.abs(y2[:, :C] - want) <= 2.0 ** -24 * np.abs(want)).all()
        assert np.array_equal(y2[:, C:], y2_before.numpy()[:, C:])


@pytest.mark.parametrize("C,taps,dil", [(16, 7, 12), (48, 3, 1), (256, 11, 5)])
def test_null_lens_is_full_length(C, taps, dil):
    tm, T, reach = _geometry(C, taps, dil)
    B = 2
    g = torch.Generator().manual_seed(C)
    X = torch.randint(-3, 4, (B * T, C), generator=g).float()
    Wh = torch.randint(-3, 4, (taps, C, C), generator=g).half()
    bias = torch.randint(-5, 6, (C,), generator=g).float()
    ref = conv_f16_ref(X.numpy(), Wh.numpy(), bias.numpy(), B, T, C, taps, dil, in_slope=0.25)
    y, _ = _launch(C, taps, dil, B, T, X.to(DEV), Wh.to(DEV), bias.to(DEV), None, Y=torch.empty(B * T, C, device=DEV),
                   in_slope=0.25)
    assert np.array_equal(y, ref["y"].astype(np.float32))
    full = torch.full((B,), T, dtype=torch.int32, device=DEV)
    y_full, _ = _launch(C, taps, dil, B, T, X.to(DEV), Wh.to(DEV), bias.to(DEV), full, Y=torch.empty(B * T, C, device=DEV),
                        in_slope=0.25)
    assert np.array_equal(y_full, y)
