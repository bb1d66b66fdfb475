"""The frame-shift origin and the column origins of the row-major weight-gradient kernels (radmmm_wgrad_rmh_shift on one f16
product, radmmm_wgrad_rm_shift on three; csrc/wgrad_rm8.hip, csrc/wgrad_rm.hip) and the grouped split pass that feeds them
(radmmm_split_f16_groups): an LSTM's recurrent weight gradients dW_hh[d] = dG_d^T h_prev read h_prev[f] = y[f -+ 1] out of y
itself.  Everything is checked against the plain entry points on an h_prev built by hand, bit for bit."""
import ctypes
import os

import pytest
import torch

from conftest import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rad_mmm_amd", "libradmmm_hip.so")
DEV = "cuda:0"
SG = 32.0


def test_shift_entry_points_validate_without_gpu():
    """Null pointers, bad pitches, bad column origins and a shift0 beyond the limit return -1 with the entry point's own error
    text before any HIP call; the dims cases pass dummy non-null addresses, which that path never dereferences.  The limit is
    the 32-bit offset arithmetic's, (R + 96 + |shift0| + (taps / 2) * dil) * ldx * 2 < 2^31 (the mask rule holds for any
    shift): with R = 64 and ldx = 64 the first shift0 refused is 16 777 056, sixteen frames earlier under a 5-tap dil-8 conv."""
    lib = ctypes.CDLL(LIB)
    lib.radmmm_last_error.restype = ctypes.c_char_p
    p, i, f, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int64
    lib.radmmm_wgrad_rmh_shift.argtypes = [p, i, i, p, i, i, i, i, i, p, i, p, i, i64, i, i, i, i, i, f, p]
    lib.radmmm_wgrad_rm_shift.argtypes = [p, p, i, i, p, p, i, i, i, i, i, p, i, p, i, i64, i, i, i, i, i, f, p]
    lib.radmmm_wgrad_rmh.argtypes = [p, i, p, i, i, i, p, i, p, i, i64, i, i, i, i, i, f, p]
    lib.radmmm_split_f16_groups.argtypes = [p, i, p, p, i, i, i, i, i, f, p, p]
    d = 0x1000                                                   # never dereferenced

    def rmh(gy=d, x=d, P=d, ldg=128, g0=0, ldx=64, x0=0, s0=-1, B=2, T=32, Mc=64, Nc=32, taps=1, dil=1, splits=1):
        return lib.radmmm_wgrad_rmh_shift(gy, ldg, g0, x, ldx, x0, s0, B * T, T, None, 0, P, Nc, Mc * Nc, Mc, Nc, taps, dil, splits,
                                          1.0, None)

    def rm(gy=d, gl=d, x=d, xl=d, P=d, ldg=128, g0=0, ldx=64, x0=0, s0=-1, B=2, T=32, Mc=64, Nc=32, taps=1, dil=1, splits=1):
        return lib.radmmm_wgrad_rm_shift(gy, gl, ldg, g0, x, xl, ldx, x0, s0, B * T, T, None, 0, P, Nc, Mc * Nc, Mc, Nc, taps, dil,
                                         splits, 1.0, None)

    for fn, name, nulls in ((rmh, b"wgrad_rmh_shift", ("gy", "x", "P")), (rm, b"wgrad_rm_shift", ("gy", "gl", "x", "xl", "P"))):
        for k in nulls:
            assert fn(**{k: None}) == -1
            assert name + b": null pointer" in lib.radmmm_last_error()
        for kw in (dict(T=31), dict(ldg=60), dict(ldx=20), dict(splits=0), dict(Mc=0)):
            assert fn(**kw) == -1
            assert name + b": bad dims" in lib.radmmm_last_error(), kw
        for kw in (dict(g0=4), dict(x0=-8), dict(g0=72), dict(x0=40), dict(g0=64, Mc=72)):
            assert fn(**kw) == -1
            assert name + b": bad column origin" in lib.radmmm_last_error(), kw
        for kw in (dict(s0=16777056), dict(s0=-16777056), dict(s0=16777040, taps=5, dil=8), dict(s0=2 ** 31 - 1), dict(s0=-(2 ** 31))):
            assert fn(**kw) == -1
            assert name + b": shift0 out of range" in lib.radmmm_last_error(), kw
        assert fn(gy=d + 8) == -1
        assert name + b": 16-byte aligned operands" in lib.radmmm_last_error()
    assert rmh(ldg=72, Mc=64) == -1 and b"bad dims" in lib.radmmm_last_error()         # one product: pitches are multiples of 32
    # the plain entry point keeps its name in its texts
    assert lib.radmmm_wgrad_rmh(None, 64, d, 64, 64, 32, None, 0, d, 64, 64 * 64, 64, 64, 1, 1, 1, 1.0, None) == -1
    assert b"wgrad_rmh: null pointer" in lib.radmmm_last_error()

    def groups(x=d, hi=d, lo=d, ld=64, ldh=64, rows=4, gcols=20, n=2, gpitch=32):
        return lib.radmmm_split_f16_groups(x, ld, hi, lo, ldh, rows, gcols, n, gpitch, 1.0, None, None)

    for kw in (dict(x=None), dict(hi=None)):
        assert groups(**kw) == -1
        assert b"split_f16_groups: null pointer" in lib.radmmm_last_error()
    for kw in (dict(gpitch=16), dict(gpitch=36), dict(ldh=56), dict(ld=39), dict(rows=0), dict(n=3)):
        assert groups(**kw) == -1
        assert b"split_f16_groups: bad dims" in lib.radmmm_last_error(), kw
    assert groups(hi=d + 8) == -1 and b"16-byte aligned planes" in lib.radmmm_last_error()


def _lens(B, T):
    """ragged lengths with a full utterance, a length of 1 (B >= 2) and odd ones"""
    return ([T - 3] if B == 1 else [T, 1] + [max(1, T - 7 * b) for b in range(2, B)])[:B]


def _operands(B, T, H, seed):
    """dG [R, 8H] (both directions' gate gradients) and y [R, 2H] as an LSTM leaves them, with their split planes: dG's pair at
    pitch 8H, y's pair with one column group per direction (radmmm_split_f16_groups)."""
    from rad_mmm_amd import ops
    g = torch.Generator().manual_seed(seed)
    R = B * T
    gy = (torch.randn(R, 8 * H, generator=g) * 0.3).to(DEV)
    y = torch.tanh(torch.randn(R, 2 * H, generator=g)).to(DEV)
    gh, gl = ops.split_f16(gy, 8 * H, SG, 8 * H)
    yh, yl = ops.split_f16_groups(y, H, 2)
    return gy, y, (gh, gl), (yh, yl)


def _h_prev(y, B, T, H, d, s, lens):
    """h_prev of direction d by hand: y's column group d moved by s frames inside each utterance, zero where the source frame
    f + s lies outside [0, T) or, with lens, at or beyond the utterance's length."""
    y3 = y.view(B, T, -1)[:, :, d * H:(d + 1) * H]
    hp = torch.zeros_like(y3)
    if s < 0:
        hp[:, -s:] = y3[:, :s]
    elif s > 0:
        hp[:, :-s] = y3[:, s:]
    else:
        hp.copy_(y3)
    if lens is not None:
        src = torch.arange(T, device=y.device)[None] + s
        hp = torch.where((src < lens[:, None])[:, :, None], hp, torch.zeros_like(hp))
    return hp.reshape(B * T, -1).contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("H", [24, 36, 524])          # (Mc, Nc) = (4H, H): 96 x 24, 144 x 36 and the context LSTM's 2096 x 524
@pytest.mark.parametrize("B,T", [(1, 32), (3, 40), (2, 77), (4, 64)])
def test_shifted_launch_equals_plain_launch_on_h_prev(B, T, H):
    """Both kernels, shift0 = -1 / +1, with and without ragged lengths (one of them 1), every pair of column origins
    g_col0 in {0, 4H} x x_col0 in {0, padded H}: the slabs of the shifted launch on y's planes are torch.equal to the slabs of
    the PLAIN entry point on operands of their own -- dG's column block copied out, h_prev built by hand and split.  (B, T):
    one K step; an utterance boundary inside a 32-frame window; T no multiple of 32.  H = 524 has partial last tiles in both
    dimensions and the 544-column groups.  shift0 = 0 on zero origins is the plain entry point, bit for bit.
    One product also against float64: 3e-6 of the largest element against the contraction of the dequantised hi planes, and
    elementwise within 2^-10 |dG|^T |h_prev| + 3e-6 max |ref| of the contraction of the fp32 tensors (the bars of
    test_wgrad_one_pass.py's kernel test); three products 3e-6 against the contraction of hi + lo (test_hip_h3probe.py)."""
    from rad_mmm_amd import ops
    Mc, Nc, R = 4 * H, H, B * T
    gy, y, (gh, gl), (yh, yl) = _operands(B, T, H, 1000 * B + T + H)
    Hg = yh.shape[1] // 2
    assert Hg % 32 == 0 and Hg >= H and yh.shape[1] == 2 * Hg and (H != 524 or Hg == 544)
    ldg1 = ops.round_up(Mc, 32)
    lens_t = torch.tensor(_lens(B, T), dtype=torch.int32, device=DEV)
    # shift0 = 0, zero origins: the plain entry points
    assert torch.equal(ops.wgrad_rmh_shift_slabs(gh, 0, yh, 0, 0, B, T, Mc, Nc, 1.0 / SG),
                       ops.wgrad_rmh_slabs(gh, yh, B, T, Mc, Nc, 1, 1, 1.0 / SG))
    assert torch.equal(ops.wgrad_rm_shift_slabs((gh, gl), 0, (yh, yl), 0, 0, B, T, Mc, Nc, 1.0 / SG, lens_t),
                       ops.wgrad_rm_slabs((gh, gl), (yh, yl), B, T, Mc, Nc, 1, 1, 1.0 / SG, lens_t))
    worst = {"hi": 0.0, "used": 0.0, "three": 0.0}
    for gd in (0, 1):                                            # dG's column block: g_col0 = gd * 4H
        g1h, g1l = (torch.zeros(R, ldg1, device=DEV, dtype=torch.float16) for _ in range(2))
        g1h[:, :Mc], g1l[:, :Mc] = gh[:, gd * Mc:(gd + 1) * Mc], gl[:, gd * Mc:(gd + 1) * Mc]
        for xd in (0, 1):                                        # y's column group: x_col0 = xd * Hg
            for s in (-1, 1):
                for lens in (None, lens_t):
                    hp = _h_prev(y, B, T, H, xd, s, lens)
                    hph, hpl = ops.split_f16(hp, H, 1.0, ops.round_up(H, 32))
                    P1 = ops.wgrad_rmh_shift_slabs(gh, gd * Mc, yh, xd * Hg, s, B, T, Mc, Nc, 1.0 / SG, lens)
                    assert torch.equal(P1, ops.wgrad_rmh_slabs(g1h, hph, B, T, Mc, Nc, 1, 1, 1.0 / SG)), (gd, xd, s, lens is None)
                    P3 = ops.wgrad_rm_shift_slabs((gh, gl), gd * Mc, (yh, yl), xd * Hg, s, B, T, Mc, Nc, 1.0 / SG, lens)
                    assert torch.equal(P3, ops.wgrad_rm_slabs((g1h, g1l), (hph, hpl), B, T, Mc, Nc, 1, 1, 1.0 / SG)), (gd, xd, s, lens is None)
                    if gd != xd:
                        continue                                 # float64: the pairs an LSTM uses
                    gq = g1h.double()[:, :Mc] / SG
                    ref_hi = gq.t() @ hph.double()[:, :Nc]
                    worst["hi"] = max(worst["hi"], rel_err(P1.sum(0)[0].double().cpu(), ref_hi.cpu()))
                    gv = gy.double()[:, gd * Mc:(gd + 1) * Mc]
                    ref = gv.t() @ hp.double()
                    bound = 2.0 ** -10 * (gv.abs().t() @ hp.double().abs()) + 3e-6 * ref.abs().max()
                    worst["used"] = max(worst["used"], float(((P1.sum(0)[0].double() - ref).abs() / bound).max()))
                    ref3 = ((g1h.double() + g1l.double())[:, :Mc] / SG).t() @ (hph.double() + hpl.double())[:, :Nc]
                    worst["three"] = max(worst["three"], rel_err(P3.sum(0)[0].double().cpu(), ref3.cpu()))
    print(f"wgrad shift B={B} T={T} {Mc}x{Nc}: one product vs hi planes {worst['hi']:.2e}, largest |P - ref| / bound "
          f"{worst['used']:.3f}; three products vs hi + lo {worst['three']:.2e}")
    assert worst["hi"] < 3e-6 and worst["used"] <= 1.0 and worst["three"] < 3e-6


@pytest.mark.gpu
@pytest.mark.parametrize("H", [36, 524])
def test_nothing_beyond_the_planes_is_read(H):
    """The operands in allocations of exactly their size against the same operands inside larger buffers whose every other
    element is NaN, in front and behind: equal results, both kernels, both directions (g_col0 = 4H with column tiles that
    reach past 8H is the case an offset base pointer used to carry beyond the tensor).  A read outside the planes would have
    to land in an accumulator that is stored to show here; what cannot show is covered by the entry points' contract (the
    buffer resources span the planes, the column test counts the origin)."""
    from rad_mmm_amd import ops
    B, T = 2, 77
    Mc, Nc = 4 * H, H
    _, _, (gh, gl), (yh, yl) = _operands(B, T, H, 77 + H)
    Hg = yh.shape[1] // 2

    def framed(t):
        pad = 4096                                               # halves: keeps the 16-byte alignment
        buf = torch.full((pad + t.numel() + pad,), float("nan"), device=DEV, dtype=torch.float16)
        buf[pad:pad + t.numel()] = t.reshape(-1)
        return buf[pad:pad + t.numel()].view(t.shape)

    exact = [t.clone() for t in (gh, gl, yh, yl)]                # allocations of exactly the planes' size
    fr = [framed(t) for t in (gh, gl, yh, yl)]
    assert all(torch.equal(a, b) and b.is_contiguous() for a, b in zip(exact, fr))
    for d, s in ((0, -1), (1, 1)):
        a1 = ops.wgrad_rmh_shift_slabs(exact[0], d * Mc, exact[2], d * Hg, s, B, T, Mc, Nc, 1.0 / SG)
        b1 = ops.wgrad_rmh_shift_slabs(fr[0], d * Mc, fr[2], d * Hg, s, B, T, Mc, Nc, 1.0 / SG)
        a3 = ops.wgrad_rm_shift_slabs((exact[0], exact[1]), d * Mc, (exact[2], exact[3]), d * Hg, s, B, T, Mc, Nc, 1.0 / SG)
        b3 = ops.wgrad_rm_shift_slabs((fr[0], fr[1]), d * Mc, (fr[2], fr[3]), d * Hg, s, B, T, Mc, Nc, 1.0 / SG)
        assert torch.isfinite(b1).all() and torch.isfinite(b3).all()
        assert torch.equal(a1, b1) and torch.equal(a3, b3)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,H,groups", [(5, 24, 2), (77, 36, 2), (33, 524, 2), (9, 50, 3), (64, 4192, 1)])
def test_split_f16_groups_has_the_bits_of_split_f16(rows, H, groups):
    """Every column group equals radmmm_split_f16 of that group's columns (hi and lo), every other column of the planes is
    zero, with_lo=False gives the same hi plane, and the saturation flag rises exactly when a scaled value passes 60000
    (H = 50: groups whose rows are not 16-byte aligned in x take the scalar path)."""
    from rad_mmm_amd import ops
    g = torch.Generator().manual_seed(rows + H)
    x = torch.randn(rows, groups * H + (3 if H % 4 else 4), generator=g).to(DEV)[:, :groups * H]      # (a pitch of its own)
    hi, lo = ops.split_f16_groups(x, H, groups, 3.0)
    gp = hi.shape[1] // groups
    assert gp == ops.round_up(H, 32) and hi.shape == lo.shape == (rows, groups * gp)
    for k in range(groups):
        rh, rl = ops.split_f16(x[:, k * H:(k + 1) * H].contiguous(), H, 3.0, gp)
        assert torch.equal(hi[:, k * gp:(k + 1) * gp], rh) and torch.equal(lo[:, k * gp:(k + 1) * gp], rl)
        assert not hi[:, k * gp + H:(k + 1) * gp].any() and not lo[:, k * gp + H:(k + 1) * gp].any()
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    hi1, none = ops.split_f16_groups(x, H, groups, 3.0, with_lo=False, sat_flag=flag)
    assert none is None and torch.equal(hi1, hi) and int(flag) == 0
    ops.split_f16_groups(x, H, groups, 60000.0 / float(x.abs().max()) * 1.01, sat_flag=flag)
    assert int(flag) & 1
