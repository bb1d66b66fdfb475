"""The producers of the split operand formats (include/radmmm_hip.h, "split formats") against the host model of
tests/_split_ref.py, bit for bit, at the edges of the formats: fp16 and e4m3 ties, fp16-subnormal hi and lo parts, fp32
subnormal inputs, the lo8 underflow, both clamps, +-0, +-Inf.

Comparisons are on the integer views of the outputs.  Every output buffer has one extra row and starts as the pattern
0x7777; each test asserts what its entry point says about padding (written as zero / left untouched) and that the extra
row is never touched.  The one exclusion: an element whose MODEL value is +-0 may differ from the device in the sign bit
only (fmed3 and t - hi are free to give either zero); _eq counts those elements and lets nothing else through.

The model itself is held to the specification by tests/test_split_ref_cpu.py."""
import pytest
import torch

import _split_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, X8A, X8B = R.SPLIT_F16, R.SPLIT_X8A, R.SPLIT_X8B


def _api():
    from rad_mmm_amd import ops
    from rad_mmm_amd import _lib
    return ops, _lib


def _buf(rows, ld):
    """[rows + 1][ld] halves (as int16) filled with 0x7777: the extra row must come back as it went in"""
    return torch.full((rows + 1, ld), R.FILL16, dtype=torch.int16, device=DEV)


def _fill(rows, ld):
    return torch.full((rows + 1, ld), R.FILL16, dtype=torch.int16)


class ZeroCount:
    """elements computed from an input (not padding) whose model value is +-0 -- the only ones allowed to differ from the
    device, in the sign bit -- as seen by _eq"""
    def __init__(self):
        self.zeros = self.sign_only = 0


def _second(t, fmt):
    """the second array of a pair as its ELEMENTS: int16 halves in the f16 format (the fp16 lo plane), uint8 e4m3 bytes of
    the cross array in the 8-bit formats.  t: an int16 [rows][ld] tensor on the host."""
    assert t.dtype == torch.int16 and not t.is_cuda
    return t if fmt == F16 else t.view(torch.uint8)


def _eq(dev, ref, what, zc=None, cols=None, fmt=None):
    """bitwise equality of two integer tensors, element type by dtype: int16 = fp16 halves, uint8 = e4m3 bytes of a
    cross array (never the bytes of a half).  Where the model ELEMENT is +-0 the device may hold the other zero.
    cols ([ld] bool, default all): the columns that carry input values -- zc counts model zeros only there, so that
    zero padding does not count as an input that is zero (a cross array needs its role fmt to map columns to bytes)."""
    assert dev.shape == ref.shape and dev.dtype == ref.dtype and dev.dtype in (torch.int16, torch.uint8), (what, dev.shape, ref.shape)
    mag = 0x7fff if dev.dtype == torch.int16 else 0x7f
    zero = (ref & mag) == 0
    same = dev == ref
    sign_only = zero & ~same & ((dev & mag) == 0)
    bad = ~(same | sign_only)
    if zc is not None:
        valid = torch.ones(ref.shape[-1], dtype=torch.bool)
        if cols is not None and dev.dtype == torch.int16:
            valid = cols
        elif cols is not None:
            valid = R.pack_cross(cols[None].to(torch.uint8), cols[None].to(torch.uint8), fmt, cols.numel())[0].bool()
        zc.zeros += int((zero & valid).sum())
        zc.sign_only += int((sign_only & valid).sum())
    if bool(bad.any()):
        idx = bad.nonzero()[:8].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} elements differ, first at {idx}: device "
                             f"{[hex(int(dev[tuple(i)]) & 0xffff) for i in idx]} model {[hex(int(ref[tuple(i)]) & 0xffff) for i in idx]}")


def _expect_rows(x, scale, fmt, e, mask=None):
    """model of a [rows][ld] tensor x -> expected (hi, second, lo16) buffers [rows + 1][ld] int16; second is the fp16 lo
    plane as int16 in the f16 format and the cross array as uint8 [rows + 1][2 ld] in the 8-bit formats (_second);
    columns outside `mask` ([ld] bool, default all) and the extra row keep the fill"""
    rows, ld = x.shape
    s = R.split_ref(x, scale, fmt, e)
    m = torch.ones(ld, dtype=torch.bool) if mask is None else mask
    hi, lo = _fill(rows, ld), _fill(rows, ld)
    hi[:rows, m] = s.hi.view(torch.int16)[:, m]
    lo[:rows, m] = s.lo.view(torch.int16)[:, m]
    if fmt == F16:
        return s, hi, lo, lo
    by = _fill(rows, ld).view(torch.uint8)
    bm = R.pack_cross(m[None].to(torch.uint8), m[None].to(torch.uint8), fmt, ld)[0].bool()
    by[:rows, bm] = R.pack_cross(s.hi8, s.lo8, fmt, ld)[:, bm]
    return s, hi, by, lo


# ---------------------------------------------------------------------------------------------------------------------
# a. radmmm_split_f16

def _split_dev(xd, cols, ldh, scale, fmt, e, with_lo16, flag=None):
    _, L = _api()
    rows = xd.shape[0]
    hi, lo = _buf(rows, ldh), _buf(rows, ldh)
    lo16 = _buf(rows, ldh) if with_lo16 else None
    L.check(L.lib.radmmm_split_f16(L.ptr(xd), xd.shape[1], L.ptr(hi), L.ptr(lo), ldh, rows, cols, scale,
                                   L.split_opts(fmt, e, flag, lo16), L.stream()), "split_f16")
    torch.cuda.synchronize()
    return hi.cpu(), _second(lo.cpu(), fmt), (lo16.cpu() if with_lo16 else None)


def _check_split(x, cols, ldh, scale, fmt, e, with_lo16, zc):
    """x [rows][ld >= cols] on the host; the columns >= cols of x hold 1e30 (never to be read)"""
    rows = x.shape[0]
    xp = torch.zeros(rows, ldh)
    xp[:, :cols] = x[:, :cols]
    s, hi_ref, second_ref, lo_ref = _expect_rows(xp, scale, fmt, e)
    hi, second, lo16 = _split_dev(x.to(DEV), cols, ldh, scale, fmt, e, with_lo16)
    tag = f"split_f16 fmt {fmt} e {e} scale {scale} cols {cols} ldh {ldh}"
    inp = torch.arange(ldh) < cols
    _eq(hi, hi_ref, tag + ": hi", zc, inp)
    _eq(second, second_ref, tag + (": lo" if fmt == F16 else ": cross array"), zc, inp, fmt)
    # the padding columns are written as zero: exactly, in every array (the extra row was checked above: still the fill)
    assert not bool(hi[:rows, cols:].any()), tag + ": hi padding"
    if fmt == F16:
        assert not bool(second[:rows, cols:].any()), tag + ": lo padding"
    else:
        pad = torch.zeros(ldh, dtype=torch.uint8)
        pad[cols:] = 1
        pb = R.pack_cross(pad[None], pad[None], fmt, ldh)[0].bool()
        assert not bool(second[:rows, pb].any()), tag + ": cross-array padding"
    if with_lo16:
        if fmt == F16:                       # (the fp16 lo part IS the second array in this format: lo16 is not written)
            assert bool((lo16 == R.FILL16).all()), tag + ": lo16 in the f16 format"
        else:
            _eq(lo16, lo_ref, tag + ": lo16", zc, inp)
            assert not bool(lo16[:rows, cols:].any()), tag + ": lo16 padding"
    return s


@pytest.mark.parametrize("fmt,e", [(F16, 0)] + [(f, e) for f in (X8A, X8B) for e in ("act", "grad", "w", -16, 16)])
def test_split_f16_matches_the_model_bit_for_bit(fmt, e):
    ops, _ = _api()
    e = {"act": ops.X8_ACT_EXP, "grad": ops.X8_GRAD_EXP, "w": ops.X8_W_EXP}.get(e, e)
    zc = ZeroCount()
    n = 0
    for scale in (1.0, 256.0, 2048.0, 2.0 ** -3):
        for cols in (1, 31, 32, 33, 100):
            base = ops.round_up(cols, 8 if fmt == F16 else 32)
            for k, ldh in enumerate((base, base + 32)):
                x = torch.full((3, cols + 3), 1e30)
                x[:, :cols] = R.edge_matrix(3, cols, scale, e, seed=n)
                _check_split(x, cols, ldh, scale, fmt, e, with_lo16=bool(k), zc=zc)
                _check_split(x, cols, ldh, scale, fmt, e, with_lo16=not k, zc=zc)
                n += 1
        # every edge value in a full 4-column group AND in a row tail (cols = 5: columns 0-3 and column 4)
        xr = R.edge_rows(scale, e)
        s = _check_split(xr, 5, 8 if fmt == F16 else 32, scale, fmt, e, with_lo16=True, zc=zc)
        assert bool((s.hi.float()[:, :5].abs() == 60000.0).any())                       # the clamp was reached
        assert bool((xr == 0).any()) and int((s.t[:, :5] == 0).sum()) >= 10              # +-0 inputs, in groups and tails
    assert zc.zeros > 0, "the input columns hold no element whose model value is +-0"
    print(f"fmt {fmt} e {e}: {zc.zeros} model zeros compared, {zc.sign_only} of them with the other sign on the device")


def test_split_f16_grid_stride():
    """4104 x 4128 / 4 = 4 235 328 groups of four: more than the launch's 16384 x 256 threads, so the last rows are
    written in a second grid-stride pass"""
    ops, _ = _api()
    rows, cols, ldh, e = 4104, 4100, 4128, ops.X8_ACT_EXP
    assert rows * (ldh // 4) > 16384 * 256
    x = R.edge_matrix(rows, cols, 1.0, e, seed=3)
    zc = ZeroCount()
    _check_split(x, cols, ldh, 1.0, X8A, e, with_lo16=True, zc=zc)
    assert zc.zeros > 0


# ---------------------------------------------------------------------------------------------------------------------
# b. the saturation word

def _flag_of(xd, cols, ldh, fmt, e, preset=0, scale=1.0, out=None):
    _, L = _api()
    rows = xd.shape[0]
    hi, lo = out if out is not None else (_buf(rows, ldh), _buf(rows, ldh))
    flag = torch.full((1,), preset, dtype=torch.int32, device=DEV)
    L.check(L.lib.radmmm_split_f16(L.ptr(xd), xd.shape[1], L.ptr(hi), L.ptr(lo), ldh, rows, cols, scale,
                                   L.split_opts(fmt, e, flag, None), L.stream()), "split_f16")
    return int(flag.item())


def _sat_magnitudes(e):
    """amax with amax * 2^e / 448 = 2^l (1 +- 2^-10), l = 0 .. 6, and 60000 (1 +- 2^-10): all exact in fp32.  The exact
    boundaries are left out on purpose: the kernel multiplies by the fp32 reciprocal of 448."""
    out = [448.0 * 2.0 ** (l - e) * (1 + sgn * 2.0 ** -10) for l in range(7) for sgn in (-1, 1)]
    return out + [60000.0 * (1 - 2.0 ** -10), 60000.0 * (1 + 2.0 ** -10)]


def _check_word(word, amax, fmt, e, what):
    ops, _ = _api()
    ref = R.flag_ref(amax, fmt, e)
    lv = ops.GradScale._x8_level
    assert word & 3 == ref & 3, (what, amax, hex(word), hex(ref))
    assert (word >> 2).bit_length() == (ref >> 2).bit_length(), (what, amax, hex(word), hex(ref))   # highest level bit, none above
    assert word >> 8 == 0 and lv(word) == lv(ref), (what, amax, hex(word), hex(ref))


@pytest.mark.parametrize("fmt,e", [(X8A, "act"), (X8A, "grad"), (X8B, "w"), (F16, 0)])
def test_saturation_word_by_position_and_level(fmt, e):
    ops, _ = _api()
    e = {"act": ops.X8_ACT_EXP, "grad": ops.X8_GRAD_EXP, "w": ops.X8_W_EXP}.get(e, e)
    rows, cols, ldh = 3, 133, 160                                        # 40 groups per row, 120 threads with work
    g = torch.Generator().manual_seed(7)
    clean = torch.randn(rows, cols, generator=g).to(DEV)
    assert _flag_of(clean, cols, ldh, fmt, e) == 0                       # a clean tensor leaves 0
    assert _flag_of(clean, cols, ldh, fmt, e, preset=0x40) == 0x40       # the word is OR-ed: a preset bit survives
    # group index -> (row, column): first element, lane 63, a lane >= 64 (101), the last valid column with cols % 4 == 1
    c4n = ldh // 4
    spots = {"first": (0, 0), "lane 63": (63 // c4n, 63 % c4n * 4 + 2), "lane 101": (101 // c4n, 101 % c4n * 4 + 1),
             "last column": (rows - 1, cols - 1)}
    assert cols % 4 == 1 and spots["lane 63"] == (1, 94) and spots["lane 101"] == (2, 85)
    for name, (r, c) in spots.items():
        for amax in _sat_magnitudes(e):
            for sgn in (1.0, -1.0):
                x = clean.clone()
                x[r, c] = sgn * amax
                assert float(x[r, c].abs()) == amax                      # exact in fp32
                word = _flag_of(x, cols, ldh, fmt, e)
                if fmt == F16:
                    assert word == (1 if amax > 60000.0 else 0), (name, amax, word)  # the f16 format can only raise bit 0
                else:
                    _check_word(word, amax, fmt, e, name)
                    assert word == R.flag_ref(amax, fmt, e)              # one saturating element: nothing else to report
    x = clean.clone()
    x[1, 7] = 448.0 * 2.0 ** (3 - e) * (1 + 2.0 ** -10)
    w = _flag_of(x, cols, ldh, fmt, e, preset=0x9)
    assert w & 0x9 == 0x9 and (fmt == F16 or _api()[0].GradScale._x8_level(w) == 4)


def test_saturation_word_second_grid_stride_pass():
    """the saturating element sits in a group only the second pass of the grid-stride loop reaches"""
    ops, _ = _api()
    e = ops.X8_ACT_EXP
    rows, cols, ldh = 4104, 4100, 4128
    r, c = 4100, 9
    assert r * (ldh // 4) + c // 4 >= 16384 * 256
    x = torch.full((rows, cols), 0.5, device=DEV)
    out = (_buf(rows, ldh), _buf(rows, ldh))
    assert _flag_of(x, cols, ldh, X8A, e, out=out) == 0
    for amax in _sat_magnitudes(e):
        x[r, c] = -amax
        word = _flag_of(x, cols, ldh, X8A, e, out=out)
        _check_word(word, amax, X8A, e, "second pass")
        assert word == R.flag_ref(amax, X8A, e)


def test_saturation_word_highest_level_wins_across_workgroups():
    ops, _ = _api()
    e = ops.X8_GRAD_EXP
    rows, cols, ldh = 40, 128, 128                                       # 1280 groups: five workgroups of 256 threads
    unit = 448.0 * 2.0 ** -e
    x = torch.full((rows, cols), 1.0, device=DEV)
    x[1, 5] = unit * 3.0                                                 # workgroup 0: level 2
    x[25, 64] = -unit * 20.0                                             # workgroup 3: level 5
    x[39, 127] = unit * 1.5                                              # workgroup 4: level 1
    word = _flag_of(x, cols, ldh, X8A, e)
    _check_word(word, unit * 20.0, X8A, e, "three workgroups")
    assert ops.GradScale._x8_level(word) == 5
    assert (word >> 2) & ~0b10011 == 0                                   # only the levels present can have been reported


# ---------------------------------------------------------------------------------------------------------------------
# c. radmmm_weightnorm_fwd_h3 and _multi

WN_SHAPES = [(5, 150, 1, (77, 80, 0), 160), (4, 64, 5, (0, 0, 0), 64), (3, 36, 3, (0, 0, 0), 64), (6, 7, 1, (0, 0, 0), 32)]


def _perm_cols(Cin, perm):
    ci = torch.arange(Cin)
    return torch.where(ci < perm[0], ci + perm[1], ci - perm[0] + perm[2])


def _wn_layout(w, ldk, perm):
    """w [Cout][Cin][taps] values -> ([taps * Cout][ldk] with w at the permuted columns, [ldk] bool of the columns hit)"""
    Cout, Cin, taps = w.shape
    col = _perm_cols(Cin, perm)
    full = torch.zeros(taps, Cout, ldk, dtype=w.dtype)
    full[:, :, col] = w.permute(2, 0, 1)
    hit = torch.zeros(ldk, dtype=torch.bool)
    hit[col] = True
    return full.reshape(taps * Cout, ldk), hit


def _wn_dev(specs, fmt, multi):
    """specs: [(v, g or None, ldk, perm)] on the host -> [(Wh, Wl bytes, inv_norm or None)] from one launch per tensor or
    from one radmmm_weightnorm_fwd_h3_multi launch for all"""
    ops, L = _api()
    outs, items, keep = [], [], []
    for v, g, ldk, perm in specs:
        Cout, Cin, taps = v.shape
        vd, gd = v.to(DEV), (g.to(DEV) if g is not None else None)
        Wh, Wl = _buf(taps * Cout, ldk), _buf(taps * Cout, ldk)
        inv = torch.full((Cout,), float("nan"), device=DEV) if g is not None else None
        keep.append((vd, gd))
        outs.append((Wh, Wl, inv))
        if multi:
            items.append(L.WnItem(L.ptr(vd), L.ptr(gd), L.ptr(Wh), L.ptr(Wl), L.ptr(inv), Cout, Cin, taps, ldk, *perm))
        else:
            L.check(L.lib.radmmm_weightnorm_fwd_h3(L.ptr(vd), L.ptr(gd), L.ptr(Wh), L.ptr(Wl), L.ptr(inv), Cout, Cin, taps, ldk,
                                                   perm[0], perm[1], perm[2], ops.W_SCALE, L.split_opts(fmt, ops.X8_W_EXP),
                                                   L.stream()), "weightnorm_fwd_h3")
    if multi:
        arr = (L.WnItem * len(items))(*items)
        L.check(L.lib.radmmm_weightnorm_fwd_h3_multi(arr, len(items), ops.W_SCALE, L.split_opts(fmt, ops.X8_W_EXP), L.stream()),
                "weightnorm_fwd_h3_multi")
    torch.cuda.synchronize()
    return [(h.cpu(), _second(l.cpu(), fmt), (i.cpu() if i is not None else None)) for h, l, i in outs]


def _wn_twin(v, g, ldk, perm):
    """the fp32 kernel radmmm_weightnorm_fwd on the same tensor -> (W [taps * Cout][ldk], inv_norm) on the host"""
    _, L = _api()
    Cout, Cin, taps = v.shape
    W = torch.zeros(taps * Cout, ldk, device=DEV)
    inv = torch.empty(Cout, device=DEV)
    vd, gd = v.to(DEV), g.to(DEV)
    L.check(L.lib.radmmm_weightnorm_fwd(L.ptr(vd), L.ptr(gd), L.ptr(W), L.ptr(inv), Cout, Cin, taps, ldk, *perm, L.stream()), "weightnorm_fwd")
    torch.cuda.synchronize()
    return W.cpu(), inv.cpu()


def _edge_weights(Cout, Cin, taps, seed):
    ops, _ = _api()
    pool, _names = R.edge_pool(ops.W_SCALE, ops.X8_W_EXP, seed)
    n = Cout * Cin * taps
    idx = (torch.arange(n) + 17 * seed) % pool.numel()
    return pool[idx].reshape(Cout, Cin, taps).contiguous()


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
@pytest.mark.parametrize("fmt", [F16, X8B])
def test_weightnorm_h3_plain_weights_match_the_model(fmt, multi):
    """g = NULL: the bytes are the model of scale * v rearranged to [tap][co][col(ci)].  (5, 150, 1) with the column
    permutation and (6, 7, 1) take the one-element store path -- the only place it meets the model -- and see the whole
    edge pool; columns the permutation does not hit stay untouched."""
    ops, _ = _api()
    specs = [(_edge_weights(Cout, Cin, taps, k), None, ldk, perm) for k, (Cout, Cin, taps, perm, ldk) in enumerate(WN_SHAPES)]
    assert specs[0][0].numel() >= 2 * R.edge_pool(ops.W_SCALE, ops.X8_W_EXP)[0].numel()
    zc = ZeroCount()
    for (v, _g, ldk, perm), (Wh, Wl, _inv) in zip(specs, _wn_dev(specs, fmt, multi)):
        full, hit = _wn_layout(v, ldk, perm)
        assert int(hit.sum()) == v.shape[1]
        _s, hi_ref, second_ref, _lo = _expect_rows(full, ops.W_SCALE, fmt, ops.X8_W_EXP, mask=hit)
        _eq(Wh, hi_ref, f"weightnorm_fwd_h3 {tuple(v.shape)} fmt {fmt}: hi", zc, hit)
        _eq(Wl, second_ref, f"weightnorm_fwd_h3 {tuple(v.shape)} fmt {fmt}: second array", zc, hit, fmt)
    assert zc.zeros > 0


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
@pytest.mark.parametrize("fmt", [F16, X8B])
def test_weightnorm_h3_exact_norm_rows_match_the_fp32_twin(fmt, multi):
    """v = k / 64 with integer |k| <= 32: the squares sum exactly in any order (below 2^24 units of 2^-12), so this kernel
    and the fp32 kernel radmmm_weightnorm_fwd see the same norm; the bytes must then be the model of scale * W_twin."""
    ops, _ = _api()
    specs = []
    for k, (Cout, Cin, taps, perm, ldk) in enumerate(WN_SHAPES):
        g = torch.Generator().manual_seed(40 + k)
        v = torch.randint(-32, 33, (Cout, Cin, taps), generator=g).float() / 64
        v[:, 0, 0] = 0.5                                                  # (no all-zero row)
        specs.append((v, torch.randn(Cout, generator=g) * 0.7, ldk, perm))
    zc = ZeroCount()
    for (v, gg, ldk, perm), (Wh, Wl, inv) in zip(specs, _wn_dev(specs, fmt, multi)):
        Wt, inv_t = _wn_twin(v, gg, ldk, perm)
        nrm = v.double().flatten(1).norm(dim=1)
        assert rel_err(inv_t.double(), 1 / nrm) <= 3 * 2.0 ** -24
        assert torch.equal(inv, inv_t)
        full, hit = _wn_layout((gg.double()[:, None, None] * v.double() / nrm[:, None, None]), ldk, perm)
        assert bool(((Wt.double() - full).abs()[:, hit] <= 3 * 2.0 ** -24 * full.abs()[:, hit]).all())
        _s, hi_ref, second_ref, _lo = _expect_rows(Wt, ops.W_SCALE, fmt, ops.X8_W_EXP, mask=hit)
        _eq(Wh, hi_ref, f"weightnorm_fwd_h3 {tuple(v.shape)} fmt {fmt}: hi", zc, hit)
        _eq(Wl, second_ref, f"weightnorm_fwd_h3 {tuple(v.shape)} fmt {fmt}: second array", zc, hit, fmt)


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
@pytest.mark.parametrize("fmt", [F16, X8B])
def test_weightnorm_h3_random_rows_within_the_summation_bound(fmt, multi):
    """inv_norm within (n / 2 + 3) 2^-24 of float64 (n = Cin * taps squares summed in any order, halved by the root, plus
    the roundings of the root and the division); the decoded (hi + lo) / scale within that plus the reconstruction
    bound 2^-22 |t| + 2^-25 of g v / ||v||"""
    ops, _ = _api()
    specs = []
    for k, (Cout, Cin, taps, perm, ldk) in enumerate(WN_SHAPES):
        g = torch.Generator().manual_seed(60 + k)
        specs.append((torch.randn(Cout, Cin, taps, generator=g) * 0.05, torch.randn(Cout, generator=g) * 0.7, ldk, perm))
    for (v, gg, ldk, perm), (Wh, Wl, inv) in zip(specs, _wn_dev(specs, fmt, multi)):
        Cout, Cin, taps = v.shape
        n = Cin * taps
        eps = (n / 2 + 3) * 2.0 ** -24
        nrm = v.double().flatten(1).norm(dim=1)
        assert bool(((inv.double() - 1 / nrm).abs() <= eps / nrm).all())
        w, hit = _wn_layout(gg.double()[:, None, None] * v.double() / nrm[:, None, None], ldk, perm)
        hi = Wh[:-1].view(torch.float16).double()
        # columns the permutation does not hit stay untouched, in both arrays
        assert bool((Wh[:, ~hit] == R.FILL16).all())
        if fmt == F16:
            lo = Wl[:-1].view(torch.float16).double()
            assert bool((Wl[:, ~hit] == R.FILL16).all())
        else:
            _h8, l8 = R.unpack_cross(Wl[:-1], fmt, ldk)
            lo = R.e4m3_value(l8).double() * 2.0 ** -(11 + ops.X8_W_EXP)
            hb = R.pack_cross(hit[None].to(torch.uint8), hit[None].to(torch.uint8), fmt, ldk)[0].bool()
            assert bool((Wl[:, ~hb] == R.FILL8).all())
        dec = (hi + lo) / ops.W_SCALE
        t = w.abs() * ops.W_SCALE * (1 + eps)
        # (the 8-bit lo part carries 4 significand bits of the residual instead of 11: 2^-11 - 2^-15 of |t| at the worst)
        recon = (2.0 ** -22 * t + 2.0 ** -25) if fmt == F16 else (2.0 ** -15 * t + 2.0 ** -21)
        bound = eps * w.abs() + recon / ops.W_SCALE
        assert bool(((dec - w).abs()[:, hit] <= bound[:, hit]).all()), float(((dec - w).abs() / bound)[:, hit].max())
        assert bool((Wh[-1] == R.FILL16).all()) and bool((Wl[-1] == (R.FILL16 if fmt == F16 else R.FILL8)).all())


# ---------------------------------------------------------------------------------------------------------------------
# d. radmmm_transpose_f16_pair and _multi

TP_SHAPES = [(1, 4, 4), (3, 33, 31), (1, 64, 64), (3, 100, 36), (1, 68, 132), (2, 65, 64)]


def _tp_source(batches, rows, cols, fmt, seed):
    """a [batches][rows][ld_src] pair written by radmmm_weightnorm_fwd_h3 (g = NULL) from edge-class weights, on the device
    and as read back"""
    ops, L = _api()
    ld_src = ops.round_up(cols, 8 if fmt == F16 else 32)
    v = _edge_weights(rows, cols, batches, seed).to(DEV)
    Wh = torch.zeros(batches * rows, ld_src, dtype=torch.int16, device=DEV)
    Wl = torch.zeros(batches * rows, ld_src, dtype=torch.int16, device=DEV)
    L.check(L.lib.radmmm_weightnorm_fwd_h3(L.ptr(v), None, L.ptr(Wh), L.ptr(Wl), None, rows, cols, batches, ld_src, 0, 0, 0,
                                           ops.W_SCALE, L.split_opts(fmt, ops.X8_W_EXP), L.stream()), "weightnorm_fwd_h3")
    return Wh, Wl, ld_src


def _tp_expect(Wh, Wl, batches, rows, cols, ld_src, ld_dst, fmt):
    """from the source pair's bytes: hi transposed, lo / lo8 moved, hi8 re-derived from the fp16 hi; everything outside
    [cols][rows] -- hi plane and both 32-byte halves of the cross rows -- and the extra row keep the fill.  Returns
    (hi, second) with second as _second gives it."""
    ops, _ = _api()
    sh = Wh.cpu().reshape(batches, rows, ld_src)[:, :, :cols]
    hi_t = sh.transpose(1, 2).reshape(batches * cols, rows)
    hi_ref = _fill(batches * cols, ld_dst)
    hi_ref[:-1, :rows] = hi_t
    if fmt == F16:
        lo_ref = _fill(batches * cols, ld_dst)
        lo_ref[:-1, :rows] = Wl.cpu().reshape(batches, rows, ld_src)[:, :, :cols].transpose(1, 2).reshape(batches * cols, rows)
        return hi_ref, lo_ref
    _h8, l8 = R.unpack_cross(Wl.cpu().view(torch.uint8).reshape(batches, rows, 2 * ld_src), fmt, cols)
    l8_t = l8.transpose(1, 2).reshape(batches * cols, rows)
    h8_t = R.rederived_hi8(hi_t.contiguous().view(torch.float16), ops.X8_W_EXP)
    by = _fill(batches * cols, ld_dst).view(torch.uint8)
    m = torch.zeros(ld_dst, dtype=torch.uint8)
    m[:rows] = 1
    bm = R.pack_cross(m[None], m[None], fmt, ld_dst)[0].bool()
    pad = lambda a: torch.cat([a, torch.zeros(a.shape[0], ld_dst - rows, dtype=torch.uint8)], 1)
    by[:-1, bm] = R.pack_cross(pad(h8_t), pad(l8_t), fmt, ld_dst)[:, bm]
    return hi_ref, by


def _same(dev, ref, what):
    """exact equality, no exclusion: a transposition moves bits (the re-derived hi8 of a -0 hi is the -0 byte in the model
    as on the device)"""
    assert dev.shape == ref.shape and dev.dtype == ref.dtype, (what, dev.shape, ref.shape)
    if not torch.equal(dev, ref):
        idx = (dev != ref).nonzero()[:8].tolist()
        raise AssertionError(f"{what}: {int((dev != ref).sum())} elements differ, first at {idx}: device "
                             f"{[hex(int(dev[tuple(i)]) & 0xffff) for i in idx]} expected {[hex(int(ref[tuple(i)]) & 0xffff) for i in idx]}")


@pytest.mark.parametrize("fmt", [F16, X8B])
@pytest.mark.parametrize("batches,rows,cols", TP_SHAPES)
def test_transpose_pair_moves_the_bytes(batches, rows, cols, fmt):
    ops, L = _api()
    Wh, Wl, ld_src = _tp_source(batches, rows, cols, fmt, seed=rows + cols)
    ld_dst = ops.round_up(rows, 8 if fmt == F16 else 32) + (32 if rows % 32 == 0 else 0)        # always some padding
    Th, Tl = _buf(batches * cols, ld_dst), _buf(batches * cols, ld_dst)
    L.check(L.lib.radmmm_transpose_f16_pair(L.ptr(Wh), L.ptr(Wl), ld_src, rows * ld_src, L.ptr(Th), L.ptr(Tl), ld_dst, cols * ld_dst,
                                            batches, rows, cols, fmt, ops.X8_W_EXP, L.stream()), "transpose_f16_pair")
    torch.cuda.synchronize()
    hi_ref, second_ref = _tp_expect(Wh, Wl, batches, rows, cols, ld_src, ld_dst, fmt)
    _same(Th.cpu(), hi_ref, f"transpose_f16_pair {batches, rows, cols} fmt {fmt}: hi")
    _same(_second(Tl.cpu(), fmt), second_ref, f"transpose_f16_pair {batches, rows, cols} fmt {fmt}: second array")


def test_transpose_pair_multi_mixes_wide_and_narrow_tiles():
    """one launch for all shapes: those with rows and cols multiples of 4 take the 64-wide tile, (3, 33, 31) and
    (2, 65, 64) must take the 32-wide one"""
    ops, L = _api()
    items, keep = [], []
    for batches, rows, cols in TP_SHAPES:
        Wh, Wl, ld_src = _tp_source(batches, rows, cols, X8B, seed=rows + cols)
        ld_dst = ops.round_up(rows, 32) + (32 if rows % 32 == 0 else 0)
        Th, Tl = _buf(batches * cols, ld_dst), _buf(batches * cols, ld_dst)
        keep.append((Wh, Wl, Th, Tl, ld_src, ld_dst))
        items.append(L.TpItem(L.ptr(Wh), L.ptr(Wl), L.ptr(Th), L.ptr(Tl), rows * ld_src, cols * ld_dst, ld_src, ld_dst, batches, rows, cols))
    assert sum(1 for b, r, c in TP_SHAPES if r % 4 == 0 and c % 4 == 0) == 4
    arr = (L.TpItem * len(items))(*items)
    L.check(L.lib.radmmm_transpose_f16_pair_multi(arr, len(items), X8B, ops.X8_W_EXP, L.stream()), "transpose_f16_pair_multi")
    torch.cuda.synchronize()
    for (batches, rows, cols), (Wh, Wl, Th, Tl, ld_src, ld_dst) in zip(TP_SHAPES, keep):
        hi_ref, second_ref = _tp_expect(Wh, Wl, batches, rows, cols, ld_src, ld_dst, X8B)
        _same(Th.cpu(), hi_ref, f"transpose_f16_pair_multi {batches, rows, cols}: hi")
        _same(_second(Tl.cpu(), X8B), second_ref, f"transpose_f16_pair_multi {batches, rows, cols}: cross array")


# ---------------------------------------------------------------------------------------------------------------------
# e. the GEMM epilogues' split outputs against the fp32 output of the same launch

S3 = (3, 64, [64, 51, 17])               # ragged batch, M = 192
W2 = (2, 224, [224, 100])                # the shared-window kernel wants T >= 32 * 7 rows per item
GEMM_CASES = {
    # name: (nprod, split format, taps, batch, N, switches, direct epilogue expected, extra descriptor fields)
    "per-tap x8": (2, X8A, 1, S3, 128, {"RADMMM_ONE": "0", "RADMMM_WIN": "0", "RADMMM_H3W_MB": "4"}, True),
    "per-tap x8 N=130": (2, X8A, 1, S3, 130, {"RADMMM_ONE": "0", "RADMMM_WIN": "0", "RADMMM_H3W_MB": "4"}, True),
    "one-tap x8": (2, X8A, 1, S3, 128, {"RADMMM_ONE": "1", "RADMMM_H3W_MB": "4"}, True),
    "one-tap x8 N=130": (2, X8A, 1, S3, 130, {"RADMMM_ONE": "1", "RADMMM_H3W_MB": "5"}, True),
    "shared window x8": (2, X8A, 5, W2, 128, {"RADMMM_WIN": "1", "RADMMM_H3W_MB": "7"}, True),
    "per-tap 5 taps x8": (2, X8A, 5, W2, 128, {"RADMMM_WIN": "0", "RADMMM_H3W_MB": "7"}, True),
    "per-tap f16": (3, F16, 1, S3, 128, {"RADMMM_H3_TILE": "256", "RADMMM_H3W_MB": "4"}, True),
    "per-tap f16 N=130": (3, F16, 1, S3, 130, {"RADMMM_H3_TILE": "256", "RADMMM_H3W_MB": "4"}, True),
    "generic f16 N=130": (3, F16, 1, S3, 130, {"RADMMM_H3_TILE": "128"}, False),
    "generic f16": (3, F16, 1, S3, 128, {"RADMMM_H3_TILE": "128"}, False),
    "generic x8 N=130": (3, X8A, 1, S3, 130, {"RADMMM_H3_TILE": "128"}, False),
    "generic x8 N=130, wide tile": (2, X8A, 1, S3, 130, {"RADMMM_ONE": "0", "RADMMM_WIN": "0", "RADMMM_H3W_MB": "4", "add": "1"}, False),
}


@pytest.mark.parametrize("launch", ["masked softplus", "scaled with flag"])
@pytest.mark.parametrize("case", list(GEMM_CASES))
def test_gemm_epilogue_split_outputs_are_the_model_of_c(case, launch, monkeypatch):
    """radmmm_rowgemm_h3 writes C and (Ch, Cl, Clo) in one launch: the split copy must be the model of ch_scale * C, whatever
    the kernel and the epilogue (store_pair_split of the direct epilogues copies the arithmetic of csrc/split_pack.h; the
    generic one calls it).  Tail rule of the generic epilogue with N % 4 != 0: the rest of the last 4-column group is
    written as zeros in the f16 format and skipped in the 8-bit formats; the direct epilogues write nothing beyond N."""
    ops, L = _api()
    nprod, fmt, taps, (B, T, lens), N, env, direct = GEMM_CASES[case]
    env = dict(env)
    with_add = env.pop("add", None)
    for k in ("RADMMM_ONE", "RADMMM_WIN", "RADMMM_H3W_MB", "RADMMM_H3_TILE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    M, K = B * T, 64
    ldch = ops.round_up(N, 32) + 32
    gen = torch.Generator().manual_seed(len(case) * 31 + N)
    grad = launch == "scaled with flag"
    S = 2048.0 if grad else 1.0
    xe = ops.X8_GRAD_EXP if grad else ops.X8_ACT_EXP
    x = ((torch.randn(M, K, generator=gen) * 3e-3) if grad else torch.nn.functional.softplus(torch.randn(M, K, generator=gen) * 2)).to(DEV)
    w = (torch.randn(N, K, taps, generator=gen) * 0.03).to(DEV)
    bias = torch.randn(N, generator=gen) * (1e-3 if grad else 0.5)
    if grad:                      # two columns beyond the 8-bit range, one of them beyond the fp16 clamp as well
        bias[7], bias[9] = 5.0, -40.0
    bias = bias.to(DEV)
    Ah, Al = ops.split_f16(x, K, S, K, nprod, xe)
    Wh, Wl, _ = ops.split_weight(w, None, K, nprod=nprod)
    Cf = torch.full((M + 1, N), float("nan"), device=DEV)
    Ch, Cl = _buf(M, ldch), _buf(M, ldch)
    Clo = _buf(M, ldch) if fmt != F16 else None
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    kw = dict(nprod=nprod, a8_exp=xe, b8_exp=ops.X8_W_EXP, acc_scale=1.0 / (S * ops.W_SCALE), T=T, Ah=Ah, Al=Al, lda_h=K, Bh=Wh,
              Bl=Wl, ldb_h=K, b_tap_stride_h=Wh.stride(0), C=Cf, ldc=N, M=M, N=N, K=K, taps=taps, dil=1, sign=1,
              lens=torch.tensor(lens, dtype=torch.int32, device=DEV), bias=bias, Ch=Ch, Cl=Cl, ldch=ldch, split_fmt=fmt, ch_x8_exp=xe)
    if Clo is not None:
        kw["Clo"] = Clo
    if with_add:
        kw.update(add=torch.zeros(M, N, device=DEV), ldadd=N)
    if grad:
        kw.update(ch_scale=S, sat_flag=flag)
    else:
        kw.update(a_mask_mode=1, postmask=1, act=1, ch_scale=1.0)
    scratch = torch.empty(int(L.lib.radmmm_rowgemm_h3_colsum_scratch_floats(M, N)), device=DEV)
    assert (L.rowgemm_h3_colsum_rows(colsum_scratch=scratch, **kw) > 0) == direct       # the epilogue this case is about
    L.rowgemm_h3(**kw)
    torch.cuda.synchronize()
    Cc = Cf.cpu()
    assert bool(torch.isnan(Cc[M]).all()) and bool(torch.isfinite(Cc[:M]).all()) and float(Cc[:M].abs().max()) > 0
    written = torch.zeros(ldch, dtype=torch.bool)
    written[:N] = True
    xfull = torch.zeros(M, ldch)
    xfull[:, :N] = Cc[:M]
    if fmt == F16 and not direct:
        written[:(N + 3) // 4 * 4] = True                                               # the partial group: zeros
    s, hi_ref, second_ref, lo_ref = _expect_rows(xfull, S if grad else 1.0, fmt, xe, mask=written)
    Chc, Clc = Ch.cpu(), _second(Cl.cpu(), fmt)
    _eq(Chc, hi_ref, case + ": Ch")
    _eq(Clc, second_ref, case + ": Cl")
    if Clo is not None:
        _eq(Clo.cpu(), lo_ref, case + ": Clo")
    if fmt == F16 and not direct:                                                       # the zero fill is exactly zero
        assert not bool(Chc[:M, N:(N + 3) // 4 * 4].any()) and not bool(Clc[:M, N:(N + 3) // 4 * 4].any())
    if grad:
        amax = float((Cc[:M] * S).abs().max())
        assert amax > 60000.0
        word = int(flag.item())
        if fmt == F16:
            assert word == 1
        else:
            _check_word(word, amax, fmt, xe, case)
    else:
        assert int(flag.item()) == 0


@pytest.mark.parametrize("fmt,with_lo16", [(F16, False), (X8A, False), (X8A, True)])
@pytest.mark.parametrize("D,h", [(8, 5), (8, 6), (7, 6), (7, 5)])
def test_wn_input_fwd_split_copy_is_the_model_of_x0(D, h, fmt, with_lo16):
    """radmmm_wn_input_fwd with X0 and X0h / X0l together: D % 4 == 0 takes the 4-wide path, D = 7 the 1-wide one, each
    with D + h odd and even; the padding columns up to ldx0 are written as zero"""
    ops, L = _api()
    rows, ldx0, e = 37, 32, ops.X8_ACT_EXP
    ctx = R.edge_matrix(rows, D, 1.0, e, seed=D)
    z = R.edge_matrix(rows, h, 1.0, e, seed=100 + h)
    ctx[0, 0], ctx[3, D - 1], z[1, h - 1], z[2, 0] = 0.0, -0.0, -0.0, 0.0                # +-0 inputs on both sides of the seam
    ldz = 8 if D % 4 == 0 else h                                         # (the 4-wide path wants ldz % 4 == 0)
    zb = torch.full((rows, ldz), 1e30)
    zb[:, :h] = z
    ctx_d, z_d = ctx.to(DEV), zb.to(DEV)
    X0 = torch.full((rows + 1, ldx0), float("nan"), device=DEV)
    Xh, Xl = _buf(rows, ldx0), _buf(rows, ldx0)
    lo16 = _buf(rows, ldx0) if with_lo16 else None
    L.check(L.lib.radmmm_wn_input_fwd(L.ptr(ctx_d), D, L.ptr(z_d), ldz, L.ptr(X0), ldx0, rows, D, h, L.ptr(Xh), L.ptr(Xl),
                                      L.split_opts(fmt, e, None, lo16), L.stream()), "wn_input_fwd")
    torch.cuda.synchronize()
    want = torch.zeros(rows, ldx0)
    want[:, :D], want[:, D:D + h] = ctx, z
    X0c = X0.cpu()
    assert torch.equal(X0c[:rows].view(torch.int32), want.view(torch.int32)) and bool(torch.isnan(X0c[rows]).all())
    _s, hi_ref, second_ref, lo_ref = _expect_rows(want, 1.0, fmt, e)
    zc = ZeroCount()
    inp = torch.arange(ldx0) < D + h
    Xhc, Xlc = Xh.cpu(), _second(Xl.cpu(), fmt)
    _eq(Xhc, hi_ref, "wn_input_fwd: hi", zc, inp)
    _eq(Xlc, second_ref, "wn_input_fwd: second array", zc, inp, fmt)
    # the padding columns are written as zero: exactly, in every array
    assert not bool(Xhc[:rows, D + h:].any())
    if fmt == F16:
        assert not bool(Xlc[:rows, D + h:].any())
    else:
        pb = R.pack_cross((~inp)[None].to(torch.uint8), (~inp)[None].to(torch.uint8), fmt, ldx0)[0].bool()
        assert not bool(Xlc[:rows, pb].any())
    if with_lo16:
        _eq(lo16.cpu(), lo_ref, "wn_input_fwd: lo16", zc, inp)
        assert not bool(lo16.cpu()[:rows, D + h:].any())
    assert zc.zeros >= 4


# ---------------------------------------------------------------------------------------------------------------------
# f. non-finite inputs

def test_infinities_clamp_and_report():
    ops, _ = _api()
    x = torch.tensor([[float("inf"), 1.0, float("-inf"), -2.0, float("inf")]], device=DEV)
    for fmt in (F16, X8A):
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        hi, second, _ = _split_dev(x, 5, 32, 1.0, fmt, ops.X8_ACT_EXP, False, flag)
        p60 = torch.tensor([60000.0, -60000.0]).half().view(torch.int16).tolist()
        assert hi[0, :5].tolist() == [p60[0], 0x3c00, p60[1], -0x4000, p60[0]]
        assert int(flag.item()) & 1
        if fmt == F16:
            assert second.view(torch.int16)[0, [0, 2, 4]].tolist() == [0, 0, 0]
        else:
            h8, l8 = R.unpack_cross(second[:1], fmt, 5)
            assert h8[0, [0, 2, 4]].tolist() == [0x7e, 0xfe, 0x7e] and l8[0, [0, 2, 4]].tolist() == [0, 0, 0]
            assert ops.GradScale._x8_level(int(flag.item())) == 6


def test_nan_gives_the_same_bytes_on_every_store_path(monkeypatch):
    """The header promises nothing for NaN (radmmm_weightnorm_bwd's `poison` argument exists because the operands clamp
    it); but the 4-wide store (radmmm_split_f16), the 1-wide store (radmmm_weightnorm_fwd_h3, Cin % 4 != 0) and the GEMM's
    pair store must agree, or an operand would depend on which kernel wrote it.  What they give is written into the
    "split formats" comment of include/radmmm_hip.h: NaN -> the bytes of -60000 (hi 0xfb53, lo 0, hi8 0xfe, lo8 0), and
    no flag bit."""
    ops, L = _api()
    e, nan = ops.X8_ACT_EXP, float("nan")
    got = {}
    # 4-wide
    x = torch.tensor([[nan, 1.0, 2.0, 3.0, 4.0, nan, 5.0, 6.0]], device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    hi, cross, lo16 = _split_dev(x, 8, 32, 1.0, X8A, e, True, flag)
    h8, l8 = R.unpack_cross(cross[:1], X8A, 8)
    for c in (0, 5):
        got[f"4-wide col {c}"] = (hi[0, c].item() & 0xffff, h8[0, c].item(), l8[0, c].item(), lo16[0, c].item() & 0xffff)
    flag4 = int(flag.item())
    # 1-wide: plain weights [Cout 1][Cin 7][taps 1] with scale 1 in the same format
    v = torch.tensor([nan, 1.0, 2.0, 3.0, 4.0, nan, 5.0], device=DEV).reshape(1, 7, 1)
    Wh, Wl = _buf(1, 32), _buf(1, 32)
    L.check(L.lib.radmmm_weightnorm_fwd_h3(L.ptr(v), None, L.ptr(Wh), L.ptr(Wl), None, 1, 7, 1, 32, 0, 0, 0, 1.0,
                                           L.split_opts(X8A, e), L.stream()), "weightnorm_fwd_h3")
    torch.cuda.synchronize()
    h8, l8 = R.unpack_cross(Wl.cpu().view(torch.uint8)[:1], X8A, 8)
    for c in (0, 5):
        got[f"1-wide col {c}"] = (Wh.cpu()[0, c].item() & 0xffff, h8[0, c].item(), l8[0, c].item(), None)
    # the GEMM's pair store: a NaN bias in an even and in an odd column
    for k in ("RADMMM_H3W_MB", "RADMMM_H3_TILE"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("RADMMM_ONE", "0")
    monkeypatch.setenv("RADMMM_WIN", "0")
    M, K, N = 64, 64, 128
    g = torch.Generator().manual_seed(3)
    a = torch.rand(M, K, generator=g).to(DEV)
    w = (torch.randn(N, K, 1, generator=g) * 0.03).to(DEV)
    bias = torch.zeros(N)
    bias[0] = bias[5] = nan
    Ah, Al = ops.split_f16(a, K, 1.0, K, 2, e)
    Bh, Bl, _ = ops.split_weight(w, None, K, nprod=2)
    Cf = torch.zeros(M, N, device=DEV)
    Ch, Cl, Clo = _buf(M, N), _buf(M, N), _buf(M, N)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    kw = dict(nprod=2, a8_exp=e, b8_exp=ops.X8_W_EXP, acc_scale=1.0 / ops.W_SCALE, T=M, Ah=Ah, Al=Al, lda_h=K, Bh=Bh, Bl=Bl, ldb_h=K,
              b_tap_stride_h=Bh.stride(0), C=Cf, ldc=N, M=M, N=N, K=K, bias=bias.to(DEV), Ch=Ch, Cl=Cl, Clo=Clo, ldch=N,
              ch_scale=1.0, split_fmt=X8A, ch_x8_exp=e, sat_flag=flag)
    scratch = torch.empty(int(L.lib.radmmm_rowgemm_h3_colsum_scratch_floats(M, N)), device=DEV)
    assert L.rowgemm_h3_colsum_rows(colsum_scratch=scratch, **kw) > 0                    # a direct epilogue: the pair store
    L.rowgemm_h3(**kw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(Cf[:, [0, 5]]).all()) and bool(torch.isfinite(Cf[:, 1:5]).all())
    h8, l8 = R.unpack_cross(Cl.cpu().view(torch.uint8)[:M], X8A, N)
    for c in (0, 5):
        for r in (0, M - 1):
            got[f"pair store row {r} col {c}"] = (Ch.cpu()[r, c].item() & 0xffff, h8[r, c].item(), l8[r, c].item(), Clo.cpu()[r, c].item() & 0xffff)
    print("NaN input ->", {k: tuple(hex(b) if b is not None else None for b in v) for k, v in got.items()},
          "flags:", hex(flag4), hex(int(flag.item())))
    first = got["4-wide col 0"]
    for k, v in got.items():
        assert v[:3] == first[:3], (k, v, first)
        assert v[3] is None or v[3] == first[3], (k, v, first)
    # what the header states
    assert first == (0xfb53, 0xfe, 0x00, 0x0000)
    assert flag4 == 0 and int(flag.item()) == 0
    # the neighbours of the NaN elements are what they would be without it
    s = R.split_ref(torch.tensor([[1.0, 2.0, 3.0, 4.0]]), 1.0, X8A, e)
    assert hi[0, 1:5].tolist() == s.hi.view(torch.int16)[0].tolist()
