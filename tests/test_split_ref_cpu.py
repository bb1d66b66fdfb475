"""The host model of the split operand formats (tests/_split_ref.py) against the specification in include/radmmm_hip.h
("split formats").  The GPU tests of tests/test_hip_split_direct.py compare the producers with this model bit for bit:
these tests are what keeps that model from being an unchecked twin.  No GPU, no built library."""
import math

import pytest
import torch

import _split_ref as R


def _f8(v):
    return R.e4m3_value(R.e4m3_bytes(torch.tensor(v, dtype=torch.float32))).tolist()


def test_host_conversions_round_to_nearest_even_subnormals_included():
    """the roundings the model rests on: torch's CPU conversions to fp16 and to e4m3"""
    # e4m3: 3 mantissa bits; spacing 2 in [16, 32), 2^-9 below 2^-6.  Ties go to the even neighbour.
    assert _f8([17.0, 19.0, 2.0 ** -10, 1.5 * 2.0 ** -9, 2.5 * 2.0 ** -9]) == [16.0, 20.0, 0.0, 2.0 ** -8, 2.0 ** -8]
    assert _f8([2.0 ** -10 * 1.001, 2.0 ** -10 * 0.999, 2.0 ** -9]) == [2.0 ** -9, 0.0, 2.0 ** -9]
    # saturation by the clamp in front: 464 and 480 would otherwise become the NaN byte
    assert _f8([447.0, 448.0, 449.0, 464.0, 480.0, 1000.0, -1e30]) == [448.0, 448.0, 448.0, 448.0, 448.0, 448.0, -448.0]
    assert R.e4m3_bytes(torch.tensor([448.0, -448.0, 0.0, 2.0 ** -9])).tolist() == [0x7e, 0xfe, 0x00, 0x01]
    # fp16: 10 mantissa bits, subnormal spacing 2^-24
    h = lambda v: torch.tensor(v, dtype=torch.float32).half().float().tolist()
    u = 2.0 ** -10
    assert h([1 + u / 2, 1 + u + u / 2, 1024.5, 1025.5]) == [1.0, 1 + 2 * u, 1024.0, 1026.0]
    assert h([2.0 ** -25, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 2.0 ** -25 * 1.001]) == [0.0, 2.0 ** -23, 2.0 ** -23, 2.0 ** -24]
    assert h([2.0 ** -14 - 2.0 ** -25]) == [2.0 ** -14]          # the largest subnormal's upper tie goes to the least normal


def test_reconstruction_bound():
    """|hi + lo - t| <= 2^-22 |t| + 2^-25 in float64: 11 + 11 significand bits, plus half the fp16 subnormal spacing
    for the lo part that has run out of exponent.  A flushed subnormal lo or a truncating conversion breaks it."""
    g = torch.Generator().manual_seed(5)
    worst = 0.0
    for mag in (1e-6, 1e-4, 1e-2, 1.0, 30.0, 3e3):
        x = torch.randn(250000, generator=g) * mag
        x = x[x.abs() >= 2.0 ** -126]
        for scale in (1.0, 2.0 ** -3):
            s = R.split_ref(x, scale)
            t = s.t.double()
            err = (s.hi.double() + s.lo.double() - t).abs()
            bound = 2.0 ** -22 * t.abs() + 2.0 ** -25
            worst = max(worst, float((err / bound).max()))
            assert bool((err <= bound).all()), (mag, scale, float((err / bound).max()))
    print(f"worst |hi + lo - t| / bound = {worst:.5f}")
    assert worst > 0.5                                           # the bound is tight: it is not a tolerance with slack


def test_split_model_fields():
    x = torch.tensor([1.0 + 2.0 ** -11 + 2.0 ** -20, -3.0, 0.0, 70000.0, float("inf"), float("-inf")])
    s = R.split_ref(x, 1.0, R.SPLIT_X8A, 2)
    assert s.t.tolist() == [x[0].item(), -3.0, 0.0, 60000.0, 60000.0, -60000.0]
    assert s.hi.float().tolist()[:2] == [1.0 + 2.0 ** -10, -3.0]
    assert s.r.tolist()[0] == x[0].item() - (1.0 + 2.0 ** -10)
    assert math.isinf(s.amax)
    # 60000 = 1875 * 32 is an fp16 value: the clamped elements have no residual
    assert s.hi.float().tolist()[3:] == [60000.0, 60000.0, -60000.0] and s.r.tolist()[3:] == [0.0, 0.0, 0.0]
    assert R.e4m3_value(s.hi8).tolist()[:2] == [4.0, -12.0]
    # lo8 = e4m3(r * 2^13): r = -2^-11 + 2^-20 -> -4 + 2^-7 -> -4
    assert R.e4m3_value(s.lo8).tolist()[0] == -4.0
    assert R.split_ref(torch.tensor([float("nan"), 2.0]), 4.0).amax == 8.0


@pytest.mark.parametrize("fmt", [R.SPLIT_X8A, R.SPLIT_X8B])
def test_cross_array_byte_round_trip(fmt):
    """all 256 e4m3 bytes (the NaN bytes 0x7f / 0xff excluded) through pack / unpack in both roles"""
    by = torch.tensor([b for b in range(256) if b not in (0x7f, 0xff)], dtype=torch.uint8)
    hi8 = by.reshape(2, 127)
    lo8 = by.flip(0).reshape(2, 127)
    ld = 160
    arr = R.pack_cross(hi8, lo8, fmt, ld, fill=R.FILL8)
    assert arr.shape == (2, 2 * ld)
    h2, l2 = R.unpack_cross(arr, fmt, 127)
    assert torch.equal(h2, hi8) and torch.equal(l2, lo8)
    # the bytes no column maps to keep the fill: column 127's two slots, and the 32-column group [128, 160)
    untouched = torch.ones(2 * ld, dtype=torch.bool)
    for c in range(127):
        untouched[R.x8_hi_off(c, fmt)] = untouched[R.x8_lo_off(c, fmt)] = False
    assert int(untouched.sum()) == 2 * ld - 2 * 127
    assert bool((arr[:, untouched] == R.FILL8).all())
    # every value survives the conversion back and forth (the bytes are e4m3 values, not opaque)
    assert torch.equal(R.e4m3_bytes(R.e4m3_value(by)), by)


def test_cross_array_layout_as_the_header_words_it():
    """per 32 columns 64 bytes: A role [ hi8 x 32 | lo8 x 32 ], B role [ lo8 x 32 | hi8 x 32 ]"""
    cols, ld = 70, 96
    hi8 = torch.arange(cols, dtype=torch.uint8)[None]                      # column c's hi8 byte is c, its lo8 byte 128 + c
    lo8 = hi8 + 128
    a = R.pack_cross(hi8, lo8, R.SPLIT_X8A, ld, fill=R.FILL8)[0].tolist()
    b = R.pack_cross(hi8, lo8, R.SPLIT_X8B, ld, fill=R.FILL8)[0].tolist()
    for c in (0, 1, 30, 31, 32, 33, 63, 64, 69):
        grp, k = divmod(c, 32)
        assert a[64 * grp + k] == c and a[64 * grp + 32 + k] == 128 + c
        assert b[64 * grp + k] == 128 + c and b[64 * grp + 32 + k] == c
    assert a[0:32] == list(range(32)) and a[32:64] == list(range(128, 160)) and a[64:96] == list(range(32, 64))
    assert a[128 + 6] == R.FILL8 and a[128 + 32 + 6] == R.FILL8            # columns 70 .. 95 of the last group
    assert b[0:32] == list(range(128, 160)) and b[32:64] == list(range(32))


def test_rederived_hi8_differs_from_hi8_only_in_double_rounding():
    # t = 17 + 2^-9: e4m3(t) = 18 (above the tie), but fp16(t) = 17 and e4m3(17) = 16 (the tie itself, to even)
    x = torch.tensor([17.0 + 2.0 ** -9, 17.0, 5.0])
    s = R.split_ref(x, 1.0, R.SPLIT_X8B, 0)
    assert R.e4m3_value(s.hi8).tolist() == [18.0, 16.0, 5.0]
    assert R.e4m3_value(R.rederived_hi8(s.hi, 0)).tolist() == [16.0, 16.0, 5.0]


@pytest.mark.parametrize("x8_exp", [2, -4, 0, -16, 16])
def test_flag_word_decodes_to_its_level(x8_exp):
    """flag_ref composed with ops.GradScale._x8_level returns L for every level, and lowering the exponent by L brings
    the element back into e4m3's range for L <= 5 (6 means "6 or more")"""
    from rad_mmm_amd.ops import GradScale
    unit = 448.0 * 2.0 ** -x8_exp
    # (with e = -16 the fp16 clamp comes first: bit 0 is judged on its own below)
    assert R.flag_ref(unit, R.SPLIT_X8A, x8_exp) & ~1 == 0 and GradScale._x8_level(0) == 0 and GradScale._x8_level(1) == 0
    assert R.flag_ref(unit * (1 - 2.0 ** -10), R.SPLIT_X8B, x8_exp) & ~1 == 0
    for L in range(1, 7):
        for amax in (unit * 2.0 ** (L - 1) * (1 + 2.0 ** -10), unit * 2.0 ** L * (1 - 2.0 ** -10), unit * 2.0 ** L):
            w = R.flag_ref(amax, R.SPLIT_X8A, x8_exp)
            assert w & 2 and w == (w & 1) | 2 | (1 << (1 + L)), (L, amax, w)          # one-hot level bit
            assert (w & 1) == (1 if amax > 60000.0 else 0)
            assert GradScale._x8_level(w) == L
            assert amax * 2.0 ** (x8_exp - L) <= 448.0
            if L > 1:
                assert amax * 2.0 ** (x8_exp - (L - 1)) > 448.0                         # and L is the smallest such
    for amax in (unit * 2.0 ** 6 * (1 + 2.0 ** -10), unit * 2.0 ** 9, float("inf")):
        assert GradScale._x8_level(R.flag_ref(amax, R.SPLIT_X8A, x8_exp)) == 6          # capped
    # several reports OR-ed into one word: the highest level wins
    w = R.flag_ref(unit * 3, R.SPLIT_X8A, x8_exp) | R.flag_ref(unit * 20, R.SPLIT_X8A, x8_exp) | R.flag_ref(unit * 1.5, R.SPLIT_X8A, x8_exp)
    assert GradScale._x8_level(w) == 5
    # the f16 format knows bit 0 only
    assert R.flag_ref(1e9, R.SPLIT_F16, x8_exp) == 1 and R.flag_ref(60000.0, R.SPLIT_F16, x8_exp) == 0
    assert R.flag_ref(60000.0 * (1 + 2.0 ** -10), R.SPLIT_F16, x8_exp) == 1


@pytest.mark.parametrize("scale,x8_exp", [(1.0, 2), (2048.0, -4), (256.0, 0), (2.0 ** -3, 2), (1.0, -16), (1.0, 16)])
def test_edge_pool_holds_the_classes_it_names(scale, x8_exp):
    """the input builder of the GPU tests, judged by the model: each class is present and has the property it is named for"""
    x, names = R.edge_pool(scale, x8_exp)
    s = R.split_ref(x, scale, R.SPLIT_X8A, x8_exp)
    cls = lambda n: torch.tensor([k == n for k in names])
    t64, r64 = s.t.double(), s.r.double()
    # fp16 ties: the residual is exactly half the spacing of hi's binade
    tie = cls("f16_tie")
    sp = torch.maximum(2.0 ** (torch.floor(torch.log2(s.t[tie].abs().double())) - 10), torch.tensor(2.0 ** -24, dtype=torch.float64))
    on_tie = (r64[tie].abs() == sp / 2)
    assert int(on_tie.sum()) >= 16
    lsb = lambda h: (h.view(torch.int16) & 1)
    assert set(lsb(s.hi[tie][on_tie]).tolist()) == {0}                       # ties went to the even neighbour ...
    away = (s.hi[tie][on_tie].float().abs() > s.t[tie][on_tie].abs())
    assert bool(away.any()) and bool((~away).any())                          # ... which lay above for some, below for others
    # e4m3 ties of the hi part: t * 2^e is exactly one of the tie values, and both directions occur
    v = (t64[cls("hi8_tie")] * 2.0 ** x8_exp).abs()
    got = R.e4m3_value(s.hi8[cls("hi8_tie")]).double().abs()
    ok = v <= 448.0
    if abs(x8_exp) <= 4:
        assert {17.0, 19.0, 2.0 ** -10, 1.5 * 2.0 ** -9} <= set(v.tolist())
        assert bool((got[ok] > v[ok]).any()) and bool((got[ok] < v[ok]).any())
    # lo8 edges: (t - hi) * 2^(11 + e) reproduces ties and the underflow neighbourhood exactly
    lv = (r64[cls("lo8_edge")] * 2.0 ** (11 + x8_exp)).abs()
    if abs(x8_exp) <= 4:
        assert {17.0, 19.0, 2.0 ** -10, 1.5 * 2.0 ** -9, 2.0 ** -9, 0.75 * 2.0 ** -10, 1.25 * 2.0 ** -10} <= set(lv.tolist())
        lo8 = R.e4m3_value(s.lo8[cls("lo8_edge")]).abs()
        assert bool((lo8 == 0).any()) and bool((lo8 == 2.0 ** -9).any())
    # subnormal classes
    lo_sub = s.lo[cls("lo_subnormal")].float().abs()
    assert bool(((lo_sub < 2.0 ** -14) & (lo_sub > 0)).any()) and bool((s.hi[cls("lo_subnormal")].float().abs() >= 2.0 ** -14).all())
    hi_sub = s.hi[cls("hi_subnormal")].float().abs()
    assert bool((hi_sub < 2.0 ** -14).all()) and bool((hi_sub > 0).any())
    xs = x[cls("x_subnormal")]
    assert bool((xs.abs() < 2.0 ** -126).all()) and bool((xs != 0).all())
    # clamps
    u = (x[cls("f16_clamp")].double() * scale).abs()
    assert {59999.0, 60000.0, 60001.0, 65504.0, 65520.0, 1e6, float("inf")} <= set(u.tolist())
    assert bool((s.t[cls("f16_clamp")].abs() <= 60000.0).all())
    c8 = (x[cls("e4m3_clamp")].double() * scale * 2.0 ** x8_exp).abs()
    assert {447.0, 448.0, 449.0, 464.0, 480.0, 1000.0} <= set(c8.tolist())
    assert not bool(((s.hi8 & 0x7f) == 0x7f).any()) and not bool(((s.lo8 & 0x7f) == 0x7f).any())      # no NaN byte anywhere
    assert bool((x[cls("zero")] == 0).all()) and cls("zero").sum() == 2
    # edge_rows puts every entry into a full group and into the tail; edge_matrix has the asked shape
    assert R.edge_rows(scale, x8_exp).shape == (x.numel(), 5)
    assert R.edge_matrix(3, 33, scale, x8_exp).shape == (3, 33)
