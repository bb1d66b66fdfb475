"""Host model of the split operand formats of include/radmmm_hip.h ("split formats"): torch on the CPU, no GPU, no built
library.  tests/test_split_ref_cpu.py holds this model to the specification; tests/test_hip_split_direct.py holds the
producers to the model, bit for bit.

  RADMMM_SPLIT_F16   hi = fp16(t), lo = fp16(t - hi),  t = clamp(scale * x, +-60000)
  RADMMM_SPLIT_X8A   hi as above + the 8-bit cross array: per 32 columns 64 bytes [ hi8 x 32 | lo8 x 32 ],
                     hi8 = e4m3(t * 2^e), lo8 = e4m3((t - hi) * 2^(11 + e))
  RADMMM_SPLIT_X8B   the same with the two 32-byte halves swapped [ lo8 | hi8 ]
  e4m3 = OCP FP8 E4M3 (torch.float8_e4m3fn), round to nearest even, saturated at +-448.

Everything is computed in fp32 with IEEE roundings (torch's CPU conversions round to nearest even, subnormals included:
checked in tests/test_split_ref_cpu.py).  No value here comes from the device."""
import math

import torch

SPLIT_F16, SPLIT_X8A, SPLIT_X8B = 0, 1, 2
F16_CLAMP = 60000.0
E4M3_MAX = 448.0
FLT_MAX = 3.4028234663852886e38
FILL16 = 0x7777                     # the pattern every output buffer of the direct tests starts as
FILL8 = 0x77


class Split:
    """model of one split: hi / lo as fp16 tensors, hi8 / lo8 as uint8 images of the e4m3 bytes (None in the f16 format),
    t / r the clamped value and its residual in fp32, amax = max |scale * x| (NaN elements ignored, as fmaxf does)"""
    __slots__ = ("hi", "lo", "hi8", "lo8", "t", "r", "amax")


def e4m3_bytes(v: torch.Tensor) -> torch.Tensor:
    """e4m3(clamp(v, +-448)) as uint8: the conversion saturates by the clamp in front of it (an unsaturated conversion
    of 464 or 480 would give the NaN byte)"""
    return v.clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).view(torch.uint8)


def e4m3_value(b: torch.Tensor) -> torch.Tensor:
    return b.contiguous().view(torch.float8_e4m3fn).float()


def split_ref(x: torch.Tensor, scale: float, fmt: int = SPLIT_F16, x8_exp: int = 0) -> Split:
    assert x.dtype == torch.float32 and not x.is_cuda
    s = Split()
    u = x * torch.tensor(scale, dtype=torch.float32)
    s.t = u.clamp(-F16_CLAMP, F16_CLAMP)
    s.hi = s.t.half()
    s.r = s.t - s.hi.float()                                   # exact in fp32 (Sterbenz / the residual of a rounding)
    s.lo = s.r.half()
    s.hi8 = s.lo8 = None
    if fmt != SPLIT_F16:
        s.hi8 = e4m3_bytes(s.t * torch.tensor(2.0 ** x8_exp, dtype=torch.float32))
        s.lo8 = e4m3_bytes(s.r * torch.tensor(2.0 ** (11 + x8_exp), dtype=torch.float32))
    au = u.abs()
    au = au[~torch.isnan(au)]
    s.amax = float(au.max()) if au.numel() else 0.0
    return s


def x8_hi_off(col, fmt):
    """byte offset of column col's hi8 inside a cross-array row"""
    return (col >> 5) * 64 + (col & 31) + (32 if fmt == SPLIT_X8B else 0)


def x8_lo_off(col, fmt):
    return (col >> 5) * 64 + (col & 31) + (0 if fmt == SPLIT_X8B else 32)


def pack_cross(hi8: torch.Tensor, lo8: torch.Tensor, fmt: int, ld: int, fill: int = 0) -> torch.Tensor:
    """[rows][cols] uint8 images -> the cross array [rows][2 * ld] bytes (ld in halves, ld % 32 == 0); bytes no column
    maps to are `fill`"""
    assert fmt in (SPLIT_X8A, SPLIT_X8B) and ld % 32 == 0 and hi8.shape == lo8.shape and hi8.shape[-1] <= ld
    cols = hi8.shape[-1]
    out = torch.full(hi8.shape[:-1] + (2 * ld,), fill, dtype=torch.uint8)
    c = torch.arange(cols)
    out[..., x8_hi_off(c, fmt)] = hi8
    out[..., x8_lo_off(c, fmt)] = lo8
    return out


def unpack_cross(by: torch.Tensor, fmt: int, cols: int):
    """cross array [rows][>= 2 * round_up(cols, 32)] bytes -> (hi8, lo8) [rows][cols] uint8"""
    assert fmt in (SPLIT_X8A, SPLIT_X8B) and by.dtype == torch.uint8
    c = torch.arange(cols)
    return by[..., x8_hi_off(c, fmt)], by[..., x8_lo_off(c, fmt)]


def rederived_hi8(hi: torch.Tensor, x8_exp: int) -> torch.Tensor:
    """what the transposes write in place of the producer's hi8: e4m3 of the value already rounded to fp16"""
    return e4m3_bytes(hi.float() * torch.tensor(2.0 ** x8_exp, dtype=torch.float32))


def flag_ref(amax: float, fmt: int, x8_exp: int) -> int:
    """the saturation word one element of magnitude amax = |scale * x| raises: bit 0 when the fp16 clamp changed it;
    in an 8-bit format bit 1 when amax * 2^e > 448 and then, one-hot, bit 1 + L, L the smallest of 1 .. 6 with
    amax * 2^e / 448 <= 2^L (6 when there is none)"""
    w = 1 if amax > F16_CLAMP else 0
    if fmt != SPLIT_F16:
        ratio = amax * 2.0 ** x8_exp / E4M3_MAX
        if ratio > 1.0:
            L = 6
            for l in range(1, 7):
                if ratio <= 2.0 ** l:
                    L = l
                    break
            w |= 2 | (1 << (1 + L))
    return w


# ---------------------------------------------------------------------------------------------------------------------
# inputs at the edges of the formats

def edge_pool(scale: float, x8_exp: int, seed: int = 0):
    """(x, cls): fp32 inputs x whose scale * x visits every rounding, subnormal and clamp edge of the formats, and the
    class name of each.  scale is a power of two, so x = target / scale is exact wherever it does not leave fp32."""
    assert math.frexp(scale)[0] == 0.5
    g = torch.Generator().manual_seed(1234 + seed)
    e = x8_exp
    groups = []

    def add(name, vals, signed=True):
        v = torch.as_tensor(vals, dtype=torch.float64).flatten()
        if signed:
            v = torch.cat([v, -v])
        groups.append((name, v))

    for sig in (1e-4, 1.0, 30.0):
        add("normal", torch.randn(24, generator=g, dtype=torch.float64) * sig, signed=False)
    # fp16 ties: t exactly halfway between two fp16 neighbours; even lower neighbour (-> down) and odd (-> up); normal
    # binades and the fp16 subnormals (2^-25: halfway between 0 and the least subnormal)
    u10 = 2.0 ** -10
    add("f16_tie", [1 + u10 / 2, 1 + u10 + u10 / 2, 1024.5, 1025.5, (1 + 3 * u10 / 2) * 2.0 ** -9, 32768 + 16, 32768 + 48,
                    2.0 ** -25, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 2.0 ** -14 - 2.0 ** -25])
    # e4m3 ties of t * 2^e (3 mantissa bits: 17 -> 16, 19 -> 20, 2^-10 -> 0, 1.5 * 2^-9 -> 2^-8), and just beside them
    ties8 = [17.0, 19.0, 2.0 ** -10, 1.5 * 2.0 ** -9, 2.5 * 2.0 ** -9, 1.0625, 1.1875, 416.0, 432.0]
    add("hi8_tie", [v * 2.0 ** -e for v in ties8])
    add("hi8_near_tie", [v * 2.0 ** -e * f for v in ties8[:4] for f in (1 - 2.0 ** -12, 1 + 2.0 ** -12)])
    # the same for r * 2^(11 + e): t = H + r with H = 2^k an fp16 value whose half-ulp exceeds r and whose fp32 significand
    # still holds r exactly (the candidates that fit neither are dropped; the tests count what is left)
    lo_vals = []
    for v in ties8 + [2.0 ** -9, 0.75 * 2.0 ** -10, 1.25 * 2.0 ** -10, 0.75 * 2.0 ** -9, 1.25 * 2.0 ** -9, 2.0 ** -11]:
        r = v * 2.0 ** -(11 + e)
        low = math.frexp(r)[1] - 1 - 5                          # exponent of the lowest of 6 significand bits of r
        for k in (min(15, low + 23), min(15, low + 20)):
            if k >= -24 and r < 2.0 ** (max(k, -14) - 11):
                lo_vals.append(2.0 ** k + r)
                lo_vals.append(2.0 ** k * 1.5 - r)
    add("lo8_edge", lo_vals)
    # |t| in [2^-14, 2^-3]: lo is an fp16 subnormal;  |t| < 2^-14: hi is one
    add("lo_subnormal", 2.0 ** (torch.rand(24, generator=g, dtype=torch.float64) * 11 - 14))
    add("hi_subnormal", 2.0 ** (torch.rand(16, generator=g, dtype=torch.float64) * 12 - 26))
    add("zero", [0.0])
    add("f16_clamp", [59999.0, 60000.0, 60001.0, 65504.0, 65520.0, 1e6])
    add("e4m3_clamp", [v * 2.0 ** -e for v in (447.0, 448.0, 449.0, 464.0, 480.0, 1000.0)])
    names, vals = [], []
    for name, v in groups:
        names += [name] * v.numel()
        vals.append(v / scale)
    x = torch.cat(vals).to(torch.float32)
    # values stated on x itself: fp32 subnormals, and the largest finite / infinite inputs (scale * x stays above the clamp)
    tiny = 2.0 ** -149
    extra = [("x_subnormal", [tiny, 3 * tiny, 2.0 ** -127, -tiny, -(2.0 ** -128 + tiny)]),
             ("f16_clamp", [FLT_MAX if scale <= 1 else FLT_MAX / scale, -(FLT_MAX if scale <= 1 else FLT_MAX / scale),
                            float("inf"), float("-inf")])]
    for name, v in extra:
        names += [name] * len(v)
        x = torch.cat([x, torch.tensor(v, dtype=torch.float64).to(torch.float32)])
    return x, names


def edge_matrix(rows: int, cols: int, scale: float, x8_exp: int, seed: int = 0) -> torch.Tensor:
    """[rows][cols] inputs: the pool of edge_pool in a seeded random order, cycled along the rows -- every window of
    columns (a full 4-column group, a row tail) sees another part of the pool in every row and for every seed.  A small
    shape cannot hold every class; edge_rows is the layout that provably puts each one in both places."""
    pool, _ = edge_pool(scale, x8_exp, seed)
    n = pool.numel()
    pool = pool[torch.randperm(n, generator=torch.Generator().manual_seed(99 + seed))]
    idx = (torch.arange(rows)[:, None] * (cols + 7) + torch.arange(cols)[None, :]) % n
    return pool[idx].contiguous()


def edge_rows(scale: float, x8_exp: int, cols: int = 5, seed: int = 0) -> torch.Tensor:
    """[len(pool)][cols] with row i filled with pool entry i: with cols % 4 != 0 every entry of every class lands both
    in a full 4-column group and in the row tail"""
    pool, _ = edge_pool(scale, x8_exp, seed)
    return pool[:, None].expand(-1, cols).contiguous()
