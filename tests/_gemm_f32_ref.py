"""Host model of the fp32 GEMM family (include/radmmm_hip.h: radmmm_rowgemm_f32 and radmmm_wgrad_f32) in float64, written
from the header's text, and the table of cases that tests/test_gemm_f32_ref_cpu.py (no GPU) and
tests/test_hip_gemm_f32_direct.py (GPU) share.  The method is the one of tests/_gemm_ref.py: operands are small signed
integers times powers of two, so every fp32 sum a kernel can form is exact whatever its tile shape, k order or split-K (each
case computes its bit budget, max over the outputs of sum |terms| * 2^q, and it must stay below 2^24: a condition of the
method, not a tolerance) and the output must equal this model word for word.

The model reads the operands the way the header addresses them -- from the FLAT arrays, with lda / a_item_stride / ldb /
b_tap_stride / b_layout -- and the flat arrays hold a quiet NaN wherever the header says a kernel must not look (A columns
[K, lda), B columns past K or past N, B rows past N, frames at or above lens[b] under a_mask_mode 1, the pad columns of
add / dact_src / c2_src, GY / X columns past Mc / Nc, X frames at or above lens[b] under x_mask_mode 1).  A model, or a
kernel, that looks there gets a NaN into a stored output.

Every case names the kernel its descriptor must reach as RADMMM_F32_KERNEL_CODE (radmmm_rowgemm_f32_plan /
radmmm_wgrad_f32_plan report it on the host): the table reaches all 21 kernels of the family by shape alone.

bug=: planted faults of the kind a kernel of this family can have.  tests/test_gemm_f32_ref_cpu.py demands that every one
of them changes at least one expected word of at least one case; inputs that cannot see a fault prove nothing about it."""

import numpy as np
import torch

from _gemm_ref import BUDGET, FILL32, accumulation_bar, row_mask, rowgemm_epilogue, tap_shifts, to_f32_exact, words, _frame_map  # noqa: F401
from _split_ref import SPLIT_F16, split_ref

GENERIC, ROWS16, MIX, WGRAD, WGRAD16 = 1, 2, 3, 4, 5
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 2, 3
EPS32 = float(np.float32(1e-6))                  # the 1e-6 of the header's ratio, as the fp32 constant a kernel holds
MAGS = tuple(range(1, 10))                       # 9 distinct non-zero magnitudes: a swapped row or column shows
Q = 3                                            # every value is an integer times 2^-Q
NAN = float("nan")

ROW_BUGS = ("drop_last_kquad", "ignore_sign", "cross_item", "ignore_lens", "m_end_short", "pass3_from_pass2",
            "framed_last_zero", "swap_masks")
WGRAD_BUGS = ("last_split_twice", "ignore_x_mask")


def kernel_code(family, bl=0, mt=0, rows=0):
    """RADMMM_F32_KERNEL_CODE of the header"""
    return family * 1000000 + bl * 100000 + mt * 1000 + rows


def code_fields(code):
    return dict(family=code // 1000000, bl=code // 100000 % 10, mt=code // 1000 % 100, rows=code % 1000)


def _vals(g, shape, scale=1.0, zero_every=8):
    """signed integers of MAGS times scale, zero with probability 1 / zero_every only (0: never)"""
    v = torch.tensor(MAGS, dtype=torch.float64)[torch.randint(0, len(MAGS), shape, generator=g)]
    v = v * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    if zero_every:
        v = v * (torch.randint(0, zero_every, shape, generator=g) != 0)
    return v * scale


def _padded(vals, ld, pad=NAN, rows=None):
    """[rows][ld] array with vals in the leading columns and `pad` everywhere else"""
    out = torch.full((rows or vals.shape[0], ld), pad, dtype=torch.float64)
    out[:vals.shape[0], :vals.shape[1]] = vals
    return out


# ---------------------------------------------------------------------------------------------------------------------
# radmmm_rowgemm_f32

def _a_rows(Aflat, c, shift, bug=None, kcols=None):
    """Am[r + shift, :K] of the header for every output row r, read from the flat A: item b, frame t at
    b * a_item_stride + t * lda (a_item_stride 0: row r at r * lda).  A frame counts when it lies in its own item and in
    [0, T) (a_mask_mode 0) or [0, lens[b]) (a_mask_mode 1); lens[b] may exceed T in the framed form."""
    M, T, K, lda = c["M"], c["T"], c["K"], c["lda"]
    kcols = K if kcols is None else kcols
    r = torch.arange(M)
    b, t = r // T, r % T
    stride = c["a_item_stride"] or T * lda
    lim = torch.full((M,), T, dtype=torch.long)
    if c["a_mask_mode"] and c.get("lens") is not None and bug != "ignore_lens":
        lim = torch.as_tensor(c["lens"], dtype=torch.long)[b]
    ts = t + shift
    ok = (ts >= 0) & (ts < lim)
    if bug == "cross_item" and not c["a_mask_mode"] and not c["a_item_stride"]:
        ok = (r + shift >= 0) & (r + shift < M)
    if bug == "framed_last_zero" and c["a_item_stride"]:
        ok = ok & ~((b == M // T - 1) & (ts > T - 1))
    idx = torch.where(ok, b * stride + ts * lda, torch.zeros_like(ts))
    rows = Aflat[idx[:, None] + torch.arange(kcols)[None, :]]
    return torch.where(ok[:, None], rows, torch.zeros((), dtype=torch.float64))     # a select: a masked frame is not looked at


def _b_tap(Bflat, c, tap, kcols=None):
    """Bt[tap](k, n) as a [K][N] view of the flat B"""
    N, K, ldb = c["N"], c["K"], c["ldb"]
    kcols = K if kcols is None else kcols
    base = tap * c["b_tap_stride"]
    st = (1, ldb) if c["b_layout"] == 0 else (ldb, 1)
    return torch.as_strided(Bflat, (kcols, N), st, base)


def rowgemm_f32_acc(Aflat, Bflat, c, bug=None, absolute=False):
    """acc[r, n] = sum_tap sum_k Am[r + shift(tap), k] * Bt[tap](k, n), float64"""
    sign = 1 if bug == "ignore_sign" else c["sign"]
    acc = torch.zeros(c["M"], c["N"], dtype=torch.float64)
    for tap, s in enumerate(tap_shifts(c["taps"], c["dil"], sign)):
        kc = c["K"] - 4 if (bug == "drop_last_kquad" and tap == c["taps"] - 1) else c["K"]
        a, b = _a_rows(Aflat, c, s, bug, kc), _b_tap(Bflat, c, tap, kc)
        acc += (a.abs() @ b.abs()) if absolute else (a @ b)
    return acc


def ratio64(c):
    """the header's ratio per row in float64: taps_r / (cnt + 1e-6), cnt = taps of a (ratio_taps, ratio_dil) window centred
    on the row whose frame is below lens[b] (and not negative); 0 where cnt == 0"""
    M, T = c["M"], c["T"]
    r = torch.arange(M)
    t = r % T
    lens = torch.as_tensor(c["lens"], dtype=torch.long)[r // T] if c.get("lens") is not None else torch.full((M,), T)
    cnt = torch.zeros(M, dtype=torch.float64)
    for k in range(c["ratio_taps"]):
        ts = t + (k - c["ratio_taps"] // 2) * c["ratio_dil"]
        cnt += ((ts >= 0) & (ts < lens)).double()
    return torch.where(cnt > 0, c["ratio_taps"] / (cnt + EPS32), torch.zeros_like(cnt))


def rowgemm_f32_expected(p, c, bug=None):
    """{"C", "C2"} in float64 (+ "mag": the magnitude sum the inexact bar is made of) from the header's epilogue order:
    pconv, premask, bias, add, postmask, dact, rowscale, act, C; C2.  The exact steps are _gemm_ref.rowgemm_epilogue's
    (premask and add are applied here and handed over as the accumulator: add sits between bias and postmask, and in
    float64 on exact values the order of the two additions is immaterial)."""
    cc = dict(c, acc_scale=1.0)
    if bug == "swap_masks":
        cc["premask"], cc["postmask"] = c["postmask"], c["premask"]
    v = rowgemm_f32_acc(p.A, p.B, c, bug)
    mag = v.abs() if c["inexact"] else None                      # |v| of the inexact steps' bar
    M, N, T = c["M"], c["N"], c["T"]
    m = row_mask(M, T, c.get("lens"))[:, None]
    side = {k: x for k, x in p.side.items()}
    if c["pconv"]:
        v, mag = v * ratio64(c)[:, None], mag * ratio64(c)[:, None]
    if cc["premask"]:
        v = v * m
    if c["add"]:
        v = v + p.side["add"][:, :N]
        if mag is not None:
            mag = mag + p.side["add"][:, :N].abs()
    if mag is not None and c["bias"]:
        mag = mag + p.side["bias"].abs()[None, :]
    if c["dact"]:
        side["dact_src"] = p.side["dact_src"][:, :N]
    if c["c2"] == "src3":
        side["c2_src"] = [s[:, :N] for s in p.side["c2_src"]]
    if not c["inexact"]:
        out = rowgemm_epilogue(v, dict(cc, premask=0), side)
    else:
        # the inexact steps, by the header's formulas in float64
        if c["bias"]:
            v = v + side["bias"][None, :]
        if cc["postmask"]:
            v = v * m
        if c["dact"] == ACT_LEAKY:
            v = v * torch.where(side["dact_src"] > 0, 1.0, 0.01)
        elif c["dact"] == ACT_RELU:
            v = v * (side["dact_src"] > 0).double()
        if c["rowscale"] == 1:
            v = v * m
        elif c["rowscale"] == 2:
            v, mag = v * m * ratio64(c)[:, None], mag * ratio64(c)[:, None]
        if c["act"] == ACT_LEAKY:
            v = torch.where(v > 0, v, 0.01 * v)
        out = {"C": v, "mag": mag}
    if bug in ("m_end_short", "pass3_from_pass2"):
        f = code_fields(c["expect"])
        assert f["family"] == ROWS16
        for k in [k for k in ("C", "C2") if k in out]:
            o = out[k].clone()
            for m0 in range(0, M, f["rows"]):
                end = min(m0 + f["rows"], M)
                if bug == "m_end_short":
                    o[end - 1] = 0                                         # the tile's last row is never produced
                elif end - m0 > 192:
                    o[m0 + 192:end] = out[k][m0 + 128:m0 + 128 + end - m0 - 192]
            out[k] = o
    return out


def _rcase(name, expect, **kw):
    c = dict(name=name, expect=expect, taps=1, dil=1, sign=1, a_mask_mode=0, b_layout=0, framed=False, lens=None, bias=False, premask=0,
             postmask=0, rowscale=0, dact=0, act=0, pconv=0, ratio_taps=1, ratio_dil=1, add=False, c2=None, odd_ldc=False, split=False,
             ch_scale=1.0, inexact=False, r=0, real=False, lda_pad=4, ldb_pad=4, ldc=None)
    c.update(kw)
    assert c["M"] % c["T"] == 0
    return c


def ragged_lens(T, items, dil, i=0):
    """ragged valid lengths: one 0, one T, one with 2 * dil >= lens[b] > 0, the rest spread over 1 .. T - 1"""
    lens = [T, 0, max(1, min(dil, T - 1))]
    lens += [1 + (7 * k + 3 * i) % (T - 1) for k in range(items - 3)]
    assert len(lens) == items and 0 in lens and T in lens and any(0 < x <= 2 * dil for x in lens)
    return lens


# the 16-row kernel: (MT, M, T, N, rows per tile) -- every rows % 4 != 0, a shorter last m-tile, N % 4 != 0, several
# items so that item borders fall inside tiles.  tests/test_gemm_f32_ref_cpu.py checks the codes on the built library.
ROWS16_SHAPES = ((4, 65, 13, 1021, 33), (6, 322, 46, 6141, 81), (8, 2241, 83, 3069, 125), (10, 774, 43, 5117, 155),
                 (12, 1938, 51, 5117, 177), (13, 1155, 77, 5117, 193), (14, 2088, 58, 3069, 209), (15, 2691, 69, 5117, 225))

# seven feature sets for the seven MT > 4; layout 1 takes them rotated by three, so every set lands on two different
# MT > 4, once per layout.  "lens": "ragged" is filled in per shape.
_FEATURES = (
    dict(taps=3, dil=1, sign=1, a_mask_mode=0, bias=True, premask=1, c2="store", lens="ragged"),
    dict(taps=5, dil=2, sign=-1, a_mask_mode=1, bias=True, postmask=1, add=True, odd_ldc=True, lens="ragged"),
    dict(taps=3, dil=8, sign=1, a_mask_mode=1, rowscale=1, dact=ACT_RELU, c2="accum", lens="ragged"),
    dict(taps=1, dil=1, sign=1, a_mask_mode=1, bias=True, add=True, c2="src3", lens="ragged"),
    dict(taps=3, dil=1, sign=1, a_mask_mode=1, framed=True, bias=True, lens="T+1"),
    dict(taps=5, dil=1, sign=-1, a_mask_mode=0, bias=True, postmask=1, split=True, ch_scale=2.0 ** -2, lens="ragged"),
    dict(taps=5, dil=8, sign=1, a_mask_mode=0, bias=True, premask=1, postmask=1, dact=ACT_RELU, c2="src3", odd_ldc=True, lens="ragged"),
)
_FEATURES_MT4 = (dict(taps=3, dil=2, sign=-1, a_mask_mode=1, bias=True, postmask=1, add=True, lens="ragged"),
                 dict(taps=5, dil=1, sign=1, a_mask_mode=0, rowscale=1, dact=ACT_RELU, c2="accum", odd_ldc=True, lens="ragged"))


def _with_lens(f, T, items, i):
    f = dict(f)
    if f["lens"] == "ragged":
        f["lens"] = ragged_lens(T, items, f["dil"], i)
    elif f["lens"] == "T+1":
        f["lens"] = [T + 1] * items
        f["dil"] = 1 + (i // 2) % 2                             # dil 2: frame T is reached from frame T - 2, T + 1 is masked
    return f


def rows16_cases():
    cases = []
    for bl in (0, 1):
        for j, (mt, M, T, N, rows) in enumerate(ROWS16_SHAPES):
            f = _FEATURES_MT4[bl] if j == 0 else _FEATURES[(j - 1 + 3 * bl) % 7]
            f = _with_lens(f, T, M // T, j + bl)
            cases.append(_rcase(f"rows16-mt{mt}-bl{bl}", kernel_code(ROWS16, bl, mt, rows), M=M, T=T, N=N, K=(16, 32)[(j + bl) % 2],
                                b_layout=bl, **f))
    return cases


def generic_cases():
    """K % 16 != 0: the 128 x 128 kernel.  K in {6, 33, 70} x M in {1, 127, 129, 300} x N in {1, 50, 130} spread over 12
    cases per layout with the same feature sets, the framed and the split case once each"""
    cases = []
    shapes = [(1, 1, 1), (127, 127, 1), (129, 43, 3), (300, 25, 12)]            # (M, T, items)
    i = 0
    for bl in (0, 1):
        for K in (6, 33, 70):
            for (M, T, items) in shapes:
                i += 1
                N = (1, 50, 130)[(i + bl) % 3]
                if items >= 3:
                    f = _with_lens(_FEATURES[(i + 2 * bl) % 7], T, items, i)
                elif items == 1 and T == 1:
                    f = dict(taps=3, dil=1, sign=-1, a_mask_mode=0, bias=True, lens=[1])
                else:
                    f = dict(taps=5, dil=(2, 8)[bl], sign=(1, -1)[bl], a_mask_mode=1, bias=True, postmask=1, add=bool(bl),
                             c2=("accum", "store")[bl], lens=[T - 30])
                cases.append(_rcase(f"generic-K{K}-M{M}-N{N}-bl{bl}", kernel_code(GENERIC, bl), M=M, T=T, N=N, K=K, b_layout=bl, **f))
    return cases


def mix_cases():
    cases = []
    lds = (160, 164, 192)
    i = 0
    for bl in (0, 1):
        for M, T in ((1, 1), (63, 63), (64, 16), (65, 13), (231, 77)):
            i += 1
            cases.append(_rcase(f"mix-M{M}-bl{bl}", kernel_code(MIX, bl), M=M, T=T, N=160, K=160, b_layout=bl, bias=bool((i + bl) % 2),
                                lda_pad=lds[i % 3] - 160, ldb_pad=lds[(i + 1) % 3] - 160, ldc=lds[(i + 2) % 3]))
    # one case per excluded condition: they must fall through to the 16-row kernel (K = 160 is a multiple of 16)
    fall = kernel_code(ROWS16, 0, 4, 58)
    cases.append(_rcase("mix-not-add", fall, M=231, T=77, N=160, K=160, add=True, bias=True, ldc=164))
    cases.append(_rcase("mix-not-premask", fall, M=231, T=77, N=160, K=160, premask=1, lens=[77, 0, 30], ldc=160))
    cases.append(_rcase("mix-not-ldc161", fall, M=231, T=77, N=160, K=160, ldc=161))
    return cases


# Inexact epilogue steps on EXACT accumulators.  r = the fp32 roundings on the element's path (a fused multiply-add only
# removes one); the bar is r * 2^-24 * (|v| * ratio + |bias| + |add|).
#   pconv + bias + add + leaky act : ratio's addition, its division, v * ratio, + bias, + add, the constant 0.01, v * 0.01  -> 7
#   rowscale 2 + leaky dact        : the constant 0.01, v * act', ratio's addition, its division, v * (mask * ratio)         -> 5
def inexact_cases():
    a = dict(taps=3, dil=2, a_mask_mode=1, pconv=1, ratio_taps=3, ratio_dil=2, bias=True, add=True, act=ACT_LEAKY, inexact=True, r=7)
    b = dict(taps=5, dil=1, sign=-1, a_mask_mode=0, rowscale=2, ratio_taps=5, ratio_dil=1, dact=ACT_LEAKY, inexact=True, r=5)
    return [
        _rcase("inexact-rows16-pconv", kernel_code(ROWS16, 0, 4, 58), M=115, T=23, N=130, K=32, lens=ragged_lens(23, 5, 2), **a),
        _rcase("inexact-rows16-rowscale2", kernel_code(ROWS16, 1, 4, 58), M=115, T=23, N=130, K=16, b_layout=1, lens=ragged_lens(23, 5, 1), **b),
        _rcase("inexact-generic-pconv", kernel_code(GENERIC, 1), M=129, T=43, N=50, K=33, b_layout=1, lens=[43, 0, 2], **a),
        _rcase("inexact-generic-rowscale2", kernel_code(GENERIC, 0), M=129, T=43, N=130, K=70, lens=[43, 0, 2], **b),
    ]


def realistic_cases():
    """Gaussian operands at scales that are no powers of two: one per family, the 16-row kernel on an MT > 8 per layout"""
    return [
        _rcase("real-rows16-mt10-bl0", kernel_code(ROWS16, 0, 10, 155), real=True, M=774, T=43, N=5117, K=32, taps=3, dil=2, a_mask_mode=1,
               lens=ragged_lens(43, 18, 2)),
        _rcase("real-rows16-mt13-bl1", kernel_code(ROWS16, 1, 13, 193), real=True, M=1155, T=77, N=5117, K=16, taps=5, dil=1, sign=-1,
               b_layout=1),
        _rcase("real-generic", kernel_code(GENERIC, 0), real=True, M=300, T=25, N=130, K=70, taps=3, dil=1, a_mask_mode=1,
               lens=ragged_lens(25, 12, 1)),
        _rcase("real-mix", kernel_code(MIX, 1), real=True, M=231, T=77, N=160, K=160, b_layout=1, ldc=164),
    ]


def rowgemm_cases():
    cases = rows16_cases() + generic_cases() + mix_cases()
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    return cases


class Problem:
    pass


def build_rowgemm(c, poison=True, seed=0):
    """flat operands (float64, NaN where a kernel must not look), side inputs, pitches, expected outputs, bit budget.
    poison=False leaves ordinary values in the masked frames (the planted-bug controls: a fault must show in VALUES)"""
    g = torch.Generator().manual_seed(3000 + seed + sum(map(ord, c["name"])))
    pad = NAN if poison else 5.0
    p = Problem()
    M, N, K, T, taps = c["M"], c["N"], c["K"], c["T"], c["taps"]
    items = M // T
    real = c["real"]
    draw = (lambda shape, scale: (torch.randn(shape, generator=g, dtype=torch.float64) * scale * 1.37).float().double()) if real else \
           (lambda shape, scale: _vals(g, shape, scale))
    if c["framed"]:
        # STFT framing: overlapping frames (lda < K), lens[b] = T + 1 frames per item, of which frame T is read by the taps of
        # the last rows only; the allocation ends exactly at the last float of frame T of the LAST item
        # (K % 4 != 0, the generic kernel only: its 16-byte loads of the last frame's last chunk end at roundup4(K))
        lda = 4 if K <= 8 else 8
        F = T + 1
        per = (F - 1) * lda + K
        stride = (per + 3) // 4 * 4 + 4                           # a gap of poison between the items
        flat = torch.full(((items - 1) * stride + per + (-K) % 4,), pad, dtype=torch.float64)
        for b in range(items):
            flat[b * stride:b * stride + per] = draw((per,), 1.0)
        c.update(lda=lda, a_item_stride=stride)
        p.A = flat
    else:
        lda = (K + 3) // 4 * 4 + c["lda_pad"]
        A = _padded(draw((M, K), 1.0), lda, pad)
        if c["a_mask_mode"] and c["lens"] is not None:
            for b in range(items):
                A[b * T + c["lens"][b]:(b + 1) * T] = pad         # frames at or above lens[b]
        c.update(lda=lda, a_item_stride=0)
        p.A = A.reshape(-1)
    wscale = 0.031 if real else 2.0 ** -Q
    if c["b_layout"] == 0:
        ldb = (K + 3) // 4 * 4 + c["ldb_pad"]
        B = torch.full((taps, N + 3, ldb), pad, dtype=torch.float64)        # rows >= N and columns >= K: poison
        B[:, :N, :K] = draw((taps, N, K), wscale)
        c.update(ldb=ldb, b_tap_stride=(N + 3) * ldb)
    else:
        ldb = (N + 3) // 4 * 4 + c["ldb_pad"]
        B = torch.full((taps, K, ldb), pad, dtype=torch.float64)            # columns >= N: poison
        B[:, :, :N] = draw((taps, K, N), wscale)
        c.update(ldb=ldb, b_tap_stride=K * ldb)
    p.B = B.reshape(-1)
    sc = 2.0 ** -Q
    side = {}
    p.ldside = (N + 3) // 4 * 4 + 4
    ints = lambda shape: _vals(g, shape, sc, zero_every=0)
    if c["bias"]:
        side["bias"] = ints((N,))
    if c["add"]:
        side["add"] = _padded(ints((M, N)), p.ldside, pad)
    if c["dact"]:
        side["dact_src"] = _padded(_vals(g, (M, N), 0.25, zero_every=4), p.ldside, pad)
    if c["c2"] == "accum":
        side["C2"] = ints((M, N))
    if c["c2"] == "src3":
        side["c2_src"] = [_padded(ints((M, N)), p.ldside, pad) for _ in range(3)]
    p.side = side
    p.ldc = c["ldc"] or ((N + 5 if (N + 5) % 2 else N + 6) if c["odd_ldc"] else (N + 3) // 4 * 4 + 4)
    out = rowgemm_f32_expected(p, c)
    p.out64 = out
    p.budget = None
    if not real:
        mag = rowgemm_f32_acc(p.A, p.B, c, absolute=True)
        for k in ("bias", "add", "C2"):
            if k in side:
                x = side[k][:, :N].abs() if side[k].dim() == 2 else side[k].abs()[None, :]
                mag = mag + x
        for s in side.get("c2_src", []):
            mag = mag + s[:, :N].abs()
        p.budget = float(mag.max()) * 2.0 ** Q                    # A integers, B and the side inputs multiples of 2^-Q
    if not real and not c["inexact"]:
        p.C = to_f32_exact(out["C"])
        p.C2 = to_f32_exact(out["C2"]) if "C2" in out else None
        p.split = split_ref(p.C, c["ch_scale"], SPLIT_F16) if c["split"] else None
        p.ldch = (N + 7) // 8 * 8 + 8
    return p


def zero_fraction(x):
    x = x[~torch.isnan(x)]
    return float((x == 0).double().mean())


# ---------------------------------------------------------------------------------------------------------------------
# radmmm_wgrad_f32

def wgrad_bk(c):
    """frames per K step: 16 on the fast path (T % 16 == 0), 32 in the generic kernel; a split owns
    steps_per = ceil(ceil(R / BK) / splits) steps"""
    return 16 if c["T"] % 16 == 0 else 32


def wgrad_split_ranges(c, splits):
    R, bk = c["R"], wgrad_bk(c)
    steps = -(-R // bk)
    per = -(-steps // splits)
    return [(min(s * per * bk, R), min((s + 1) * per * bk, R)) for s in range(splits)]


def wgrad_f32_model(GY, X, c, splits, bug=None, absolute=False):
    """P[split][tap][m][n] = sum_{r in split} GY[r, m] * Xm[r + shift(tap), n], shift = (tap - taps/2) * dil, Xm masked as
    the row GEMM's A (x_mask_mode); an empty trailing split is a slab of zeros.  GY [R][ldgy], X [R][ldx] float64."""
    R, T, Mc, Nc, taps = c["R"], c["T"], c["Mc"], c["Nc"], c["taps"]
    mode = c["x_mask_mode"] if bug != "ignore_x_mask" else 0
    P = torch.zeros(splits, taps, Mc, Nc, dtype=torch.float64)
    gy = GY[:, :Mc]
    ranges = wgrad_split_ranges(c, splits)
    last = max(s for s, (lo, hi) in enumerate(ranges) if hi > lo)
    for tap in range(taps):
        src, ok = _frame_map(R, T, c["lens"], mode, (tap - taps // 2) * c["dil"])
        xs = torch.where(ok[:, None], X[src, :Nc], torch.zeros((), dtype=torch.float64))
        for s, (lo, hi) in enumerate(ranges):
            a, b = gy[lo:hi], xs[lo:hi]
            t = (a.abs().T @ b.abs()) if absolute else (a.T @ b)
            P[s, tap] = t * (2 if (bug == "last_split_twice" and s == last and splits > 1) else 1)
    return P


def wgrad_cases():
    cases = []
    i = 0
    mn = ((16, 16), (130, 144), (257, 40))
    td = ((1, 1), (5, 1), (5, 4), (5, 8), (1, 1), (5, 4))
    # fast path: T % 16 == 0; R = 96 = 6 steps of 16, so 5 splits own 2 steps each and the last two are empty
    for T, lens in ((16, [16, 0, 5, 16, 3, 9]), (32, [32, 0, 13])):
        for (Mc, Nc) in mn:
            taps, dil = td[i % 6]
            cases.append(dict(name=f"wgrad16-T{T}-{Mc}x{Nc}", expect=kernel_code(WGRAD16), R=96, T=T, lens=lens, Mc=Mc, Nc=Nc, taps=taps,
                              dil=dil, x_mask_mode=i % 2, real=False))
            i += 1
    # generic path: T % 16 != 0, R no multiple of 32 (111: 4 steps of 32, 5 splits leave one empty; 180: 6 steps, two empty)
    for T, lens in ((37, [37, 0, 11]), (45, [45, 0, 17, 30])):
        for (Mc, Nc) in mn:
            taps, dil = td[(i + 1) % 6]
            cases.append(dict(name=f"wgrad-T{T}-{Mc}x{Nc}", expect=kernel_code(WGRAD), R=T * len(lens), T=T, lens=lens, Mc=Mc, Nc=Nc,
                              taps=taps, dil=dil, x_mask_mode=(i + 1) % 2, real=False))
            i += 1
    return cases


def wgrad_realistic_cases():
    return [dict(name="real-wgrad16", expect=kernel_code(WGRAD16), R=96, T=32, lens=[32, 0, 13], Mc=130, Nc=144, taps=5, dil=4, x_mask_mode=1, real=True),
            dict(name="real-wgrad", expect=kernel_code(WGRAD), R=180, T=45, lens=[45, 0, 17, 30], Mc=130, Nc=144, taps=5, dil=4, x_mask_mode=1, real=True)]


WGRAD_SPLITS = (1, 3, 5)


def build_wgrad(c, poison=True, seed=0):
    g = torch.Generator().manual_seed(4000 + seed + sum(map(ord, c["name"])))
    pad = NAN if poison else 5.0
    p = Problem()
    R, T, Mc, Nc = c["R"], c["T"], c["Mc"], c["Nc"]
    draw = (lambda shape, scale: (torch.randn(shape, generator=g, dtype=torch.float64) * scale * 1.37).float().double()) if c["real"] else \
           (lambda shape, scale: _vals(g, shape, scale))
    p.ldgy, p.ldx = (Mc + 3) // 4 * 4 + 4, (Nc + 3) // 4 * 4 + 8
    p.GY = _padded(draw((R, Mc), 0.0029 if c["real"] else 1.0), p.ldgy, pad)
    p.X = _padded(draw((R, Nc), 1.0 if c["real"] else 2.0 ** -Q), p.ldx, pad)
    if c["x_mask_mode"]:
        for b in range(R // T):
            p.X[b * T + c["lens"][b]:(b + 1) * T] = pad
    p.P = {s: wgrad_f32_model(p.GY, p.X, c, s) for s in WGRAD_SPLITS}
    p.budget = None
    if not c["real"]:
        p.budget = float(wgrad_f32_model(p.GY, p.X, c, 1, absolute=True).max()) * 2.0 ** Q
    return p


# ---------------------------------------------------------------------------------------------------------------------
# descriptors

def rowgemm_pointer_names(c):
    """the operand / side pointers case c's descriptor carries"""
    names = ["A", "B", "C"]
    names += ["lens"] if c["lens"] is not None else []
    names += [k for k, on in (("bias", c["bias"]), ("add", c["add"]), ("dact_src", c["dact"]), ("C2", c["c2"]),
                              ("c2_src", c["c2"] == "src3"), ("Ch", c["split"]), ("Cl", c["split"])) if on]
    return names


def rowgemm_desc(c, p, ptrs):
    """keywords of rad_mmm_amd._lib.rowgemm / rowgemm_plan for case c on problem p (build_rowgemm has filled in the pitches);
    ptrs: name -> tensor (or, for the plan query, any 16-byte aligned address) for rowgemm_pointer_names(c); c2_src a list of 3"""
    kw = dict(lda=c["lda"], a_item_stride=c["a_item_stride"], ldb=c["ldb"], b_tap_stride=c["b_tap_stride"], b_layout=c["b_layout"],
              ldc=p.ldc, M=c["M"], N=c["N"], K=c["K"], taps=c["taps"], dil=c["dil"], sign=c["sign"], T=c["T"], a_mask_mode=c["a_mask_mode"],
              pconv=c["pconv"], premask=c["premask"], postmask=c["postmask"], ratio_taps=c["ratio_taps"], ratio_dil=c["ratio_dil"],
              dact=c["dact"], rowscale=c["rowscale"], act=c["act"])
    if c["add"]:
        kw["ldadd"] = p.ldside
    if c["dact"]:
        kw["lddact"] = p.ldside
    if c["c2"]:
        kw.update(ldc2=p.ldside, c2_accum=1 if c["c2"] == "accum" else 0)
    if c["split"]:
        kw.update(ldch=p.ldch, ch_scale=c["ch_scale"], split_fmt=SPLIT_F16)
    for k in rowgemm_pointer_names(c):
        kw[k] = ptrs[k]
    return kw


def wgrad_desc(c, p, splits, ldp, split_stride, ptrs):
    kw = dict(ldgy=p.ldgy, ldx=p.ldx, ldp=ldp, split_stride=split_stride, R=c["R"], Mc=c["Mc"], Nc=c["Nc"], taps=c["taps"], dil=c["dil"],
              T=c["T"], x_mask_mode=c["x_mask_mode"], splits=splits)
    kw.update(ptrs)
    return kw
