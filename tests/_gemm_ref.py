"""Host model of the CONSUMERS of the split operands (include/radmmm_hip.h: radmmm_rowgemm_h3 and the four weight
gradients radmmm_wgrad_h3 / _rm / _rm8 / _rmh): torch / numpy on the CPU in float64, no GPU, no built library.
tests/test_gemm_ref_cpu.py holds this model to torch.nn.functional.conv1d; tests/test_hip_gemm_direct.py holds the
kernels to the model, BIT FOR BIT.

Why bits can be demanded.  An fp32 accumulator is exact when every term is a multiple of 2^-q and the sum of the terms'
magnitudes stays below 2^(24 - q): every partial sum, in every order, is then a multiple of 2^-q below 2^(24 - q) and so
an fp32 number.  The result does not depend on the accumulation order, on how a matrix instruction adds inside, on the
tile shape or on split-K: it is THE sum.  gen_split builds operands of that kind (small signed integers times powers of
two in each of the arrays), every case computes its bit budget  max over the outputs of sum |terms| * 2^q  and asserts
it below 2^24 before anything is launched.  That is a condition of the method, not a tolerance.

What a kernel must compute, from the header, with A8 / B8 the decoded e4m3 bytes of the cross arrays:
  acc = sum Ah.Bh + sum Ah.Bl + sum Al.Bh                                          nprod 0 / 3
  acc = sum Ah.Bh                                                                  nprod 1
  acc = sum Ah.Bh + 2^-(11 + a8_exp + b8_exp) * sum (Ahi8.Blo8 + Alo8.Bhi8)         nprod 2
over taps and k with the header's shift / item-boundary / length-mask rules, the extra K segment included; then
acc_scale and the epilogue.  Under nprod 2 the hi8 bytes are filled independently of the fp16 hi plane (the operation
is linear in each array), so a kernel that reads one where it should read the other differs.

The sign of a zero is not part of the contract (the header states real arithmetic: "v *= mask"; a kernel may multiply
by 0 or select 0): words() maps -0 to +0 on both sides before words are compared."""
import torch

from _split_ref import SPLIT_F16, SPLIT_X8A, e4m3_bytes, e4m3_value, pack_cross, rederived_hi8, split_ref

BUDGET = 2 ** 24
FILL16 = 0x7777
FILL32 = 0x7fc12345                        # a quiet NaN with a recognisable payload: the fp32 outputs start as this
HI_SET = (0, 1, -1, 2, -2)
LO_MAX = 3
# the project's exponents of the 8-bit parts (rad_mmm_amd/ops.py X8_ACT_EXP / X8_GRAD_EXP / X8_W_EXP; tests/test_gemm_ref_cpu.py
# checks that they still are): this module must import without the built library
X8_ACT_EXP, X8_GRAD_EXP, X8_W_EXP = 2, -4, 0
H3_NARROW, H3_H3D, H3_WIN, H3_ONE = 1, 2, 3, 4
EK_GENERIC, EK_PLAIN, EK_SPLIT, EK_RES, EK_DGRAD = 0, 1, 2, 3, 4


def kernel_code(family, nprod, mb, ek):
    """RADMMM_H3_KERNEL_CODE of the header"""
    return family * 1000 + nprod * 100 + mb * 10 + ek


# ---------------------------------------------------------------------------------------------------------------------
# exactly summable operands

class SplitOperand:
    """one split tensor [rows][ld]: hi / lo fp16 planes, hi8 / lo8 uint8 images of e4m3 bytes (None without x8_exp), and
    the float64 values they decode to (d_hi, d_lo, d_hi8, d_lo8).  lo and lo8 hold the SAME residual r = int * 2^lo_log2
    (lo8 = r * 2^(11 + e), as a producer writes it); hi8 holds integers of its own times 2^e."""
    __slots__ = ("hi", "lo", "hi8", "lo8", "d_hi", "d_lo", "d_hi8", "d_lo8", "x8_exp", "lo_log2", "ld")

    def cross(self, fmt):
        return pack_cross(self.hi8, self.lo8, fmt, self.ld)


def _choice(g, vals, shape):
    v = torch.tensor(vals, dtype=torch.float64)
    return v[torch.randint(0, len(vals), shape, generator=g)]


def gen_split(rows, ld, g, lo_log2=-12, x8_exp=None, hi_set=HI_SET, lo_max=LO_MAX, zero_every=8, hi8_from_hi=False):
    """hi: values of hi_set, zero with probability 1 / zero_every only (never a quarter: a dropped term must show);
    lo: +-1 .. +-lo_max times 2^lo_log2, never zero.  EVERY column up to ld is filled: what lies past a kernel's K is
    poison by construction."""
    s = SplitOperand()
    s.ld, s.x8_exp, s.lo_log2 = ld, x8_exp, lo_log2
    nz = [v for v in hi_set if v != 0]

    def hi_like():
        v = _choice(g, nz, (rows, ld))
        if 0 in hi_set:
            v = v * (torch.randint(0, zero_every, (rows, ld), generator=g) != 0)
        return v

    s.d_hi = hi_like()
    lo_int = _choice(g, [v for v in range(-lo_max, lo_max + 1) if v != 0], (rows, ld))
    s.d_lo = lo_int * 2.0 ** lo_log2
    s.hi, s.lo = s.d_hi.half(), s.d_lo.half()
    assert torch.equal(s.hi.double(), s.d_hi) and torch.equal(s.lo.double(), s.d_lo)
    s.hi8 = s.lo8 = s.d_hi8 = s.d_lo8 = None
    if x8_exp is not None:
        if hi8_from_hi:                                 # radmmm_wgrad_rm8's contract: hi8 re-derived from the fp16 plane
            s.hi8 = rederived_hi8(s.hi, x8_exp)
            s.d_hi8 = e4m3_value(s.hi8).double()
            assert torch.equal(s.d_hi8, s.d_hi * 2.0 ** x8_exp)
        else:
            s.d_hi8 = hi_like() * 2.0 ** x8_exp
            s.hi8 = e4m3_bytes(s.d_hi8.float())
        s.d_lo8 = s.d_lo * 2.0 ** (11 + x8_exp)
        s.lo8 = e4m3_bytes(s.d_lo8.float())
        assert torch.equal(e4m3_value(s.hi8).double(), s.d_hi8) and torch.equal(e4m3_value(s.lo8).double(), s.d_lo8), \
            "value set not representable in e4m3 at this exponent"
    return s


# ---------------------------------------------------------------------------------------------------------------------
# radmmm_rowgemm_h3

def _frame_map(M, T, lens, a_mask_mode, shift):
    """(source row, valid) of every output row for one tap: the shifted frame must lie in the same item and inside
    [0, T) (a_mask_mode 0) or [0, lens[b]) (a_mask_mode 1 with lens)"""
    r = torch.arange(M)
    b, t = r // T, r % T
    lim = torch.full((M,), T, dtype=torch.long)
    if a_mask_mode and lens is not None:
        lim = torch.as_tensor(lens, dtype=torch.long)[b]
    ts = t + shift
    ok = (ts >= 0) & (ts < lim)
    return (b * T + ts.clamp(0, T - 1)), ok


def tap_shifts(taps, dil, sign):
    return [sign * (tap - taps // 2) * dil for tap in range(taps)]


def _contract(A, B, c):
    """sum over taps (and the extra segment) of Am[tap] . B[tap]^T for one pair of decoded arrays: A [rowsA][lda],
    B [ntaps][Nalloc][ldb]"""
    M, N, K, T = c["M"], c["N"], c["K"], c["T"]
    acc = torch.zeros(M, N, dtype=torch.float64)
    for tap, s in enumerate(tap_shifts(c["taps"], c["dil"], c["sign"])):
        src, ok = _frame_map(M, T, c.get("lens"), c.get("a_mask_mode", 0), s)
        Am = A[src, :K] * ok[:, None]
        acc += Am @ B[tap, :N, :K].T
    if c.get("extra_tap"):
        r0 = c["extra_a_rows"]
        acc += A[r0:r0 + M, :K] @ B[c["taps"], :N, :K].T
    return acc


def product_pairs(nprod, a8_exp=0, b8_exp=0):
    """[(A array name, B array name, factor)] of a product scheme"""
    if nprod == 1:
        return [("d_hi", "d_hi", 1.0)]
    if nprod == 2:
        f = 2.0 ** -(11 + a8_exp + b8_exp)
        return [("d_hi", "d_hi", 1.0), ("d_hi8", "d_lo8", f), ("d_lo8", "d_hi8", f)]
    return [("d_hi", "d_hi", 1.0), ("d_hi", "d_lo", 1.0), ("d_lo", "d_hi", 1.0)]


def rowgemm_acc(A, B, c, absolute=False):
    """the accumulator of radmmm_rowgemm_h3 (before acc_scale) in float64.  A: SplitOperand [rowsA][lda]; B: SplitOperand
    whose rows are [ntaps * Nalloc] (tap stride Nalloc * ldb halves).  absolute: sum of the terms' magnitudes instead."""
    nt = c["taps"] + (1 if c.get("extra_tap") else 0)
    acc = 0
    for an, bn, f in product_pairs(c["nprod"], c.get("a8_exp", 0), c.get("b8_exp", 0)):
        a, b = getattr(A, an), getattr(B, bn)
        b = b.view(nt, -1, b.shape[-1])
        if absolute:
            a, b = a.abs(), b.abs()
        acc = acc + f * _contract(a, b, c)
    return acc


def rowgemm_terms(A, B, c, r, n):
    """every scalar term of accumulator element (r, n), one by one, as a 1-D float64 array: an independent path to the
    same sum (tests/test_gemm_ref_cpu.py adds them in random orders in fp32)"""
    nt = c["taps"] + (1 if c.get("extra_tap") else 0)
    K, T = c["K"], c["T"]
    out = []
    for an, bn, f in product_pairs(c["nprod"], c.get("a8_exp", 0), c.get("b8_exp", 0)):
        a = getattr(A, an)
        b = getattr(B, bn).view(nt, -1, getattr(B, bn).shape[-1])
        for tap, s in enumerate(tap_shifts(c["taps"], c["dil"], c["sign"])):
            bi, t = divmod(r, T)
            lim = c["lens"][bi] if (c.get("a_mask_mode", 0) and c.get("lens") is not None) else T
            if 0 <= t + s < lim:
                out.append(f * a[r + s, :K] * b[tap, n, :K])
        if c.get("extra_tap"):
            out.append(f * a[c["extra_a_rows"] + r, :K] * b[c["taps"], n, :K])
    return torch.cat(out) if out else torch.zeros(0, dtype=torch.float64)


def row_mask(M, T, lens):
    r = torch.arange(M)
    if lens is None:
        return torch.ones(M, dtype=torch.float64)
    return ((r % T) < torch.as_tensor(lens, dtype=torch.long)[r // T]).double()


def rowgemm_epilogue(acc, c, side):
    """the header's epilogue steps that are exact, in the header's order: v = acc * acc_scale; premask; bias; postmask;
    dact = ReLU as a 0 / 1 factor of the saved output; rowscale 1; act none; C = v; the second output (C2 accumulate /
    store, or ((src0 + src1) + src2) + v with c2_src).  Returns {"C": .., "C2": ..} in float64."""
    M, T = c["M"], c["T"]
    m = row_mask(M, T, c.get("lens"))[:, None]
    v = acc * c["acc_scale"]
    if c.get("premask"):
        v = v * m
    if side.get("bias") is not None:
        v = v + side["bias"].double()[None, :]
    if c.get("postmask"):
        v = v * m
    if c.get("dact"):
        assert c["dact"] == 2                                    # RADMMM_ACT_RELU: the only derivative that is exact
        v = v * (side["dact_src"].double() > 0).double()
    if c.get("rowscale"):
        assert c["rowscale"] == 1
        v = v * m
    out = {"C": v}
    if c.get("c2") == "accum":
        out["C2"] = side["C2"].double() + v
    elif c.get("c2") == "store":
        out["C2"] = v.clone()
    elif c.get("c2") == "src3":
        s = side["c2_src"]
        out["C2"] = ((s[0].double() + s[1].double()) + s[2].double()) + v
    return out


def words(t):
    """bit image of an fp32 / fp16 / uint8-e4m3 tensor (or its integer view) as integers, -0 mapped to +0 (module docstring)"""
    if t.dtype in (torch.float32, torch.int32):
        w = t.contiguous().view(torch.int32).clone()
        w[w == -2 ** 31] = 0
    elif t.dtype in (torch.float16, torch.int16):
        w = t.contiguous().view(torch.int16).clone()
        w[w == -2 ** 15] = 0
    else:
        assert t.dtype == torch.uint8
        w = t.clone()
        w[w == 0x80] = 0
    return w


def to_f32_exact(x64):
    x = x64.float()
    assert torch.equal(x.double(), x64), "the model's value is not an fp32 number: the case is outside its budget"
    return x


# --- the cases -------------------------------------------------------------------------------------------------------

def _case(**kw):
    c = dict(taps=1, dil=1, sign=1, a_mask_mode=0, extra_tap=0, a8_exp=0, b8_exp=0, lo_log2=-12, acc_scale=2.0 ** -8,
             premask=0, postmask=0, rowscale=0, dact=0, bias=False, c2=None, split=False, clo=False, ch_scale=1.0, ch_x8_exp=0,
             odd_ldc=False, env={})
    c.update(kw)
    c["M"] = len(c["lens"]) * c["T"]
    if c["extra_tap"]:
        c["extra_a_rows"] = c["M"] + 5                           # a gap of poison rows between the two matrices
    if c["split"] and c["nprod"] == 2:
        c["ch_x8_exp"] = c["a8_exp"]
    return c


# the switches a case's `env` may set: a test clears them all before it applies a case's (RADMMM_DEBUG=1 is the session's)
ROWGEMM_SWITCHES = ("RADMMM_H3_TILE", "RADMMM_H3W_MB", "RADMMM_SLOT3", "RADMMM_WIN", "RADMMM_ONE", "RADMMM_WIN_XT", "RADMMM_H3_1X1")
_WIDE_OFF = {"RADMMM_H3_TILE": "256", "RADMMM_SLOT3": "0", "RADMMM_WIN": "0", "RADMMM_ONE": "0"}
_EXPS = [(X8_ACT_EXP, X8_W_EXP, 2.0 ** -8), (X8_GRAD_EXP, X8_W_EXP, 2.0 ** -19), (-3, 1, 2.0 ** -10), (1, -2, 2.0 ** -6)]
_EK_NAME = {EK_GENERIC: "generic", EK_PLAIN: "plain", EK_SPLIT: "split", EK_RES: "res", EK_DGRAD: "dgrad"}


def _epilogue_of(ek, i, nprod):
    """descriptor options that make the launcher pick epilogue kind ek (rowgemm_h3w.hip pick_h3w_ek)"""
    if ek == EK_GENERIC:          # odd pitch of C: no direct kernel takes it; every option at once
        return dict(odd_ldc=True, bias=True, postmask=1, split=True, c2="accum" if i % 2 else "store")
    if ek == EK_PLAIN:
        return dict(bias=bool(i % 2), premask=i % 2, postmask=(i // 2) % 2)
    if ek == EK_SPLIT:
        return dict(split=True, bias=True, postmask=1, clo=(nprod == 2 and i % 2 == 0), ch_scale=1.0)
    if ek == EK_RES:
        return dict(bias=True, c2=("accum", "store", "src3")[i % 3])
    return dict(split=True, dact=2, rowscale=1, ch_scale=2048.0, clo=(nprod == 2 and i % 2 == 1))


def rowgemm_cases():
    """the matrix of tests/test_hip_gemm_direct.py: (kernel family, products, tile height, epilogue kind) x shapes at the
    edges.  Every case names the kernel code the launch must report."""
    cases = []
    i = 0
    # the 128 x 128 kernel: products 3 and 1, taps 1 / 3 / 5, both signs, both mask modes
    for nprod in (3, 1):
        for taps in (1, 3, 5):
            for sign in (1, -1):
                for mask in (0, 1):
                    i += 1
                    cases.append(_case(name=f"narrow-p{nprod}-t{taps}-s{sign}-m{mask}", expect=kernel_code(H3_NARROW, nprod, 4, 0),
                                       nprod=nprod, taps=taps, sign=sign, a_mask_mode=mask, dil=(1, 2, 8)[i % 3], T=97,
                                       lens=[97, 1, 40, 3], N=150, K=(64, 128)[i % 2], bias=True, postmask=i % 2, split=bool(i % 3 == 0),
                                       lo_log2=(-12, -10, -13)[i % 3] if taps < 5 else -12, env={"RADMMM_H3_TILE": "128"}))
    # rowgemm_h3d: products 1 / 2 / 3 x tile heights x the five epilogue kinds
    for nprod in (1, 2, 3):
        for mb in (4, 5, 6, 7, 8):
            for ek in (EK_GENERIC, EK_PLAIN, EK_SPLIT, EK_RES, EK_DGRAD):
                i += 1
                a8, b8, sc = _EXPS[i % 4] if nprod == 2 else (0, 0, (2.0 ** -8, 2.0 ** -19)[i % 2])
                taps = (1, 3, 5)[i % 3]
                cases.append(_case(name=f"h3d-p{nprod}-mb{mb}-{_EK_NAME[ek]}", expect=kernel_code(H3_H3D, nprod, mb, ek), nprod=nprod,
                                   taps=taps, sign=(1, -1)[(i // 3) % 2], a_mask_mode=(i // 2) % 2, dil=(1, 2, 8)[(i // 3) % 3],
                                   T=97, lens=[97, 1, 40, 3] if i % 2 else [3, 97, 1], N=290, K=(64, 128)[i % 2], a8_exp=a8, b8_exp=b8,
                                   acc_scale=sc, env=dict(_WIDE_OFF, RADMMM_H3W_MB=str(mb)), **_epilogue_of(ek, i, nprod)))
    for nprod in (2, 3):            # the extra K segment
        for mb, ek in ((4, EK_DGRAD), (7, EK_PLAIN), (8, EK_GENERIC)):
            i += 1
            a8, b8, sc = _EXPS[i % 2] if nprod == 2 else (0, 0, 2.0 ** -19)
            cases.append(_case(name=f"h3d-p{nprod}-mb{mb}-{_EK_NAME[ek]}-extra", expect=kernel_code(H3_H3D, nprod, mb, ek), nprod=nprod,
                               taps=(5, 3)[i % 2], sign=-1, dil=(2, 1)[i % 2], T=97, lens=[97, 1, 40, 3], N=290, K=128, a8_exp=a8, b8_exp=b8,
                               acc_scale=sc, extra_tap=1, env=dict(_WIDE_OFF, RADMMM_H3W_MB=str(mb)), **_epilogue_of(ek, i, nprod)))
    # rowgemm_win: 5 taps, T = 32 mb exactly and one more, dilations 1 / 2 / 8
    win_env = {"RADMMM_H3_TILE": "256"}
    for mb in (7, 8):
        for T in (32 * mb, 32 * mb + 1):
            for nprod, ek, extra in ((2, EK_PLAIN, 0), (2, EK_SPLIT, 0), (2, EK_DGRAD, 0), (2, EK_DGRAD, 1), (3, EK_PLAIN, 0)):
                i += 1
                a8, b8, sc = _EXPS[i % 4] if nprod == 2 else (0, 0, 2.0 ** -8)
                cases.append(_case(name=f"win-p{nprod}-mb{mb}-T{T}-{_EK_NAME[ek]}" + ("-extra" if extra else ""),
                                   expect=kernel_code(H3_WIN, nprod, mb, ek), nprod=nprod, taps=5, sign=(1, -1)[i % 2],
                                   a_mask_mode=0 if extra else (i // 2) % 2, dil=(1, 2, 8)[i % 3], T=T, lens=[T, 1, 3] if i % 2 else [3, T - 3, 1],
                                   N=290, K=(64, 128)[i % 2] if not extra else 64, a8_exp=a8, b8_exp=b8, acc_scale=sc, extra_tap=extra,
                                   env=dict(win_env, RADMMM_H3W_MB=str(mb)), **_epilogue_of(ek, i, nprod)))
    # rowgemm_one: 1 tap
    for mb in (4, 5, 6, 7, 8):
        for ek, sub in ((EK_PLAIN, 0), (EK_SPLIT, 0), (EK_RES, 0), (EK_RES, 1), (EK_RES, 2), (EK_DGRAD, 0)):
            i += 1
            a8, b8, sc = _EXPS[i % 4]
            cases.append(_case(name=f"one-p2-mb{mb}-{_EK_NAME[ek]}{sub}", expect=kernel_code(H3_ONE, 2, mb, ek), nprod=2, taps=1,
                               a_mask_mode=i % 2, T=97, lens=[97, 1, 40, 3] if i % 2 else [3, 97, 1], N=290, K=(64, 128)[(i // 2) % 2],
                               a8_exp=a8, b8_exp=b8, acc_scale=sc, lo_log2=(-12, -13, -10)[i % 3],
                               env={"RADMMM_H3_TILE": "256", "RADMMM_H3W_MB": str(mb)}, **_epilogue_of(ek, sub if ek == EK_RES else i, 2)))
    for mb in (7, 8):
        i += 1
        cases.append(_case(name=f"one-p3-mb{mb}-plain", expect=kernel_code(H3_ONE, 3, mb, EK_PLAIN), nprod=3, taps=1, a_mask_mode=1,
                           T=97, lens=[97, 1, 40, 3], N=290, K=(64, 128)[i % 2], env={"RADMMM_H3_TILE": "256", "RADMMM_H3W_MB": str(mb)},
                           **_epilogue_of(EK_PLAIN, i, 3)))
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    return cases


class RowGemmProblem:
    """operands, side inputs, expected outputs and bit budget of one case"""


def _ints(g, shape, lim, scale):
    v = torch.randint(1, lim + 1, shape, generator=g).double() * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    return (v * scale).float()


def rowgemm_layout(c):
    """pitches and formats of case c's arrays (a RowGemmProblem without data: what the descriptor says about them)"""
    p = RowGemmProblem()
    p.lda = c["K"] + 32
    p.ldb = c["K"] + 64
    p.Nalloc = c["N"] + 3                                        # B rows >= N of every tap are poison
    if c["split"]:
        p.split_fmt = SPLIT_X8A if c["nprod"] == 2 else SPLIT_F16
        p.ldch = ((c["N"] + 31) // 32) * 32 + 32
    return p


def out_pitches(c):
    """(ldc, ldc2) of a launch of case c"""
    return c["N"] + (7 if c["odd_ldc"] else 6), (c["N"] + 3) // 4 * 4 + 4


def rowgemm_operands(c):
    """names of the arrays a launch of case c takes (c2_src: a list of three)"""
    names = ["Ah", "Al", "Bh", "Bl", "lens", "C"]
    names += ["bias"] if c["bias"] else []
    names += ["dact_src"] if c["dact"] else []
    names += ["C2"] if c["c2"] else []
    names += ["c2_src"] if c["c2"] == "src3" else []
    names += ["Ch", "Cl"] if c["split"] else []
    names += ["Clo"] if c["split"] and c["clo"] else []
    return names


def standin_addresses(c):
    """an aligned address per array of case c, for the host-only plan query (it never looks behind a pointer)"""
    arr = {name: 0x10000 + 0x1000 * i for i, name in enumerate(rowgemm_operands(c))}
    if "c2_src" in arr:
        arr["c2_src"] = [arr["c2_src"] + 0x100 * k for k in range(3)]
    return arr


def rowgemm_kw(c, p, arr):
    """keywords of rad_mmm_amd._lib.rowgemm_h3 / rowgemm_h3_plan for case c with the layout of p (rowgemm_layout, or a problem
    with pitches of its own) on the arrays arr[name]: device tensors for a launch, anything with an address for the plan"""
    assert sorted(arr) == sorted(rowgemm_operands(c))
    ldc, ldc2 = out_pitches(c)
    kw = dict(Ah=arr["Ah"], Al=arr["Al"], lda_h=p.lda, Bh=arr["Bh"], Bl=arr["Bl"], ldb_h=p.ldb, b_tap_stride_h=p.Nalloc * p.ldb,
              acc_scale=c["acc_scale"], nprod=c["nprod"], a8_exp=c["a8_exp"], b8_exp=c["b8_exp"], extra_tap=c["extra_tap"],
              extra_a_rows=c.get("extra_a_rows", 0), C=arr["C"], ldc=ldc, M=c["M"], N=c["N"], K=c["K"], taps=c["taps"], dil=c["dil"],
              sign=c["sign"], T=c["T"], lens=arr["lens"], a_mask_mode=c["a_mask_mode"], premask=c["premask"], postmask=c["postmask"],
              rowscale=c["rowscale"])
    if c["bias"]:
        kw["bias"] = arr["bias"]
    if c["dact"]:
        kw.update(dact=c["dact"], dact_src=arr["dact_src"], lddact=c["N"])
    if c["c2"]:
        kw.update(C2=arr["C2"], ldc2=ldc2, c2_accum=1 if c["c2"] == "accum" else 0)
        if c["c2"] == "src3":
            kw["c2_src"] = arr["c2_src"]
    if c["split"]:
        kw.update(Ch=arr["Ch"], Cl=arr["Cl"], ldch=p.ldch, ch_scale=c["ch_scale"], split_fmt=p.split_fmt, ch_x8_exp=c["ch_x8_exp"])
        if c["clo"]:
            kw["Clo"] = arr["Clo"]
    return kw


def build_rowgemm(c, seed=0):
    g = torch.Generator().manual_seed(1000 + seed + sum(map(ord, c["name"])))
    p = rowgemm_layout(c)
    M, N, K, T = c["M"], c["N"], c["K"], c["T"]
    x8 = c["nprod"] == 2
    nt = c["taps"] + (1 if c["extra_tap"] else 0)
    rowsA = c["extra_a_rows"] + M + 2 if c["extra_tap"] else M + 4
    p.A = gen_split(rowsA, p.lda, g, c["lo_log2"], c["a8_exp"] if x8 else None)
    p.B = gen_split(nt * p.Nalloc, p.ldb, g, c["lo_log2"], c["b8_exp"] if x8 else None)
    sc = c["acc_scale"]
    side = {}
    if c["bias"]:
        side["bias"] = _ints(g, (N,), 8, sc)
    if c["dact"]:
        side["dact_src"] = _ints(g, (M, N), 3, 0.25)
    if c["c2"] == "accum":
        side["C2"] = _ints(g, (M, N), 8, sc)
    if c["c2"] == "src3":
        side["c2_src"] = [_ints(g, (M, N), 8, sc) for _ in range(3)]
    p.side = side
    acc = rowgemm_acc(p.A, p.B, c)
    out = rowgemm_epilogue(acc, c, side)
    # bit budget: sum of the magnitudes of everything an output element adds up, in units of the finest term
    q = -c["lo_log2"] if c["nprod"] != 1 else 0
    mag = rowgemm_acc(p.A, p.B, c, absolute=True)
    for k in ("bias", "C2"):
        if k in side:
            mag = mag + side[k].double().abs() / sc
    for s in side.get("c2_src", []):
        mag = mag + s.double().abs() / sc
    p.q = q
    p.budget = float(mag.max()) * 2.0 ** q
    p.grid_ok = bool(torch.equal(acc * 2.0 ** q, (acc * 2.0 ** q).round()))
    p.acc = acc
    p.C = to_f32_exact(out["C"]) if p.budget < BUDGET else out["C"].float()
    p.C2 = None
    if "C2" in out:
        p.C2 = to_f32_exact(out["C2"]) if p.budget < BUDGET else out["C2"].float()
    p.split = None
    if c["split"]:
        p.split = split_ref(p.C, c["ch_scale"], p.split_fmt, c["ch_x8_exp"])
    return p


def zero_fraction(op):
    arrs = [op.d_hi, op.d_lo] + ([op.d_hi8, op.d_lo8] if op.d_hi8 is not None else [])
    return max(float((a == 0).double().mean()) for a in arrs)


# ---------------------------------------------------------------------------------------------------------------------
# the weight gradients

def wgrad_rows_model(GY, X, c, absolute=False):
    """radmmm_wgrad_rm / _rm8 / _rmh, summed over the splits, before acc_scale:
    P[tap][m][n] = sum_f GY[f][m] * X[f + s][n], s = (tap - taps/2) * dil, over the frames f = b*T + t whose partner t + s
    lies in [0, T) and, under x_mask, below lens[b].  GY / X: SplitOperand [R][ld].  c["kind"]: "rm" three f16 products,
    "rm8" hi.hi + the cross terms from the lo8 bytes and the hi8 re-derived from the fp16 planes, "rmh" hi.hi alone."""
    R, T, Mc, Nc = c["R"], c["T"], c["Mc"], c["Nc"]
    if c["kind"] == "rm":
        pairs = product_pairs(3)
    elif c["kind"] == "rmh":
        pairs = product_pairs(1)
    else:
        pairs = product_pairs(2, c["g8_exp"], c["x8_exp"])
    lens = c.get("lens") if c.get("x_mask") else None
    P = torch.zeros(c["taps"], Mc, Nc, dtype=torch.float64)
    for gn, xn, f in pairs:
        gy, x = getattr(GY, gn), getattr(X, xn)
        if absolute:
            gy, x = gy.abs(), x.abs()
        for tap in range(c["taps"]):
            s = (tap - c["taps"] // 2) * c["dil"]
            src, ok = _frame_map(R, T, lens, 1 if lens is not None else 0, s)
            Xs = x[src, :Nc] * ok[:, None]
            P[tap] += f * (gy[:, :Mc].T @ Xs)
    return P


def wgrad_rows_terms(GY, X, c, tap, m, n):
    """every scalar term of element (tap, m, n), one by one (the independent path of the order test)"""
    pairs = {"rm": product_pairs(3), "rmh": product_pairs(1)}.get(c["kind"]) or product_pairs(2, c["g8_exp"], c["x8_exp"])
    lens = c.get("lens") if c.get("x_mask") else None
    s = (tap - c["taps"] // 2) * c["dil"]
    src, ok = _frame_map(c["R"], c["T"], lens, 1 if lens is not None else 0, s)
    return torch.cat([f * getattr(GY, gn)[:, m] * getattr(X, xn)[src, n] * ok for gn, xn, f in pairs])


def wgrad_h3_terms(GYt, Xt, c, tap, m, n):
    k0, Kt = c["k0"], c["Kt"]
    s = (tap - c["taps"] // 2) * c["dil"]
    pairs = [("hi", "hi")] if c["nprod"] == 1 else [("hi", "hi"), ("hi", "lo"), ("lo", "hi")]
    return torch.cat([GYt[gn][m, k0:k0 + Kt] * Xt[xn][n, k0 + s:k0 + s + Kt] for gn, xn in pairs])


def wgrad_h3_layout(vals, B, T, Tp, front, ldk, lens=None):
    """radmmm_transpose_split_act's layout of a [B*T][C] matrix: out[c][front + b*Tp + t] = vals[b*T + t][c] for
    t < (lens[b] if lens else T), zeros in the gaps, the front columns and the row tail"""
    Cn = vals.shape[1]
    out = torch.zeros(Cn, ldk, dtype=vals.dtype)
    for b in range(B):
        n = T if lens is None else min(T, lens[b])
        out[:, front + b * Tp: front + b * Tp + n] = vals[b * T: b * T + n].T
    return out


def advanced(xt):
    """the copy advanced by one column: X1[k] = X[k + 1] (odd tap shifts read it at an even offset)"""
    o = torch.zeros_like(xt)
    o[:, :-1] = xt[:, 1:]
    return o


def wgrad_h3_model(GYt, Xt, c, absolute=False):
    """radmmm_wgrad_h3 summed over the splits, before acc_scale, on the TRANSPOSED arrays as the kernel sees them:
    P[tap][m][n] = sum_{k0 <= k < k0 + Kt} GYt[m][k] * Xt[n][k + (tap - taps/2) * dil].  GYt / Xt: dicts of float64
    arrays "hi", "lo" [channels][ldk]."""
    k0, Kt, Mc, Nc = c["k0"], c["Kt"], c["Mc"], c["Nc"]
    pairs = [("hi", "hi")] if c["nprod"] == 1 else [("hi", "hi"), ("hi", "lo"), ("lo", "hi")]
    P = torch.zeros(c["taps"], Mc, Nc, dtype=torch.float64)
    for gn, xn in pairs:
        gy, x = GYt[gn], Xt[xn]
        if absolute:
            gy, x = gy.abs(), x.abs()
        for tap in range(c["taps"]):
            s = (tap - c["taps"] // 2) * c["dil"]
            P[tap] += gy[:Mc, k0:k0 + Kt] @ x[:Nc, k0 + s:k0 + s + Kt].T
    return P


def wgrad_cases():
    cases = []
    i = 0
    # radmmm_wgrad_h3 picks its tile height from Mc alone (wgrad_h3.hip wgrad_mb: the tallest of 256 .. 160 rows that wastes
    # at most a quarter of a tile, else 128): these five reach 128 / 160 / 192 / 224 / 256 rows, each with a partial last tile
    h3_mc = (264, 310, 380, 440, 500)
    for kind in ("rm", "rm8", "rmh", "h3", "h3one"):
        for j, (taps, dil) in enumerate(((1, 1), (3, 1), (3, 2), (5, 3), (5, 4))):
            i += 1
            g8, x8 = ((X8_GRAD_EXP, X8_ACT_EXP), (-2, -3), (1, 0))[i % 3]
            Mc, Nc = ((264, 40), (40, 264))[i % 2]
            if kind in ("h3", "h3one"):
                Mc = h3_mc[j]
            cases.append(dict(name=f"wgrad-{kind}-t{taps}-d{dil}", kind=kind, taps=taps, dil=dil, T=45, lens=[45, 1, 17, 30], R=180,
                              x_mask=i % 2 if taps > 1 else 1, Mc=Mc, Nc=Nc, g8_exp=g8, x8_exp=x8,
                              lo_log2=(-12, -13, -10)[i % 3], acc_scale=(2.0 ** -11, 2.0 ** -19)[i % 2]))
    return cases


class WgradProblem:
    pass


def build_wgrad(c, seed=0):
    g = torch.Generator().manual_seed(2000 + seed + sum(map(ord, c["name"])))
    p = WgradProblem()
    R, T, Mc, Nc = c["R"], c["T"], c["Mc"], c["Nc"]
    B = R // T
    q = 0 if c["kind"] in ("rmh", "h3one") else -c["lo_log2"]
    if c["kind"] in ("rm", "rm8", "rmh"):
        p.ldg, p.ldx = ((Mc + 31) // 32) * 32 + 32, ((Nc + 31) // 32) * 32 + 32
        x8 = c["kind"] == "rm8"
        p.GY = gen_split(R, p.ldg, g, c["lo_log2"], c["g8_exp"] if x8 else None, hi8_from_hi=True)
        p.X = gen_split(R, p.ldx, g, c["lo_log2"], c["x8_exp"] if x8 else None, hi8_from_hi=True)
        P = wgrad_rows_model(p.GY, p.X, c)
        mag = wgrad_rows_model(p.GY, p.X, c, absolute=True)
    else:
        # the transposed, zero-gapped layout: the values of a [B*T][C] matrix, masked by the utterance lengths on the X side
        c.update(nprod=1 if c["kind"] == "h3one" else 3)
        shift = (c["taps"] // 2) * c["dil"]
        p.front = 16
        p.Tp = T + 16 - 1                                        # >= T + the largest shift (12), odd: utterances start anywhere
        p.Kt = ((B * p.Tp + 31) // 32) * 32
        p.ldk = ((p.front + p.Kt + shift + 7) // 8) * 8
        assert p.front >= shift and p.Tp >= T + shift
        c.update(k0=p.front, Kt=p.Kt)
        gy = gen_split(R, Mc, g, c["lo_log2"])
        x = gen_split(R, Nc, g, c["lo_log2"])
        lens = c["lens"] if c["x_mask"] else None
        p.GYt = {k: wgrad_h3_layout(getattr(gy, "d_" + k), B, T, p.Tp, p.front, p.ldk) for k in ("hi", "lo")}
        p.Xt = {k: wgrad_h3_layout(getattr(x, "d_" + k), B, T, p.Tp, p.front, p.ldk, lens) for k in ("hi", "lo")}
        P = wgrad_h3_model(p.GYt, p.Xt, c)
        mag = wgrad_h3_model(p.GYt, p.Xt, c, absolute=True)
    p.q = q
    p.budget = float(mag.max()) * 2.0 ** q
    p.acc = P
    p.P = to_f32_exact(P * c["acc_scale"]) if p.budget < BUDGET else (P * c["acc_scale"]).float()
    return p


# ---------------------------------------------------------------------------------------------------------------------
# realistic values: the per-element bar of an fp32 accumulation

def accumulation_bar(n_products, abs_sum):
    """n * 2^-23 * sum |a||b| per output element: the first-order worst case of ANY order of an fp32 accumulation of n
    products is (n - 1) * 2^-24 * sum |a||b| with round-to-nearest adds; the unit 2^-23 also covers an adder that
    truncates instead of rounding, and the one rounding of the product with acc_scale.  Derived, not tuned."""
    return n_products * 2.0 ** -23 * abs_sum


def realistic_split(x, scale, fmt, x8_exp):
    """SplitOperand of real data through the producers' own model (split_ref): hi8 != hi, residuals of every size"""
    r = split_ref(x, scale, fmt, x8_exp)
    s = SplitOperand()
    s.ld, s.x8_exp, s.lo_log2 = x.shape[1], x8_exp, None
    s.hi, s.lo, s.hi8, s.lo8 = r.hi, r.lo, r.hi8, r.lo8
    s.d_hi, s.d_lo = r.hi.double(), r.lo.double()
    s.d_hi8 = e4m3_value(r.hi8).double() if r.hi8 is not None else None
    s.d_lo8 = e4m3_value(r.lo8).double() if r.lo8 is not None else None
    return s


def n_products(c, r_valid_taps):
    """scalar products entering an element: K per valid tap (and the extra segment) and product"""
    per = {1: 1, 2: 3, 3: 3, 0: 3}[c["nprod"]]
    return per * c["K"] * r_valid_taps
