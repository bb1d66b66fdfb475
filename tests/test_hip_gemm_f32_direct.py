"""The fp32 GEMM family (radmmm_rowgemm_f32, radmmm_wgrad_f32: 21 kernels) held to the float64 host model of
tests/_gemm_f32_ref.py through the C ABI.

Exact cases: operands of small signed integers times powers of two, so every fp32 sum a kernel can form is exact (the bit
budget is asserted below 2^24 on the host before the launch) and C, C2, the split copy Ch / Cl and every slab of P must
equal the model WORD FOR WORD, whatever the tile height, the k order or the split.  Every input holds a quiet NaN where a
kernel must not look, every output starts as a pattern that must survive outside [M][N].  Every case asserts, before it
launches, that its descriptor reaches the kernel it is about (radmmm_rowgemm_f32_plan / radmmm_wgrad_f32_plan); no debug
switch is set, the table reaches all 21 kernels by shape alone (tests/test_gemm_f32_ref_cpu.py proves that without a GPU).

Realistic cases, one per family: Gaussian operands at scales that are no powers of two, every element within
n * 2^-23 * sum |a||b| of the float64 model (_gemm_ref.accumulation_bar).  Inexact epilogue steps (pconv, rowscale 2, leaky
act / dact) on exact accumulators: every element within r * 2^-24 * (|v| * ratio + |bias| + |add|), r roundings counted in
the table.  The largest ratios of error to bar are printed."""
import pytest
import torch

import _gemm_f32_ref as F
from _gemm_ref import FILL16

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PAD_ROWS = 3
ROWS16_CASES, GENERIC_CASES, MIX_CASES = F.rows16_cases(), F.generic_cases(), F.mix_cases()
INEXACT_CASES, REAL_CASES = F.inexact_cases(), F.realistic_cases()
WG_CASES, WG_REAL_CASES = F.wgrad_cases(), F.wgrad_realistic_cases()
_ids = lambda c: c["name"]


def _sync():
    """wait for the launch; a device error ends the session (nothing more is launched on a device that has faulted)"""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error after a launch of this file, stopping: {e}", returncode=3)


def _filled32(rows, ld):
    return torch.full((rows, ld), F.FILL32, dtype=torch.int32, device=DEV)


def _filled16(rows, ld):
    return torch.full((rows, ld), FILL16, dtype=torch.int16, device=DEV)


def _assert_words(name, got, want):
    """word-for-word equality with a report of WHERE it fails: which rows, columns, and how many"""
    got, want = F.words(got.cpu()), F.words(want.cpu())
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = (got != want).nonzero()
    if bad.numel():
        r, c = bad[:, 0], bad[:, 1]
        some = [(int(a), int(b), hex(int(got[a, b]) & 0xffffffff), hex(int(want[a, b]) & 0xffffffff)) for a, b in bad[:6].tolist()]
        raise AssertionError(f"{name}: {bad.shape[0]} of {got.numel()} words differ; rows {int(r.min())}..{int(r.max())} "
                             f"({r.unique().numel()} distinct), columns {int(c.min())}..{int(c.max())} ({c.unique().numel()} distinct); "
                             f"first (row, col, got, want): {some}")


def _outside_is_fill(name, buf, M, N, fill):
    b = buf.cpu()
    assert bool((b[M:] == fill).all()), f"{name}: rows past M were written"
    assert bool((b[:M, N:] == fill).all()), f"{name}: columns past N were written"


def _dev32(x64):
    return x64.float().to(DEV).contiguous()


def _launch_rowgemm(c, p):
    """one radmmm_rowgemm_f32 launch of case c on problem p, after the plan query has confirmed the kernel; returns the
    output buffers (device) by name"""
    from rad_mmm_amd._lib import rowgemm, rowgemm_plan
    M, N = c["M"], c["N"]
    out = {"C": _filled32(M + PAD_ROWS, p.ldc)}
    ptrs = {"A": _dev32(p.A), "B": _dev32(p.B), "C": out["C"]}
    if c["lens"] is not None:
        ptrs["lens"] = torch.tensor(c["lens"], dtype=torch.int32, device=DEV)
    for k in ("bias", "add", "dact_src"):
        if k in p.side:
            ptrs[k] = _dev32(p.side[k])
    if c["c2"]:
        out["C2"] = _filled32(M + PAD_ROWS, p.ldside)
        ptrs["C2"] = out["C2"]
        if c["c2"] == "accum":
            out["C2"][:M, :N] = p.side["C2"].float().view(torch.int32).to(DEV)
        if c["c2"] == "src3":
            ptrs["c2_src"] = [_dev32(s) for s in p.side["c2_src"]]
    if c["split"]:
        out["Ch"], out["Cl"] = _filled16(M + PAD_ROWS, p.ldch), _filled16(M + PAD_ROWS, p.ldch)
        ptrs.update(Ch=out["Ch"], Cl=out["Cl"])
    kw = F.rowgemm_desc(c, p, ptrs)
    code = rowgemm_plan(**kw)
    assert code == c["expect"], f"the descriptor reaches kernel {code}, the case is about {c['expect']}"
    rowgemm(**kw)
    _sync()
    return out


def _run_exact(c):
    p = F.build_rowgemm(c)
    assert p.budget < F.BUDGET, "the case leaves its bit budget: equality would not be a fair demand"
    out = _launch_rowgemm(c, p)
    M, N = c["M"], c["N"]
    _assert_words("C", out["C"][:M, :N], F.words(p.C))
    _outside_is_fill("C", out["C"], M, N, F.FILL32)
    if c["c2"]:
        _assert_words("C2", out["C2"][:M, :N], F.words(p.C2))
        _outside_is_fill("C2", out["C2"], M, N, F.FILL32)
    if c["split"]:
        # (the f16 pair store works on 4 columns: it writes zeros into the columns N .. roundup4(N) of a row, rowgemm_epilogue.h
        #  store_split4)
        n4 = (N + 3) // 4 * 4
        for name, want in (("Ch", p.split.hi), ("Cl", p.split.lo)):
            got = out[name].cpu()
            _assert_words(name, got[:M, :N], F.words(want))
            assert bool((got[:M, N:n4] == 0).all())
            _outside_is_fill(name, got, M, n4, FILL16)


@pytest.mark.parametrize("c", ROWS16_CASES, ids=_ids)
def test_rowgemm16_exact(c):
    _run_exact(c)


@pytest.mark.parametrize("c", GENERIC_CASES, ids=_ids)
def test_rowgemm_generic_exact(c):
    _run_exact(c)


@pytest.mark.parametrize("c", MIX_CASES, ids=_ids)
def test_rowgemm_mix_exact(c):
    _run_exact(c)


def _report(name, err, bar, what):
    assert bool((err[bar == 0] == 0).all()), name
    ratio = float((err / bar.clamp_min(1e-300))[bar > 0].max())
    print(f"[gemm-f32-direct] {name}: largest |error| / ({what}) = {ratio:.4f} over {err.numel()} elements")
    assert ratio <= 1.0, (name, ratio)


@pytest.mark.parametrize("c", INEXACT_CASES, ids=_ids)
def test_rowgemm_inexact_epilogue_steps_within_their_rounding_bar(c):
    p = F.build_rowgemm(c)
    assert p.budget < F.BUDGET                                    # the accumulators are exact: the error is the epilogue's alone
    out = _launch_rowgemm(c, p)
    M, N = c["M"], c["N"]
    got = out["C"][:M, :N].cpu().view(torch.float32).double()
    assert bool(torch.isfinite(got).all())
    _outside_is_fill("C", out["C"], M, N, F.FILL32)
    _report(c["name"], (got - p.out64["C"]).abs(), c["r"] * 2.0 ** -24 * p.out64["mag"], f"{c['r']} 2^-24 (|v| ratio + |bias| + |add|)")


@pytest.mark.parametrize("c", REAL_CASES, ids=_ids)
def test_rowgemm_realistic_values_within_the_accumulation_bar(c):
    p = F.build_rowgemm(c)
    out = _launch_rowgemm(c, p)
    M, N, T = c["M"], c["N"], c["T"]
    got = out["C"][:M, :N].cpu().view(torch.float32).double()
    assert bool(torch.isfinite(got).all())
    _outside_is_fill("C", out["C"], M, N, F.FILL32)
    mag = F.rowgemm_f32_acc(p.A, p.B, c, absolute=True)
    taps_valid = sum((F._a_rows(torch.ones_like(p.A), c, s)[:, 0] != 0).long() for s in F.tap_shifts(c["taps"], c["dil"], c["sign"]))
    n = (c["K"] * taps_valid).double()[:, None]
    _report(c["name"], (got - p.out64["C"]).abs(), F.accumulation_bar(n, mag), "n 2^-23 sum|a||b|")


# ---------------------------------------------------------------------------------------------------------------------
# the weight gradient

def _launch_wgrad(c, p, splits, ldp):
    from rad_mmm_amd._lib import wgrad, wgrad_plan
    Mc, Nc, taps = c["Mc"], c["Nc"], c["taps"]
    slab = taps * Mc * ldp
    stride = slab + 64
    P = torch.full((splits * stride + 32,), F.FILL32, dtype=torch.int32, device=DEV)
    ptrs = dict(GY=_dev32(p.GY), X=_dev32(p.X), P=P, lens=torch.tensor(c["lens"], dtype=torch.int32, device=DEV))
    kw = F.wgrad_desc(c, p, splits, ldp, stride, ptrs)
    code = wgrad_plan(**kw)
    assert code == c["expect"], f"the descriptor reaches kernel {code}, the case is about {c['expect']}"
    wgrad(**kw)
    _sync()
    P = P.cpu()
    slabs = torch.stack([P[s * stride: s * stride + slab].view(taps, Mc, ldp) for s in range(splits)])
    # nothing outside the [taps][Mc][Nc] blocks of the slabs may change
    assert bool((slabs[..., Nc:] == F.FILL32).all()), "pad columns of P were written"
    for s in range(splits):
        assert bool((P[s * stride + slab: (s + 1) * stride] == F.FILL32).all()), "the gap between two slabs was written"
    assert bool((P[splits * stride:] == F.FILL32).all())
    return slabs[..., :Nc].contiguous()


@pytest.mark.parametrize("c", WG_CASES, ids=_ids)
def test_wgrad_exact(c):
    p = F.build_wgrad(c)
    assert p.budget < F.BUDGET
    Mc, Nc, taps = c["Mc"], c["Nc"], c["taps"]
    total = F.words(F.to_f32_exact(p.P[1][0])).view(taps * Mc, Nc)
    for splits in F.WGRAD_SPLITS:
        want = F.to_f32_exact(p.P[splits])
        for ldp in (Nc + 4 - Nc % 4, Nc + 5 - Nc % 2):            # ldp % 4 == 0 (16-byte stores) and ldp odd (scalar stores)
            slabs = _launch_wgrad(c, p, splits, ldp)
            for s in range(splits):                               # every slab is the model's slab of the same row range,
                _assert_words(f"P slab {s} of {splits}, ldp {ldp}", slabs[s].view(taps * Mc, Nc), F.words(want[s]).view(taps * Mc, Nc))
            vals = slabs.view(torch.float32).double().sum(0)     # an empty trailing split a slab of zeros, and the sum THE value
            _assert_words(f"P summed over {splits} split(s), ldp {ldp}", vals.float().view(taps * Mc, Nc), total)


@pytest.mark.parametrize("c", WG_REAL_CASES, ids=_ids)
def test_wgrad_realistic_values_within_the_accumulation_bar(c):
    p = F.build_wgrad(c)
    got = _launch_wgrad(c, p, 1, c["Nc"] + 4 - c["Nc"] % 4)[0].view(torch.float32).double()
    assert bool(torch.isfinite(got).all())
    mag = F.wgrad_f32_model(p.GY, p.X, c, 1, absolute=True)[0]
    live = [F._frame_map(c["R"], c["T"], c["lens"], c["x_mask_mode"], (tap - c["taps"] // 2) * c["dil"])[1].sum() for tap in range(c["taps"])]
    n = torch.stack(live).double()[:, None, None]
    _report(c["name"], (got - p.P[1][0]).abs(), F.accumulation_bar(n, mag), "n 2^-23 sum|a||b|")
