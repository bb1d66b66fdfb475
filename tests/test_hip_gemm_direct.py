"""The split-operand GEMMs held to the host model of tests/_gemm_ref.py through the C ABI.

Exact cases: the operands are built here (not by the producers) from small signed integers times powers of two, so that
every fp32 sum the kernel can form is exact (the case's bit budget is asserted below 2^24 on the host before the launch)
and the output must equal the float64 model BIT FOR BIT, whatever the accumulation order, the tile shape or the matrix
instruction's internals.  Every input is poison where the kernel must not look (columns past K, masked frames, the
neighbouring item, weight rows past N, the gap in front of the extra segment); every output starts as a pattern that
must survive outside [M][N].  Every case asserts the kernel code the launch reports (radmmm_rowgemm_h3_last_kernel), and
that it is the one the host plan names for the same keywords (radmmm_rowgemm_h3_plan): a shape that does not reach its
kernel fails.

Realistic cases, one per kernel family: operands from the producers' model (split_ref) of softplus / Gaussian data at
scales that are no powers of two; every element within n * 2^-23 * sum |a||b| of the float64 model of the decoded
operands (_gemm_ref.accumulation_bar).  The largest ratio of error to bar is printed."""
import pytest
import torch

import _gemm_ref as G
from _split_ref import FILL8, SPLIT_F16, SPLIT_X8A, SPLIT_X8B, e4m3_bytes, pack_cross, split_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROW_CASES = G.rowgemm_cases()
WG_CASES = G.wgrad_cases()
PAD_ROWS = 3


def _sync():
    """wait for the launch; a device error ends the session (nothing more is launched on a device that has faulted)"""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error after a launch of this file, stopping: {e}", returncode=3)


def _filled32(rows, ld):
    return torch.full((rows, ld), G.FILL32, dtype=torch.int32, device=DEV)


def _filled16(rows, ld):
    return torch.full((rows, ld), G.FILL16, dtype=torch.int16, device=DEV)


def _assert_words(name, got, want):
    """word-for-word equality with a report of WHERE it fails: which rows, columns, and how many"""
    got, want = G.words(got.cpu()), G.words(want.cpu())
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


def _a_operand(op, x8):
    hi = op.hi.to(DEV)
    lo = op.cross(SPLIT_X8A).to(DEV) if x8 else op.lo.to(DEV)
    return hi, lo


def _b_operand(op, x8):
    hi = op.hi.to(DEV)
    lo = op.cross(SPLIT_X8B).to(DEV) if x8 else op.lo.to(DEV)
    return hi, lo


def _launch_rowgemm(c, p, monkeypatch):
    """one radmmm_rowgemm_h3 launch of case c on problem p; returns the output buffers (device) by name"""
    from rad_mmm_amd._lib import rowgemm_h3, rowgemm_h3_last_kernel, rowgemm_h3_plan
    for k in G.ROWGEMM_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    M, N = c["M"], c["N"]
    x8 = c["nprod"] == 2
    ldc, ldc2 = G.out_pitches(c)
    out = {"C": _filled32(M + PAD_ROWS, ldc)}
    arr = {"lens": torch.tensor(c["lens"], dtype=torch.int32, device=DEV)}
    arr["Ah"], arr["Al"] = _a_operand(p.A, x8)
    arr["Bh"], arr["Bl"] = _b_operand(p.B, x8)
    if c["bias"]:
        arr["bias"] = p.side["bias"].to(DEV)
    if c["dact"]:
        arr["dact_src"] = p.side["dact_src"].to(DEV).contiguous()
    if c["c2"]:
        out["C2"] = _filled32(M + PAD_ROWS, ldc2)
        if c["c2"] == "accum":
            out["C2"][:M, :N] = p.side["C2"].view(torch.int32).to(DEV)
        if c["c2"] == "src3":
            arr["c2_src"] = []
            for s in p.side["c2_src"]:
                t = torch.full((M, ldc2), 7.0, device=DEV)               # (poison in the pad columns)
                t[:, :N] = s.to(DEV)
                arr["c2_src"].append(t)
    if c["split"]:
        out["Ch"] = _filled16(M + PAD_ROWS, p.ldch)
        out["Cl"] = torch.full((M + PAD_ROWS, 2 * p.ldch), FILL8, dtype=torch.uint8, device=DEV) if x8 else _filled16(M + PAD_ROWS, p.ldch)
        if c["clo"]:
            out["Clo"] = _filled16(M + PAD_ROWS, p.ldch)
    kw = G.rowgemm_kw(c, p, dict(arr, **out))
    rowgemm_h3(**kw)
    code = rowgemm_h3_last_kernel()
    _sync()
    assert rowgemm_h3_plan(**kw) == code, "the launch did not take the kernel the plan names for the same keywords"
    return out, code


def _check_rowgemm_exact(c, p, out):
    M, N = c["M"], c["N"]
    Cw = out["C"]
    _assert_words("C", Cw[:M, :N], G.words(p.C))
    _outside_is_fill("C", Cw, M, N, G.FILL32)
    if c["c2"]:
        _assert_words("C2", out["C2"][:M, :N], G.words(p.C2))
        _outside_is_fill("C2", out["C2"], M, N, G.FILL32)
    if c["split"]:
        s = p.split
        generic_f16 = p.split_fmt == SPLIT_F16 and (c["expect"] % 10) == G.EK_GENERIC
        # (the generic epilogue's f16 pair store works on 4 columns: it writes zeros into the columns N .. roundup4(N) of a row,
        #  rowgemm_epilogue.h store_split4; every other store leaves them alone)
        n4 = (N + 3) // 4 * 4 if generic_f16 else N
        hi = out["Ch"].cpu()
        _assert_words("Ch", hi[:M, :N], G.words(s.hi))
        assert bool((hi[:M, N:n4] == 0).all())
        _outside_is_fill("Ch", hi, M, n4, G.FILL16)
        if p.split_fmt == SPLIT_F16:
            lo = out["Cl"].cpu()
            _assert_words("Cl", lo[:M, :N], G.words(s.lo))
            assert bool((lo[:M, N:n4] == 0).all())
            _outside_is_fill("Cl", lo, M, n4, G.FILL16)
        else:
            by = out["Cl"].cpu()
            want = pack_cross(s.hi8, s.lo8, p.split_fmt, p.ldch, fill=FILL8)
            _assert_words("Cl (8-bit cross array)", G.words(by[:M]), G.words(want))
            assert bool((by[M:] == FILL8).all()), "cross array: rows past M were written"
        if c["clo"]:
            lo16 = out["Clo"].cpu()
            _assert_words("Clo", lo16[:M, :N], G.words(s.lo))
            _outside_is_fill("Clo", lo16, M, N, G.FILL16)


@pytest.mark.parametrize("c", ROW_CASES, ids=[c["name"] for c in ROW_CASES])
def test_rowgemm_h3_exact(c, monkeypatch):
    p = G.build_rowgemm(c)
    assert p.budget < G.BUDGET and p.grid_ok, "the case leaves its bit budget: equality would not be a fair demand"
    out, code = _launch_rowgemm(c, p, monkeypatch)
    assert code == c["expect"], f"the launch took kernel {code}, the case is about {c['expect']}"
    _check_rowgemm_exact(c, p, out)


# ---------------------------------------------------------------------------------------------------------------------
# the weight gradients

def _poison_cross(op, g):
    """cross array of a radmmm_wgrad_rm8 operand: the lo8 halves are the operand's, the hi8 halves are poison (the kernel
    derives hi8 from the fp16 plane in registers and must not read them)"""
    junk = e4m3_bytes(torch.randint(1, 4, op.hi8.shape, generator=g).float() * 3.0)
    return pack_cross(junk, op.lo8, SPLIT_X8A, op.ld)


def _launch_wgrad(c, p, splits, operands=None):
    from rad_mmm_amd._lib import check, lib, ptr, stream
    Mc, Nc, taps = c["Mc"], c["Nc"], c["taps"]
    ldp = Nc + 5
    slab = taps * Mc * ldp
    stride = slab + 64
    P = torch.full((splits * stride + 32,), G.FILL32, dtype=torch.int32, device=DEV)
    lens = torch.tensor(c["lens"], dtype=torch.int32, device=DEV)
    kind = c["kind"]
    g = torch.Generator().manual_seed(5)
    if kind in ("rm", "rm8", "rmh"):
        gh, xh = p.GY.hi.to(DEV), p.X.hi.to(DEV)
        if kind == "rm":
            gl, xl = p.GY.lo.to(DEV), p.X.lo.to(DEV)
            check(lib.radmmm_wgrad_rm(ptr(gh), ptr(gl), p.ldg, ptr(xh), ptr(xl), p.ldx, c["R"], c["T"], ptr(lens), c["x_mask"], ptr(P), ldp,
                                      stride, Mc, Nc, taps, c["dil"], splits, c["acc_scale"], stream()), "wgrad_rm")
        elif kind == "rm8":
            gx, xx = _poison_cross(p.GY, g).to(DEV), _poison_cross(p.X, g).to(DEV)
            check(lib.radmmm_wgrad_rm8(ptr(gh), ptr(gx), p.ldg, c["g8_exp"], ptr(xh), ptr(xx), p.ldx, c["x8_exp"], c["R"], c["T"], ptr(lens),
                                       c["x_mask"], ptr(P), ldp, stride, Mc, Nc, taps, c["dil"], splits, c["acc_scale"], stream()), "wgrad_rm8")
        else:
            check(lib.radmmm_wgrad_rmh(ptr(gh), p.ldg, ptr(xh), p.ldx, c["R"], c["T"], ptr(lens), c["x_mask"], ptr(P), ldp, stride, Mc, Nc,
                                       taps, c["dil"], splits, c["acc_scale"], stream()), "wgrad_rmh")
    else:
        dev = lambda t: t.half().to(DEV).contiguous()
        gh, gl = dev(p.GYt["hi"]), dev(p.GYt["lo"])
        xh, xl = dev(p.Xt["hi"]), dev(p.Xt["lo"])
        x1h, x1l = dev(G.advanced(p.Xt["hi"])), dev(G.advanced(p.Xt["lo"]))
        if c["nprod"] == 1:                                       # one product: the lo planes must not be read
            gl, xl, x1l = (torch.full_like(t, 3.0) for t in (gl, xl, x1l))
        check(lib.radmmm_wgrad_h3(ptr(gh), ptr(gl), ptr(xh), ptr(xl), ptr(x1h), ptr(x1l), p.ldk, c["k0"], c["Kt"], ptr(P), ldp, stride, Mc,
                                  Nc, taps, c["dil"], splits, c["acc_scale"], c["nprod"], stream()), "wgrad_h3")
    _sync()
    P = P.cpu()
    slabs = torch.stack([P[s * stride: s * stride + slab].view(taps, Mc, ldp) for s in range(splits)])
    # nothing outside the [taps][Mc][Nc] blocks of the slabs may change
    assert bool((slabs[..., Nc:] == G.FILL32).all()), "pad columns of P were written"
    for s in range(splits):
        assert bool((P[s * stride + slab: (s + 1) * stride] == G.FILL32).all()), "the gap between two slabs was written"
    assert bool((P[splits * stride:] == G.FILL32).all())
    return slabs[..., :Nc].contiguous()


@pytest.mark.parametrize("c", WG_CASES, ids=[c["name"] for c in WG_CASES])
def test_wgrad_exact(c):
    c = dict(c)
    p = G.build_wgrad(c)
    assert p.budget < G.BUDGET
    want = G.words(p.P).view(c["taps"] * c["Mc"], c["Nc"])
    sums = {}
    for splits in (1, 3):
        slabs = _launch_wgrad(c, p, splits)
        vals = slabs.view(torch.float32)
        assert bool(torch.isfinite(vals).all()), "a slab element was not written"
        # every partial sum is exact, so is the float64 sum of the slabs: it must be THE value
        total = vals.double().sum(0).float()
        assert torch.equal(total.double(), vals.double().sum(0))
        sums[splits] = G.words(total).view(c["taps"] * c["Mc"], c["Nc"])
        _assert_words(f"P summed over {splits} split(s)", sums[splits], want)
    assert torch.equal(sums[1], sums[3])


# ---------------------------------------------------------------------------------------------------------------------
# realistic values

def _softplus_rows(g, rows, cols):
    return torch.nn.functional.softplus(torch.randn(rows, cols, generator=g) * 2)


def _report(name, err, bar):
    assert bool((err[bar == 0] == 0).all())
    ratio = float((err / bar.clamp_min(1e-300))[bar > 0].max())
    print(f"[gemm-direct] {name}: largest |error| / (n 2^-23 sum|a||b|) = {ratio:.4f} over {err.numel()} elements")
    assert ratio <= 1.0, (name, ratio)


REAL_ROW = [
    dict(name="real-narrow-p3", expect=G.kernel_code(G.H3_NARROW, 3, 4, 0), nprod=3, taps=3, dil=2, env={"RADMMM_H3_TILE": "128"}, N=150, T=97),
    dict(name="real-h3d-p2", expect=G.kernel_code(G.H3_H3D, 2, 7, G.EK_PLAIN), nprod=2, taps=3, dil=2,
         env=dict(G._WIDE_OFF, RADMMM_H3W_MB="7"), N=290, T=97),
    dict(name="real-h3d-p3", expect=G.kernel_code(G.H3_H3D, 3, 6, G.EK_PLAIN), nprod=3, taps=3, dil=1,
         env=dict(G._WIDE_OFF, RADMMM_H3W_MB="6"), N=290, T=97),
    dict(name="real-h3d-p1", expect=G.kernel_code(G.H3_H3D, 1, 5, G.EK_PLAIN), nprod=1, taps=5, dil=1,
         env=dict(G._WIDE_OFF, RADMMM_H3W_MB="5"), N=290, T=97),
    dict(name="real-win-p2", expect=G.kernel_code(G.H3_WIN, 2, 7, G.EK_PLAIN), nprod=2, taps=5, dil=2,
         env={"RADMMM_H3_TILE": "256", "RADMMM_H3W_MB": "7"}, N=290, T=225),
    dict(name="real-one-p2", expect=G.kernel_code(G.H3_ONE, 2, 7, G.EK_PLAIN), nprod=2, taps=1, dil=1,
         env={"RADMMM_H3_TILE": "256", "RADMMM_H3W_MB": "7"}, N=290, T=97),
]


@pytest.mark.parametrize("r", REAL_ROW, ids=[r["name"] for r in REAL_ROW])
def test_rowgemm_h3_realistic_values_within_the_accumulation_bar(r, monkeypatch):
    import numpy as np
    T = r["T"]
    a_scale, w_scale = 0.83, 200.0                                 # no powers of two
    acc_scale = float(np.float32(1.0) / (np.float32(a_scale) * np.float32(w_scale)))
    c = G._case(name=r["name"], expect=r["expect"], nprod=r["nprod"], taps=r["taps"], dil=r["dil"], sign=1, a_mask_mode=1, T=T,
                lens=[T, 1, T - 9], N=r["N"], K=128, a8_exp=G.X8_ACT_EXP, b8_exp=G.X8_W_EXP, acc_scale=acc_scale, env=r["env"])
    g = torch.Generator().manual_seed(77)
    x8 = c["nprod"] == 2
    p = G.RowGemmProblem()
    p.lda, p.ldb, p.Nalloc, p.side, p.split = 128, 128, c["N"], {}, None
    p.A = G.realistic_split(_softplus_rows(g, c["M"], 128), a_scale, SPLIT_X8A if x8 else SPLIT_F16, c["a8_exp"])
    p.B = G.realistic_split(torch.randn(c["taps"] * c["N"], 128, generator=g) * 0.03, w_scale, SPLIT_X8B if x8 else SPLIT_F16, c["b8_exp"])
    if x8:
        assert not torch.equal(G.e4m3_value(p.A.hi8).double() * 2.0 ** -c["a8_exp"], p.A.d_hi)      # hi8 != hi: the 8-bit rounding is in play
    out, code = _launch_rowgemm(c, p, monkeypatch)
    assert code == c["expect"], (code, c["expect"])
    got = out["C"][:c["M"], :c["N"]].cpu().view(torch.float32).double()
    want = G.rowgemm_acc(p.A, p.B, c) * acc_scale
    mag = G.rowgemm_acc(p.A, p.B, c, absolute=True) * acc_scale
    taps_valid = sum(G._frame_map(c["M"], T, c["lens"], 1, s)[1].long() for s in G.tap_shifts(c["taps"], c["dil"], 1))
    n = (G.n_products(c, 1) * taps_valid).double()[:, None]
    _outside_is_fill("C", out["C"], c["M"], c["N"], G.FILL32)
    _report(r["name"], (got - want).abs(), G.accumulation_bar(n, mag))


@pytest.mark.parametrize("kind", ["rm", "rm8", "rmh", "h3"])
def test_wgrad_realistic_values_within_the_accumulation_bar(kind):
    c = dict(name=f"real-wgrad-{kind}", kind=kind, taps=3, dil=2, T=45, lens=[45, 1, 17, 30], R=180, x_mask=1, Mc=264, Nc=40,
             g8_exp=G.X8_GRAD_EXP, x8_exp=G.X8_ACT_EXP, lo_log2=None)
    g_scale, x_scale = 1900.0, 0.83
    import numpy as np
    c["acc_scale"] = float(np.float32(1.0) / (np.float32(g_scale) * np.float32(x_scale)))
    g = torch.Generator().manual_seed(78)
    gy = torch.randn(c["R"], c["Mc"], generator=g) * 3e-3
    x = _softplus_rows(g, c["R"], c["Nc"])
    p = G.WgradProblem()
    B = c["R"] // c["T"]
    per = {"rm": 3, "rm8": 3, "rmh": 1, "h3": 3}[kind]
    if kind == "h3":
        c.update(nprod=3)
        p.front, p.Tp = 16, c["T"] + 15
        p.Kt = (B * p.Tp + 31) // 32 * 32
        p.ldk = (p.front + p.Kt + 2 + 7) // 8 * 8
        c.update(k0=p.front, Kt=p.Kt)
        sg, sx = split_ref(gy, g_scale), split_ref(x, x_scale)
        p.GYt = {k: G.wgrad_h3_layout(getattr(sg, k).double(), B, c["T"], p.Tp, p.front, p.ldk) for k in ("hi", "lo")}
        p.Xt = {k: G.wgrad_h3_layout(getattr(sx, k).double(), B, c["T"], p.Tp, p.front, p.ldk, c["lens"]) for k in ("hi", "lo")}
        want, mag = G.wgrad_h3_model(p.GYt, p.Xt, c), G.wgrad_h3_model(p.GYt, p.Xt, c, absolute=True)
    else:
        p.ldg, p.ldx = 288, 64
        pad = lambda t, ld: torch.cat([t, torch.zeros(t.shape[0], ld - t.shape[1])], 1)
        fmt = SPLIT_X8A if kind == "rm8" else SPLIT_F16
        p.GY = G.realistic_split(pad(gy, p.ldg), g_scale, fmt, c["g8_exp"])
        p.X = G.realistic_split(pad(x, p.ldx), x_scale, fmt, c["x8_exp"])
        if kind == "rm8":                                        # the kernel's hi8 is the re-derived one
            for op, e in ((p.GY, c["g8_exp"]), (p.X, c["x8_exp"])):
                op.d_hi8 = G.e4m3_value(G.rederived_hi8(op.hi, e)).double()
        want, mag = G.wgrad_rows_model(p.GY, p.X, c), G.wgrad_rows_model(p.GY, p.X, c, absolute=True)
    slabs = _launch_wgrad(c, p, 1)
    got = slabs[0].view(torch.float32).double()
    # scalar products entering an element of tap's slab: `per` for every frame whose partner frame is live
    live = [G._frame_map(c["R"], c["T"], c["lens"], 1, (tap - c["taps"] // 2) * c["dil"])[1].sum() for tap in range(c["taps"])]
    n = (per * torch.stack(live)).double()[:, None, None]
    _report(c["name"], (got - want * c["acc_scale"]).abs(), G.accumulation_bar(n, mag * c["acc_scale"]))
