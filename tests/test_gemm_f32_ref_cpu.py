"""The host model of the fp32 GEMM family (tests/_gemm_f32_ref.py) held to account on the CPU: against
torch.nn.functional.conv1d and autograd in float64 (equality: the values are exact), the bit budget of every exact case, the
kernel every case's descriptor reaches on the built library (radmmm_rowgemm_f32_plan / radmmm_wgrad_f32_plan are host-only:
the table reaches all 21 kernels of the family), and planted-bug controls: every fault of _gemm_f32_ref.ROW_BUGS /
WGRAD_BUGS changes at least one expected word of a case, so the inputs can see it.  No GPU."""
import functools

import pytest
import torch

import _gemm_f32_ref as F

ROW_CASES = F.rowgemm_cases()
INEXACT_CASES = F.inexact_cases()
EXTRA_CASES = INEXACT_CASES + F.realistic_cases()
WG_CASES = F.wgrad_cases()
BY_NAME = {c["name"]: c for c in ROW_CASES + EXTRA_CASES}
ADDR = 0x10000                                             # any 16-byte aligned address: the plan query never looks behind it


@functools.lru_cache(maxsize=None)
def _problem(name, poison=True):
    return F.build_rowgemm(BY_NAME[name], poison=poison)


def _small(**kw):
    c = F._rcase("cpu-" + "-".join(f"{k}{v}" for k, v in sorted(kw.items()) if k != "lens"), 0, M=4 * 29, T=29, N=10, K=32,
                 lens=[29, 1, 3, 17], **kw)
    return c, F.build_rowgemm(c)


def _b_as_conv_weight(p, c):
    """[N][K][taps] from the flat B through the header's addressing"""
    return torch.stack([F._b_tap(p.B, c, tap).T for tap in range(c["taps"])], -1).contiguous()


def _a_matrix(p, c):
    A = p.A.view(c["M"], c["lda"])[:, :c["K"]].clone()
    for b in range(c["M"] // c["T"]):
        lim = c["lens"][b] if c["a_mask_mode"] else c["T"]
        A[b * c["T"] + lim:(b + 1) * c["T"]] = 0             # masking by zeroing the input (this also removes the poison)
    return A


@pytest.mark.parametrize("taps,dil,mask", [(1, 1, 1), (3, 1, 0), (3, 8, 1), (5, 2, 1), (5, 8, 0)])
def test_forward_model_equals_conv1d(taps, dil, mask):
    c, p = _small(taps=taps, dil=dil, a_mask_mode=mask, b_layout=0)
    A, w = _a_matrix(p, c), _b_as_conv_weight(p, c)
    want = torch.zeros(c["M"], c["N"], dtype=torch.float64)
    for b in range(4):
        x = A[b * 29:(b + 1) * 29].T[None]
        want[b * 29:(b + 1) * 29] = torch.nn.functional.conv1d(x, w, padding=(taps // 2) * dil, dilation=dil)[0].T
    assert torch.equal(F.rowgemm_f32_acc(p.A, p.B, c), want)


@pytest.mark.parametrize("taps,dil,mask", [(3, 1, 0), (3, 2, 1), (5, 8, 1), (5, 1, 0)])
def test_data_gradient_model_equals_autograd(taps, dil, mask):
    """sign -1, b_layout 1: A = the output's gradient [frames][Cout = K], B[tap][k = co][n = ci] the forward weight"""
    c, p = _small(taps=taps, dil=dil, a_mask_mode=mask, b_layout=1, sign=-1)
    gy = _a_matrix(p, c)
    w = torch.stack([F._b_tap(p.B, c, tap) for tap in range(taps)], -1).contiguous()            # [co = K][ci = N][taps]
    want = torch.zeros(c["M"], c["N"], dtype=torch.float64)
    for b in range(4):
        x = torch.zeros(1, c["N"], 29, dtype=torch.float64, requires_grad=True)
        y = torch.nn.functional.conv1d(x, w, padding=(taps // 2) * dil, dilation=dil)
        y.backward(gy[b * 29:(b + 1) * 29].T[None])
        want[b * 29:(b + 1) * 29] = x.grad[0].T
    assert torch.equal(F.rowgemm_f32_acc(p.A, p.B, c), want)


@pytest.mark.parametrize("c", WG_CASES, ids=[c["name"] for c in WG_CASES])
def test_weight_gradient_model_equals_autograd(c):
    p = F.build_wgrad(c)
    R, T, Mc, Nc, taps, dil = c["R"], c["T"], c["Mc"], c["Nc"], c["taps"], c["dil"]
    X = p.X[:, :Nc].clone()
    for b in range(R // T):
        X[b * T + (c["lens"][b] if c["x_mask_mode"] else T):(b + 1) * T] = 0
    w = torch.zeros(Mc, Nc, taps, dtype=torch.float64, requires_grad=True)
    for b in range(R // T):
        y = torch.nn.functional.conv1d(X[b * T:(b + 1) * T].T[None], w, padding=(taps // 2) * dil, dilation=dil)
        y.backward(p.GY[b * T:(b + 1) * T, :Mc].T[None])
    want = w.grad.permute(2, 0, 1)
    for splits in F.WGRAD_SPLITS:
        assert torch.equal(p.P[splits].sum(0), want), splits
        ranges = F.wgrad_split_ranges(c, splits)
        assert ranges[0][0] == 0 and max(hi for _, hi in ranges) == R
        for s, (lo, hi) in enumerate(ranges):
            if hi == lo:
                assert not p.P[splits][s].any()                    # an empty trailing split is a slab of zeros
    assert wgrad_has_empty_splits(c)
    assert p.budget < F.BUDGET


def wgrad_has_empty_splits(c):
    r = F.wgrad_split_ranges(c, 5)
    return r[-1][0] == r[-1][1]


def test_framed_model_equals_unfold():
    """a_item_stride with lda < K: item b's frames are its samples unfolded with step lda, T + 1 of them, and a tap reads
    frame T from the last rows"""
    c = BY_NAME["rows16-mt8-bl1"]
    assert c["framed"]
    p = _problem(c["name"])
    M, T, K, N = c["M"], c["T"], c["K"], c["N"]
    assert c["lda"] < K and all(x == T + 1 for x in c["lens"])
    want = torch.zeros(M, N, dtype=torch.float64)
    for b in range(M // T):
        frames = p.A[b * c["a_item_stride"]:].unfold(0, K, c["lda"])[:T + 1]
        for tap, s in enumerate(F.tap_shifts(c["taps"], c["dil"], c["sign"])):
            for t in range(T):
                if 0 <= t + s < T + 1:
                    want[b * T + t] += frames[t + s] @ F._b_tap(p.B, c, tap)
    assert torch.equal(F.rowgemm_f32_acc(p.A, p.B, c), want)
    # the allocation ends exactly with frame T of the last item
    assert p.A.numel() == (M // T - 1) * c["a_item_stride"] + T * c["lda"] + K


@pytest.mark.parametrize("c", ROW_CASES + INEXACT_CASES, ids=lambda c: c["name"])
def test_bit_budget_and_poison(c):
    p = _problem(c["name"])
    assert p.budget < F.BUDGET
    for k, v in p.out64.items():
        assert bool(torch.isfinite(v).all()), f"the model read poison ({k})"
    for op in (p.A, p.B):
        live = op[~torch.isnan(op)]
        if live.numel() >= 2000:                                  # (the smallest operands hold too few values for statistics)
            assert F.zero_fraction(op) < 0.15                     # a value is zero with probability 1/8 only
            assert (live.abs().unique() > 0).sum() >= 9           # at least 9 distinct non-zero magnitudes
    if c["a_mask_mode"] and not c["framed"] and any(x < c["T"] for x in c["lens"]):
        assert bool(torch.isnan(p.A.view(c["M"], c["lda"])[:, :c["K"]]).any())  # masked frames are poison


def _rowgemm_plan(c, p):
    from rad_mmm_amd._lib import rowgemm_plan
    ptrs = {k: ADDR for k in F.rowgemm_pointer_names(c)}
    if "c2_src" in ptrs:
        ptrs["c2_src"] = _Addrs(3)
    return rowgemm_plan(**F.rowgemm_desc(c, p, ptrs))


class _Addrs(list):
    """three stand-in tensors of a c2_src list: objects with a data_ptr()"""
    class _T:
        def data_ptr(self):
            return ADDR

    def __init__(self, n):
        super().__init__(self._T() for _ in range(n))


@pytest.mark.parametrize("c", ROW_CASES + EXTRA_CASES, ids=lambda c: c["name"])
def test_every_rowgemm_case_reaches_its_kernel(c):
    p = _problem(c["name"]) if not c["real"] else F.build_rowgemm(c)
    assert _rowgemm_plan(c, p) == c["expect"]


def test_every_wgrad_case_reaches_its_kernel():
    from rad_mmm_amd._lib import wgrad_plan
    for c in WG_CASES + F.wgrad_realistic_cases():
        p = F.build_wgrad(c)
        for splits in F.WGRAD_SPLITS:
            for ldp in (c["Nc"] + 4 - c["Nc"] % 4, c["Nc"] + 5 - c["Nc"] % 2):
                kw = F.wgrad_desc(c, p, splits, ldp, c["taps"] * c["Mc"] * ldp + 64, dict(GY=ADDR, X=ADDR, P=ADDR, lens=ADDR))
                assert wgrad_plan(**kw) == c["expect"], (c["name"], splits, ldp)


def test_the_table_reaches_all_21_kernels_and_spreads_the_features():
    codes = {c["expect"] for c in ROW_CASES}
    rows16 = [c for c in ROW_CASES if c["name"].startswith("rows16")]
    got = {(F.code_fields(c["expect"])["mt"], c["b_layout"]) for c in rows16}
    assert got == {(mt, bl) for mt in (4, 6, 8, 10, 12, 13, 14, 15) for bl in (0, 1)}
    assert all(F.code_fields(c["expect"])["family"] == F.ROWS16 for c in rows16)
    assert {F.kernel_code(F.GENERIC, 0), F.kernel_code(F.GENERIC, 1), F.kernel_code(F.MIX, 0), F.kernel_code(F.MIX, 1)} <= codes
    assert {c["expect"] for c in WG_CASES} == {F.kernel_code(F.WGRAD), F.kernel_code(F.WGRAD16)}
    for c in rows16:
        f = F.code_fields(c["expect"])
        M, rows = c["M"], f["rows"]
        nmt = -(-M // rows)
        assert c["K"] in (16, 32) and rows % 4 != 0 and M - (nmt - 1) * rows < rows and c["N"] % 4 != 0 and M // c["T"] >= 3
        assert rows > 16 * (f["mt"] - 1) or f["mt"] == 4       # the tile's last row subtile is in use (4 is the smallest height)
        if f["mt"] >= 13:
            assert rows > 192                                  # the fourth staging pass stores rows
    # every feature on at least two different MT > 4, once per layout
    big = [c for c in rows16 if F.code_fields(c["expect"])["mt"] > 4]
    feats = {
        "taps1": lambda c: c["taps"] == 1, "taps3": lambda c: c["taps"] == 3, "taps5": lambda c: c["taps"] == 5,
        "dil1": lambda c: c["taps"] > 1 and c["dil"] == 1, "dil2": lambda c: c["taps"] > 1 and c["dil"] == 2, "dil8": lambda c: c["dil"] == 8,
        "sign-": lambda c: c["sign"] == -1 and c["taps"] > 1, "sign+": lambda c: c["sign"] == 1 and c["taps"] > 1,
        "mode0": lambda c: c["a_mask_mode"] == 0 and c["taps"] > 1,
        "mode1-ragged": lambda c: c["a_mask_mode"] == 1 and not c["framed"] and 0 in c["lens"] and c["T"] in c["lens"] and
        any(0 < x <= 2 * c["dil"] for x in c["lens"]),
        "bias": lambda c: c["bias"], "premask": lambda c: c["premask"], "postmask": lambda c: c["postmask"], "rowscale1": lambda c: c["rowscale"] == 1,
        "relu-dact": lambda c: c["dact"] == F.ACT_RELU, "add": lambda c: c["add"], "c2-store": lambda c: c["c2"] == "store",
        "c2-accum": lambda c: c["c2"] == "accum", "c2-src3": lambda c: c["c2"] == "src3", "odd-ldc": lambda c: c["odd_ldc"],
        "ldc%4": lambda c: not c["odd_ldc"], "framed": lambda c: c["framed"], "split": lambda c: c["split"],
    }
    for name, has in feats.items():
        on = [(F.code_fields(c["expect"])["mt"], c["b_layout"]) for c in big if has(c)]
        assert {bl for _, bl in on} == {0, 1} and len({mt for mt, _ in on}) >= 2, (name, on)
    assert any(c["split"] and F.code_fields(c["expect"])["mt"] > 8 for c in rows16)
    gen = [c for c in ROW_CASES if c["name"].startswith("generic")]
    for bl in (0, 1):
        mine = [c for c in gen if c["b_layout"] == bl]
        assert {c["K"] for c in mine} == {6, 33, 70} and {c["M"] for c in mine} == {1, 127, 129, 300} and {c["N"] for c in mine} == {1, 50, 130}
    assert any(c["framed"] for c in gen) and any(c["split"] for c in gen)
    mix = [c for c in ROW_CASES if c["expect"] // 1000000 == F.MIX]
    assert {c["M"] for c in mix} == {1, 63, 64, 65, 231} and {c["bias"] for c in mix} == {True, False}
    fast = [c for c in WG_CASES if c["expect"] == F.kernel_code(F.WGRAD16)]
    for grp in (fast, [c for c in WG_CASES if c not in fast]):
        assert {(c["Mc"], c["Nc"]) for c in grp} == {(16, 16), (130, 144), (257, 40)} and {c["taps"] for c in grp} == {1, 5}
        assert {c["x_mask_mode"] for c in grp} == {0, 1}
    assert {c["dil"] for c in WG_CASES if c["taps"] > 1} == {1, 4, 8}


# ---------------------------------------------------------------------------------------------------------------------
# planted bugs

BUG_CASES = {
    "drop_last_kquad": ["rows16-mt4-bl0", "generic-K33-M129-N50-bl0"],
    "ignore_sign": ["rows16-mt4-bl0"],
    "cross_item": ["rows16-mt4-bl1", "rows16-mt6-bl0"],
    "ignore_lens": ["rows16-mt4-bl0"],
    "m_end_short": ["rows16-mt6-bl1", "rows16-mt10-bl0"],
    "pass3_from_pass2": ["rows16-mt13-bl0"],
    "framed_last_zero": ["rows16-mt13-bl0", "rows16-mt8-bl1"],
    "swap_masks": ["rows16-mt6-bl0"],
}


def test_the_bug_lists_are_complete():
    assert set(BUG_CASES) == set(F.ROW_BUGS)


@pytest.mark.parametrize("bug", F.ROW_BUGS)
def test_planted_rowgemm_bug_changes_the_expected_words(bug):
    for name in BUG_CASES[bug]:
        c = BY_NAME[name]
        p = _problem(name, poison=False)                          # ordinary values in the masked frames: the fault must show in VALUES
        good = F.rowgemm_f32_expected(p, c)
        bad = F.rowgemm_f32_expected(p, c, bug=bug)
        assert bool(torch.isfinite(bad["C"]).all())
        changed = int((F.words(good["C"].float()) != F.words(bad["C"].float())).sum())
        assert changed > 0, f"{name} cannot see {bug}"
        assert torch.equal(good["C"], F.rowgemm_f32_expected(_problem(name), c)["C"])      # poison or not: the same expectation


@pytest.mark.parametrize("bug", F.WGRAD_BUGS)
def test_planted_wgrad_bug_changes_the_expected_words(bug):
    seen = 0
    for c in WG_CASES:
        if bug == "ignore_x_mask" and not (c["x_mask_mode"] and c["taps"] >= 1):
            continue
        p = F.build_wgrad(c, poison=False)
        good = F.wgrad_f32_model(p.GY, p.X, c, 3)
        bad = F.wgrad_f32_model(p.GY, p.X, c, 3, bug=bug)
        assert int((F.words(good.float().view(-1, c["Nc"])) != F.words(bad.float().view(-1, c["Nc"]))).sum()) > 0, (c["name"], bug)
        seen += 1
    assert seen >= 4
