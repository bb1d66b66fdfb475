"""The host model of the split-operand GEMMs (tests/_gemm_ref.py) held to account on the CPU: against
torch.nn.functional.conv1d in float64 (equality: the values are exact), the bit budget of every operand set the GPU tests
use (an fp32 accumulation in random term orders equals the float64 result bit for bit), and the model's sensitivity to
every one of the six operand arrays.  No GPU; the built library is asked one host-only question: which kernel every case of
the GPU tests' table reaches (radmmm_rowgemm_h3_plan)."""
import numpy as np
import pytest
import torch

import _gemm_ref as G

ROW_CASES = G.rowgemm_cases()
WG_CASES = G.wgrad_cases()


def test_the_projects_exponents_are_the_ones_the_cases_use():
    import re
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rad_mmm_amd", "ops.py")).read()
    m = re.search(r"^X8_ACT_EXP, X8_GRAD_EXP, X8_W_EXP = (-?\d+), (-?\d+), (-?\d+)", src, flags=re.M)
    assert tuple(map(int, m.groups())) == (G.X8_ACT_EXP, G.X8_GRAD_EXP, G.X8_W_EXP)
    # at least one case per kernel family with them, and one with a negative exponent
    for fam in ("h3d", "win", "one"):
        mine = [c for c in ROW_CASES if c["name"].startswith(fam) and c["nprod"] == 2]
        assert any((c["a8_exp"], c["b8_exp"]) in ((G.X8_ACT_EXP, G.X8_W_EXP), (G.X8_GRAD_EXP, G.X8_W_EXP)) for c in mine), fam
        assert any(c["a8_exp"] < 0 or c["b8_exp"] < 0 for c in mine), fam
    rm8 = [c for c in WG_CASES if c["kind"] == "rm8"]
    assert any((c["g8_exp"], c["x8_exp"]) == (G.X8_GRAD_EXP, G.X8_ACT_EXP) for c in rm8) and any(c["g8_exp"] < 0 and c["x8_exp"] < 0 for c in rm8)


def test_the_matrix_covers_what_it_claims():
    fam = lambda c: c["expect"] // 1000
    codes = {c["expect"] for c in ROW_CASES}
    for nprod in (1, 2, 3):
        for mb in (4, 5, 6, 7, 8):
            for ek in range(5):
                assert G.kernel_code(G.H3_H3D, nprod, mb, ek) in codes
    for mb in (4, 5, 6, 7, 8):
        for ek in (G.EK_PLAIN, G.EK_SPLIT, G.EK_RES, G.EK_DGRAD):
            assert G.kernel_code(G.H3_ONE, 2, mb, ek) in codes
    for mb in (7, 8):
        for ek in (G.EK_PLAIN, G.EK_SPLIT, G.EK_DGRAD):
            assert G.kernel_code(G.H3_WIN, 2, mb, ek) in codes
        assert G.kernel_code(G.H3_WIN, 3, mb, G.EK_PLAIN) in codes and G.kernel_code(G.H3_ONE, 3, mb, G.EK_PLAIN) in codes
    assert {G.kernel_code(G.H3_NARROW, 3, 4, 0), G.kernel_code(G.H3_NARROW, 1, 4, 0)} <= codes
    win = [c for c in ROW_CASES if fam(c) == G.H3_WIN]
    assert {c["dil"] for c in win} == {1, 2, 8} and {c["T"] - 32 * ((c["expect"] // 10) % 10) for c in win} == {0, 1}
    assert any(c["extra_tap"] for c in win) and any(c["extra_tap"] and c["nprod"] == 3 for c in ROW_CASES)
    for c in ROW_CASES:                       # ragged: a length of 1 and one below taps/2 * dil wherever there are taps
        rows = 32 * ((c["expect"] // 10) % 10)                     # (T = 32 mb exactly makes M a multiple: the window kernel's edge)
        assert 1 in c["lens"] and (c["M"] % rows != 0 or c["T"] == rows) and c["N"] % 2 == 0 and c["K"] in (64, 128)
        if (c["taps"] // 2) * c["dil"] > 2:
            assert any(1 < l < (c["taps"] // 2) * c["dil"] for l in c["lens"])
    assert {(c["taps"], c["dil"] % 2) for c in WG_CASES} >= {(1, 1), (3, 1), (3, 0), (5, 1), (5, 0)}


@pytest.mark.parametrize("c", ROW_CASES, ids=[c["name"] for c in ROW_CASES])
def test_every_rowgemm_case_reaches_its_kernel(c, monkeypatch):
    """the plan (host only: stand-in addresses, the MI355X's CU count without a device) names the case's kernel under the
    switches the case sets -- what tests/test_hip_gemm_direct.py then holds the launch to"""
    from rad_mmm_amd._lib import rowgemm_h3_plan
    for k in G.ROWGEMM_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    assert rowgemm_h3_plan(**G.rowgemm_kw(c, G.rowgemm_layout(c), G.standin_addresses(c))) == c["expect"]


# ---------------------------------------------------------------------------------------------------------------------
# against conv1d

def _conv_ref(A, B, c):
    """the same accumulator through F.conv1d in float64, item by item, masking done by zeroing the input"""
    M, N, K, T, taps, dil = c["M"], c["N"], c["K"], c["T"], c["taps"], c["dil"]
    out = torch.zeros(M, N, dtype=torch.float64)
    for an, bn, f in G.product_pairs(c["nprod"], c["a8_exp"], c["b8_exp"]):
        a = getattr(A, an)
        w = getattr(B, bn).view(taps, -1, getattr(B, bn).shape[-1])[:, :N, :K]          # [taps][N][K]
        w = w.permute(1, 2, 0)                                                          # conv1d weight [N][K][taps]
        if c["sign"] < 0:
            w = w.flip(-1)                                                              # the data gradient walks the taps backwards
        for b in range(M // T):
            lim = c["lens"][b] if c["a_mask_mode"] else T
            x = a[b * T:(b + 1) * T, :K].clone()
            x[lim:] = 0
            y = torch.nn.functional.conv1d(x.T[None], w.contiguous(), padding=(taps // 2) * dil, dilation=dil)[0].T
            out[b * T:(b + 1) * T] += f * y
    return out


@pytest.mark.parametrize("nprod,taps,dil,sign,mask", [(3, 5, 2, 1, 0), (3, 5, 2, -1, 1), (2, 3, 8, 1, 1), (2, 5, 1, -1, 0), (1, 3, 1, -1, 1),
                                                      (2, 5, 8, 1, 1), (3, 1, 1, 1, 1)])
def test_model_equals_conv1d(nprod, taps, dil, sign, mask):
    # ragged lengths, an item shorter than taps/2 * dil (1 and 3 frames), an item boundary every 29 rows
    c = G._case(name=f"conv-{nprod}-{taps}-{dil}-{sign}-{mask}", nprod=nprod, taps=taps, dil=dil, sign=sign, a_mask_mode=mask, T=29,
                lens=[29, 1, 3, 17], N=10, K=32, a8_exp=-3, b8_exp=1)
    p = G.build_rowgemm(c)
    assert torch.equal(p.acc, _conv_ref(p.A, p.B, c))


# ---------------------------------------------------------------------------------------------------------------------
# the bit budget

def _orders_equal(terms64, expect64, seed):
    """fp32 accumulation of the terms, strictly one after the other (numpy's accumulate), in three random orders"""
    t32 = terms64.numpy().astype(np.float32)
    assert np.array_equal(t32.astype(np.float64), terms64.numpy())
    rng = np.random.default_rng(seed)
    res = []
    for _ in range(3):
        s = np.add.accumulate(t32[rng.permutation(t32.size)], dtype=np.float32)
        res.append(float(s[-1]) if s.size else 0.0)
    return [r == float(expect64) for r in res]


def _probe_elements(mag, n, seed):
    """element of the largest budget + n random ones"""
    g = torch.Generator().manual_seed(seed)
    flat = [int(mag.argmax())] + torch.randint(0, mag.numel(), (n,), generator=g).tolist()
    return [np.unravel_index(i, tuple(mag.shape)) for i in flat]


@pytest.mark.parametrize("c", ROW_CASES, ids=[c["name"] for c in ROW_CASES])
def test_rowgemm_operand_sets_are_exactly_summable(c):
    p = G.build_rowgemm(c)
    assert p.budget < G.BUDGET and p.grid_ok
    assert G.zero_fraction(p.A) < 0.25 and G.zero_fraction(p.B) < 0.25
    mag = G.rowgemm_acc(p.A, p.B, c, absolute=True)
    for r, n in _probe_elements(mag, 6, 5):
        terms = G.rowgemm_terms(p.A, p.B, c, int(r), int(n))
        assert float(terms.sum()) == float(p.acc[r, n])                  # the element-wise path agrees with the matrix path
        assert all(_orders_equal(terms, p.acc[r, n], 7)), (c["name"], r, n)


@pytest.mark.parametrize("c", WG_CASES, ids=[c["name"] for c in WG_CASES])
def test_wgrad_operand_sets_are_exactly_summable(c):
    c = dict(c)
    p = G.build_wgrad(c)
    assert p.budget < G.BUDGET
    for tap, m, n in _probe_elements(p.acc.abs() + 1, 6, 5):
        if c["kind"] in ("rm", "rm8", "rmh"):
            terms = G.wgrad_rows_terms(p.GY, p.X, c, int(tap), int(m), int(n))
        else:
            terms = G.wgrad_h3_terms(p.GYt, p.Xt, c, int(tap), int(m), int(n))
        assert float(terms.sum()) == float(p.acc[tap, m, n])
        assert all(_orders_equal(terms, p.acc[tap, m, n], 11))


def test_past_the_budget_the_orders_disagree():
    """the check above has teeth: with the value sets widened (hi up to +-64, the residuals at 2^-13) the budget is above
    2^24 and fp32 accumulations in random orders no longer all equal the float64 sum"""
    c = G._case(name="wide", nprod=3, taps=5, dil=1, T=40, lens=[40, 7], N=6, K=128, lo_log2=-13)
    g = torch.Generator().manual_seed(3)
    A = G.gen_split(c["M"] + 4, c["K"], g, -13, hi_set=tuple(range(-64, 65)), zero_every=64)
    B = G.gen_split(5 * 8, c["K"], g, -13, hi_set=tuple(range(-64, 65)), zero_every=64)
    mag = G.rowgemm_acc(A, B, c, absolute=True)
    assert float(mag.max()) * 2.0 ** 13 >= G.BUDGET
    acc = G.rowgemm_acc(A, B, c)
    bad = 0
    for r in range(8, 24):
        for n in range(6):
            bad += not all(_orders_equal(G.rowgemm_terms(A, B, c, r, n), acc[r, n], r * 6 + n))
    assert bad > 0


# ---------------------------------------------------------------------------------------------------------------------
# sensitivity: one element of any of the six arrays changes the output; a hidden row does not

def _flip(op, name, r, k):
    """add one unit to element (r, k) of a decoded array (hi / hi8: the next integer; lo / lo8: the next residual)"""
    a = getattr(op, name)
    a = a.clone()
    unit = {"d_hi": 1.0, "d_lo": 2.0 ** op.lo_log2}.get(name)
    if unit is None:
        unit = 2.0 ** op.x8_exp if name == "d_hi8" else 2.0 ** (op.lo_log2 + 11 + op.x8_exp)
    a[r, k] += unit
    setattr(op, name, a)


@pytest.mark.parametrize("nprod,arrays", [(3, ("d_hi", "d_lo")), (2, ("d_hi", "d_hi8", "d_lo8")), (1, ("d_hi",))])
def test_model_sees_every_array_and_hides_what_the_mask_hides(nprod, arrays):
    import copy
    c = G._case(name=f"sens-{nprod}", nprod=nprod, taps=3, dil=2, sign=1, a_mask_mode=1, T=20, lens=[20, 9, 1], N=8, K=64,
                a8_exp=G.X8_ACT_EXP, b8_exp=G.X8_W_EXP, extra_tap=0)
    cx = G._case(name=f"sensx-{nprod}", nprod=nprod, taps=3, dil=2, sign=-1, a_mask_mode=0, T=20, lens=[20, 9, 1], N=8, K=64,
                 a8_exp=G.X8_GRAD_EXP, b8_exp=G.X8_W_EXP, extra_tap=1)
    for case in (c, cx):
        p = G.build_rowgemm(case)
        base = G.rowgemm_acc(p.A, p.B, case)
        K, T, M = case["K"], case["T"], case["M"]
        a_spots = [(5, 17), (5, K - 1), (T + 8, 3)]                # interior, the last k of a row, the last valid frame of item 1 (length 9)
        if case["extra_tap"]:
            a_spots.append((case["extra_a_rows"] + 7, K - 1))      # the extra segment
        for name in arrays:
            for r, k in a_spots:
                A2 = copy.copy(p.A)
                _flip(A2, name, r, k)
                assert not torch.equal(G.rowgemm_acc(A2, p.B, case), base), (name, r, k)
            hidden = [(5, K), (5, K + 31)]                         # columns past K
            if case["a_mask_mode"]:
                hidden += [(T + 9, 3), (T + 19, 0), (2 * T + 1, 5)]  # frames at and past lens[b]
            if case["extra_tap"]:
                hidden += [(M + 1, 0), (M + 4, K - 1)]             # the gap between the two matrices
            for r, k in hidden:
                A2 = copy.copy(p.A)
                _flip(A2, name, r, k)
                assert torch.equal(G.rowgemm_acc(A2, p.B, case), base), (name, r, k)
            nt = case["taps"] + case["extra_tap"]
            for tap in range(nt):                                  # every tap's weights, the extra segment's included
                for n, k in ((0, 0), (case["N"] - 1, K - 1)):
                    B2 = copy.copy(p.B)
                    _flip(B2, name, tap * p.Nalloc + n, k)
                    assert not torch.equal(G.rowgemm_acc(p.A, B2, case), base), (name, tap, n, k)
                for n, k in ((case["N"], 0), (p.Nalloc - 1, K - 1), (0, K)):   # rows >= N, columns >= K
                    B2 = copy.copy(p.B)
                    _flip(B2, name, tap * p.Nalloc + n, k)
                    assert torch.equal(G.rowgemm_acc(p.A, B2, case), base), (name, tap, n, k)
    # without the mask the same frames DO count: the neighbour of a masked row is a live row under a_mask_mode 0
    c0 = dict(c, a_mask_mode=0)
    p = G.build_rowgemm(c)
    A2 = copy.copy(p.A)
    _flip(A2, arrays[0], c["T"] + 9, 3)
    assert not torch.equal(G.rowgemm_acc(A2, p.B, c0), G.rowgemm_acc(p.A, p.B, c0))


def test_wgrad_model_masks_and_boundaries():
    """the weight-gradient model: a partner frame in the neighbouring utterance or at / past the length does not count"""
    import copy
    c = dict(name="wsens", kind="rm8", taps=3, dil=2, T=32, lens=[32, 1, 20], R=96, x_mask=1, Mc=8, Nc=8, g8_exp=-2, x8_exp=-3,
             lo_log2=-12, acc_scale=1.0)
    p = G.build_wgrad(c)
    base = G.wgrad_rows_model(p.GY, p.X, c)
    for name in ("d_hi", "d_hi8", "d_lo8"):
        for op_name in ("GY", "X"):
            # (row, column, counts as a GY row, counts as an X row).  Shifts -2 / 0 / 2.  A GY row is not masked itself: it
            # counts when one of its partner frames is live.  Row 33 = item 1 (length 1), frame 1: partners -1 / 1 / 3, none
            # live.  Row 84 = item 2 (length 20), frame 20: partner 18 is live, the X row itself is masked.
            for r, k, live_g, live_x in ((5, 3, True, True), (31, 7, True, True), (32, 0, True, True), (64 + 19, 2, True, True),
                                         (33, 0, False, False), (64 + 20, 2, True, False), (5, 8, False, False)):
                q = copy.copy(p)
                op = copy.copy(getattr(p, op_name))
                _flip(op, name, r, k)
                setattr(q, op_name, op)
                changed = not torch.equal(G.wgrad_rows_model(q.GY, q.X, c), base)
                assert changed == (live_g if op_name == "GY" else live_x), (name, op_name, r, k)
