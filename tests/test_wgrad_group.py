"""The grouped one-product weight gradient (radmmm_wgrad_rmh_group: up to 8 radmmm_wgrad_rmh_shift jobs behind one job table)
and the grouped weight-norm backward (radmmm_weightnorm_bwd_multi): argument checks without a GPU, every slab bit for bit
against per-job launches at the same split factor, the contraction against float64, dv / dg bit for bit against per-item
calls, and the decoder with the flow steps' res/skip weight gradients grouped against the per-layer launches."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import sub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "radmmm_hip.h")
DEV = "cuda:0"


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------ without a GPU
def test_group_entry_points_validate_without_gpu():
    """Null items, n = 0, n = 9 and a job with ld % 32 != 0 return -1 with their text before any HIP call (the addresses are
    stand-ins, never dereferenced); an accepted table is never sent to the entry points here.  The same for the grouped
    weight-norm backward, whose refusal of an item off the register path is what sends the caller to per-item calls."""
    import rad_mmm_amd._lib as L
    lib = L.lib
    d = 0x10000

    def wg(n, items, **kw):
        a = dict(shift0=0, R=64, T=32, taps=1, dil=1, splits=1)
        a.update(kw)
        return lib.radmmm_wgrad_rmh_group(items, n, a["shift0"], a["R"], a["T"], None, 0, a["taps"], a["dil"], a["splits"], 1.0, None)

    def item(**kw):
        a = dict(GYh=d, Xh=d, P=d, split_stride=64 * 64, ldg=64, g_col0=0, ldx=64, x_col0=0, Mc=64, Nc=64, ldp=64)
        a.update(kw)
        return L.WgItem(**a)

    def arr(*its):
        return (L.WgItem * len(its))(*its)

    assert wg(1, None) == -1 and lib.radmmm_last_error() == b"wgrad_rmh_group: null items"
    assert wg(0, arr(item())) == -1 and lib.radmmm_last_error().startswith(b"wgrad_rmh_group: n=0 jobs")
    assert wg(9, arr(*[item()] * 9)) == -1 and lib.radmmm_last_error().startswith(b"wgrad_rmh_group: n=9 jobs")
    for bad, text in ((item(ldg=40, Mc=40), b"wgrad_rmh_group: bad dims"), (item(ldx=72), b"wgrad_rmh_group: bad dims"),
                      (item(Xh=None), b"wgrad_rmh_group: null pointer"), (item(GYh=d + 8), b"wgrad_rmh_group: 16-byte aligned operands"),
                      (item(g_col0=4), b"wgrad_rmh_group: bad column origin"), (item(x_col0=8), b"wgrad_rmh_group: bad column origin")):
        assert wg(2, arr(item(), bad)) == -1 and lib.radmmm_last_error().startswith(text), lib.radmmm_last_error()
    assert wg(1, arr(item()), T=31, R=62) == -1 and lib.radmmm_last_error().startswith(b"wgrad_rmh_group: bad dims")
    assert wg(1, arr(item()), splits=0) == -1 and lib.radmmm_last_error().startswith(b"wgrad_rmh_group: bad dims")
    assert wg(1, arr(item(ldx=1 << 20, Nc=64)), shift0=-1, R=1024, T=1024) == -1
    assert lib.radmmm_last_error().startswith(b"wgrad_rmh_group: shift0 out of range")

    def wnb(n, items, taps=1):
        return lib.radmmm_weightnorm_bwd_multi(items, n, taps, None, None)

    def witem(**kw):
        a = dict(v=d, g=d, inv_norm=d, dW=d, dv=d, dg=d, split_stride=64 * 64, splits=1, Cout=64, Cin=64, ldw=64, perm_split=0,
                 off_lo=0, off_hi=0)
        a.update(kw)
        return L.WnbItem(**a)

    def warr(*its):
        return (L.WnbItem * len(its))(*its)

    assert wnb(1, None) == -1 and lib.radmmm_last_error() == b"weightnorm_bwd_multi: null items"
    assert wnb(0, warr(witem())) == -1 and lib.radmmm_last_error().startswith(b"weightnorm_bwd_multi: n=0 items")
    assert wnb(9, warr(*[witem()] * 9)) == -1 and lib.radmmm_last_error().startswith(b"weightnorm_bwd_multi: n=9 items")
    assert wnb(1, warr(witem()), taps=3) == -1 and lib.radmmm_last_error().startswith(b"weightnorm_bwd_multi: taps=3")
    assert wnb(2, warr(witem(), witem(dv=None))) == -1 and lib.radmmm_last_error().startswith(b"weightnorm_bwd_multi: null pointer (item 1)")
    for bad in (witem(Cin=34, ldw=36), witem(Cin=2052, ldw=2052), witem(ldw=66), witem(split_stride=4098), witem(dW=d + 4),
                witem(perm_split=2), witem(off_hi=6)):
        assert wnb(2, warr(witem(), bad)) == -1 and b"item 1 is not on the register path" in lib.radmmm_last_error()


def test_group_structs_match_the_c_layout(tmp_path):
    """sizeof / offsetof of radmmm_wg_item and radmmm_wnb_item as gcc lays them out == the ctypes mirrors; the header says what
    the binding's argument lists say."""
    import rad_mmm_amd._lib as L
    pairs = [("radmmm_wg_item", L.WgItem), ("radmmm_wnb_item", L.WnbItem)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HDR}"', "int main(void) {"]
    for cname, mirror in pairs:
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in mirror._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    r = subprocess.run(["gcc", "-std=c99", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    for cname, mirror in pairs:
        assert int(got[cname]) == ctypes.sizeof(mirror), cname
        for fname, _ in mirror._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(mirror, fname).offset, f"{cname}.{fname}"
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    assert re.search(r"int radmmm_wgrad_rmh_group\(const radmmm_wg_item\* items, int n, int shift0, int R, int T,", hdr)
    assert re.search(r"int radmmm_weightnorm_bwd_multi\(const radmmm_wnb_item\* items, int n, int taps,", hdr)


# ------------------------------------------------------------------------------------------ the grouped launch
def _planes(seed, R, ld, tail_of=None):
    """fp16 hi planes [R, ld] of gy = randn * 0.3 * 32 and x = softplus(randn), every column filled.  tail_of: the planes are the
    LAST R rows of an allocation of tail_of rows (the extents given to the kernel cover exactly the planes)."""
    g = torch.Generator().manual_seed(seed)
    rows = tail_of or R
    gy = (torch.randn(rows, ld, generator=g) * 9.6).half().to(DEV)
    x = torch.nn.functional.softplus(torch.randn(rows, ld, generator=g)).half().to(DEV)
    return gy[rows - R:], x[rows - R:]


def _run_group(jobs, B, T, taps, dil, splits, lens, shift0=0):
    """jobs: (gh, xh, Mc, Nc, g_col0, x_col0) -> (slabs of the grouped launch, slabs of one radmmm_wgrad_rmh_shift launch per job),
    every slab tensor [S, taps, Mc, Nc] pre-filled with NaN."""
    import rad_mmm_amd._lib as L
    from rad_mmm_amd._lib import lib, check, ptr, stream
    R = B * T
    nan = lambda Mc, Nc: torch.full((splits, taps, Mc, Nc), float("nan"), device=DEV)      # noqa: E731
    Pg = [nan(j[2], j[3]) for j in jobs]
    Ps = [nan(j[2], j[3]) for j in jobs]
    items = (L.WgItem * len(jobs))(*[L.WgItem(ptr(gh), ptr(xh), ptr(P), P.stride(0), gh.stride(0), g0, xh.stride(0), x0, Mc, Nc, Nc)
                                     for (gh, xh, Mc, Nc, g0, x0), P in zip(jobs, Pg)])
    check(lib.radmmm_wgrad_rmh_group(items, len(jobs), shift0, R, T, ptr(lens), 1 if lens is not None else 0, taps, dil, splits,
                                     1.0 / 32, stream()), "wgrad_rmh_group")
    for (gh, xh, Mc, Nc, g0, x0), P in zip(jobs, Ps):
        check(lib.radmmm_wgrad_rmh_shift(ptr(gh), gh.stride(0), g0, ptr(xh), xh.stride(0), x0, shift0, R, T, ptr(lens),
                                         1 if lens is not None else 0, ptr(P), Nc, P.stride(0), Mc, Nc, taps, dil, splits, 1.0 / 32,
                                         stream()), "wgrad_rmh_shift")
    torch.cuda.synchronize()
    return Pg, Ps


MIXED = [(64, 96), (288, 32), (256, 320)]       # 1, 2 and 2 tiles: different tile counts, partial tiles in M and in N


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,shapes,taps,dil,splits,masked,origins,shift0,tail", [
    (3, 40, [(64, 96)], 1, 1, 1, False, False, 0, False),                 # n = 1: ONE workgroup; K-step tail, two utterance boundaries
    (4, 64, [(256, 256)] * 4, 1, 1, 2, False, False, 0, False),           # four equal jobs, 8 workgroups
    (3, 40, MIXED, 1, 1, 3, False, False, 0, False),                      # 15 workgroups; 4 K steps in 3 splits: the last one is empty
    (4, 64, MIXED, 1, 1, 5, False, False, 0, False),                      # 25 workgroups; 8 K steps in 5 splits: 2, 2, 2, 2, 0
    (3, 40, MIXED, 1, 1, 5, False, False, 0, False),                      # more splits than K steps
    (3, 40, MIXED, 5, 2, 2, True, False, 0, False),                       # five taps, dilation 2, lens / x_mask: 50 workgroups
    (4, 64, MIXED, 1, 1, 3, True, True, -1, False),                       # column origins, a frame-shift origin, the length mask
    (3, 40, MIXED, 1, 1, 2, False, True, 0, True),                        # planes at the very end of their allocations
])
def test_group_slabs_are_the_single_launches_bit_for_bit(B, T, shapes, taps, dil, splits, masked, origins, shift0, tail):
    """Every slab of the grouped launch == the slab of a radmmm_wgrad_rmh_shift launch of that job alone with the same split
    factor, bit for bit, and no element of a slab is left unwritten (NaN pre-fill): an empty split writes zeros."""
    R = B * T
    jobs = []
    for k, (Mc, Nc) in enumerate(shapes):
        g0, x0 = ((8 * (k + 1), 24 + 8 * k) if origins else (0, 0))
        ldg, ldx = -(-(Mc + g0) // 32) * 32, -(-(Nc + x0) // 32) * 32
        gh, _ = _planes(100 * k + R, R, ldg, tail_of=R + 3 + k if tail else None)
        _, xh = _planes(100 * k + R + 1, R, ldx, tail_of=R + 5 if tail else None)
        jobs.append((gh, xh, Mc, Nc, g0, x0))
    lens = torch.tensor([max(1, T - 7 * b) for b in range(B)], dtype=torch.int32, device=DEV) if masked else None
    Pg, Ps = _run_group(jobs, B, T, taps, dil, splits, lens, shift0)
    for k, (a, b) in enumerate(zip(Pg, Ps)):
        assert not torch.isnan(b).any() and not torch.isnan(a).any(), k
        assert torch.equal(_bits(a), _bits(b)), (k, float((a - b).abs().max()))
        assert a.abs().max() > 0
    steps = -(-R // 32)
    per = -(-steps // splits)
    if per * (splits - 1) >= steps:
        assert all(float(P[-1].abs().max()) == 0.0 for P in Pg)          # the empty split's slab


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,splits", [(3, 40, 2), (2, 352, 4)])
def test_group_against_float64(B, T, splits):
    """Each job of a grouped launch (the three shapes above, through ops.wgrad_rmh_group_slabs) against the float64 contraction
    of its fp16 hi planes at R = 120 and 704 frames.  Products of fp16 values are exact in fp32, so what is left is the fp32
    accumulation: an element is a sum of R exact products in some order plus the sum of S slabs and the final scale, at most
    R + S + 1 roundings of at most 2^-24 of the running magnitude each, which |gy|^T |x| bounds: |P - ref| <=
    1.01 (R + S + 1) 2^-24 |gy|^T |x| elementwise (1.01: the second-order terms)."""
    from rad_mmm_amd import ops
    R = B * T
    jobs = []
    for k, (Mc, Nc) in enumerate(MIXED):
        gh, _ = _planes(7 * k + R, R, -(-Mc // 32) * 32)
        _, xh = _planes(7 * k + R + 1, R, -(-Nc // 32) * 32)
        jobs.append((gh, xh, Mc, Nc))
    Ps = ops.wgrad_rmh_group_slabs(jobs, B, T, 1, 1, 1.0 / 32, splits=splits)
    for (gh, xh, Mc, Nc), P in zip(jobs, Ps):
        assert P.shape == (splits, 1, Mc, Nc)
        gv, xv = gh.double()[:, :Mc] / 32, xh.double()[:, :Nc]
        ref = gv.t() @ xv
        bound = 1.01 * (R + splits + 1) * 2.0 ** -24 * (gv.abs().t() @ xv.abs())
        got = P.sum(0)[0].double()
        used = float(((got - ref).abs() / bound).max())
        print(f"grouped wgrad R={R} S={splits} {Mc}x{Nc}: largest |P - ref| / bound {used:.4f}")
        assert used <= 1.0


# ------------------------------------------------------------------------------------------ weight-norm backward
@pytest.mark.gpu
@pytest.mark.parametrize("poison_nan", [False, True])
def test_weightnorm_bwd_multi_is_the_single_calls_bit_for_bit(poison_nan):
    """Four items -- Cout in {5, 64}, Cin in {32, 1024}, 1 and 4 slabs, one with a column permutation -- through
    radmmm_weightnorm_bwd_multi and through one radmmm_weightnorm_bwd each: dv and dg bit-equal, with poison 0 and NaN."""
    import rad_mmm_amd._lib as L
    from rad_mmm_amd._lib import lib, check, ptr, stream
    g = torch.Generator().manual_seed(5)
    specs = [(5, 32, 1, (0, 0, 0), 32), (64, 1024, 4, (0, 0, 0), 1024), (64, 32, 4, (16, 24, 0), 40), (5, 1024, 1, (16, 1016, 0), 1032)]
    poison = torch.tensor([float("nan") if poison_nan else 0.0], device=DEV)
    items, singles, outs = [], [], []
    for Cout, Cin, S, perm, ldw in specs:
        v = torch.randn(Cout, Cin, 1, generator=g).to(DEV)
        gg = torch.randn(Cout, 1, 1, generator=g).to(DEV)
        inv = (1.0 / v.flatten(1).norm(dim=1)).contiguous()
        dW = torch.randn(S, 1, Cout, ldw, generator=g).to(DEV)
        dv_m, dg_m = torch.full_like(v, float("nan")), torch.full_like(gg, 7.0)
        dv_s, dg_s = torch.full_like(v, float("nan")), torch.full_like(gg, 7.0)
        items.append(L.WnbItem(ptr(v), ptr(gg), ptr(inv), ptr(dW), ptr(dv_m), ptr(dg_m), dW.stride(0), S, Cout, Cin, ldw, *perm))
        singles.append((v, gg, inv, dW, dv_s, dg_s, S, Cout, Cin, ldw, perm))
        outs.append((dv_m, dg_m, dv_s, dg_s))
    check(lib.radmmm_weightnorm_bwd_multi((L.WnbItem * len(items))(*items), len(items), 1, ptr(poison), stream()), "weightnorm_bwd_multi")
    for v, gg, inv, dW, dv_s, dg_s, S, Cout, Cin, ldw, perm in singles:
        check(lib.radmmm_weightnorm_bwd(ptr(v), ptr(gg), ptr(inv), ptr(dW), S, dW.stride(0), ptr(dv_s), ptr(dg_s), Cout, Cin, 1, ldw,
                                        perm[0], perm[1], perm[2], ptr(poison), stream()), "weightnorm_bwd")
    torch.cuda.synchronize()
    for k, (dv_m, dg_m, dv_s, dg_s) in enumerate(outs):
        assert torch.equal(_bits(dv_m), _bits(dv_s)) and torch.equal(_bits(dg_m), _bits(dg_s)), k
        assert not torch.isnan(dv_m).any() and bool(torch.isnan(dg_m).all()) == poison_nan
    # the permuted item against the formula: dg = sum_ci dW[col(ci)] v / |v|
    v, gg, inv, dW, _, _, S, Cout, Cin, ldw, perm = singles[2]
    cols = torch.tensor([ci + perm[1] if ci < perm[0] else ci - perm[0] + perm[2] for ci in range(Cin)], device=DEV)
    if not poison_nan:
        want = (dW.double().sum(0)[0][:, cols] * v[:, :, 0].double()).sum(1) * inv.double()
        assert torch.allclose(outs[2][1].flatten().double(), want, rtol=1e-5, atol=1e-6)


@pytest.mark.gpu
def test_weightnorm_bwd_multi_leaves_other_items_to_single_calls():
    """ops.weightnorm_bwd_multi with an item off the register path (Cin = 34) or with three taps: the grouped entry point
    refuses, every item goes through radmmm_weightnorm_bwd, and the results are those of ops.weightnorm_bwd."""
    from rad_mmm_amd import ops
    g = torch.Generator().manual_seed(9)
    for shapes in ([(8, 32, 1), (8, 34, 1)], [(8, 32, 3), (8, 32, 3)]):
        vs = [torch.randn(*s, generator=g).to(DEV) for s in shapes]
        gs = [torch.randn(s[0], 1, 1, generator=g).to(DEV) for s in shapes]
        invs = [(1.0 / v.flatten(1).norm(dim=1)).contiguous() for v in vs]
        slabs = [torch.randn(2, s[2], s[0], 36, generator=g).to(DEV) for s in shapes]
        got = ops.weightnorm_bwd_multi(vs, gs, invs, slabs, 36)
        for (dv, dg), v, gg, inv, P in zip(got, vs, gs, invs, slabs):
            dv1, dg1 = ops.weightnorm_bwd(v, gg, inv, P, 36)
            assert torch.equal(dv, dv1) and torch.equal(dg, dg1)


# ------------------------------------------------------------------------------------------ the decoder
def _decoder_step(golden, group, monkeypatch, calls):
    from oracle import radmmm_oracle as O
    from rad_mmm_amd import ops
    from rad_mmm_amd.common import SequenceLength
    from rad_mmm_amd.decoders import RADMMMFlow
    from rad_mmm_amd.loss import RADMMMLoss
    monkeypatch.setenv("RADMMM_CONVNORM_H3_MIN_ROWS", "0")
    monkeypatch.setenv("RADMMM_F8X_MIN_ROWS", "0")      # keep the FP8-cross scheme on this small batch
    monkeypatch.setenv("RADMMM_PRECISION", "f8x")
    monkeypatch.setenv("RADMMM_WGRAD_PRODUCTS", "1")
    monkeypatch.setenv("RADMMM_DEBUG", "1")
    monkeypatch.setenv("RADMMM_WGRAD_GROUP", group)
    inner = ops.wgrad_rmh_group_slabs

    def counted(jobs, *a, **kw):
        Ps = inner(jobs, *a, **kw)
        calls.append((len(jobs), Ps[0].shape[0]))
        return Ps
    monkeypatch.setattr(ops, "wgrad_rmh_group_slabs", counted)
    g = golden("decoder_cfg2_small.npz")
    kw = {k: (v.item() if v.shape == () else v) for k, v in sub(g, "cfg.").items()}
    cfg = O.DecoderConfig(**kw)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in O.procedural_decoder_state(O.decoder_state_shapes(cfg)).items()}
    dec = RADMMMFlow(use_accent=True, **kw)
    dec.load_state_dict(sd)
    dec.gemm_precision = "f8x"
    dec = dec.to(DEV).train()
    b = {k: torch.from_numpy(np.asarray(v)) for k, v in O.synthetic_batch(int(g["B"]), int(g["T"]), cfg, 1234, bool(g["ragged"])).items()}
    gb = {k: v.to(DEV) for k, v in b.items()}
    mel = gb["mel"].clone().requires_grad_(True)
    ctx = gb["context"].clone().requires_grad_(True)
    sl = SequenceLength(gb["lengths"])
    out = dec(mel, gb["spk"], ctx, sl, gb["f0"], gb["energy"], gb["accent"])
    loss = RADMMMLoss(sigma=1.0, n_group_size=cfg.n_group_size)(out, None, sl, 0)["loss_mel"][0]
    loss.backward()
    res = {"z_mel": out["z_mel"].detach(), "loss": loss.detach(), "grad.mel": mel.grad, "grad.context": ctx.grad}
    for i, ls in enumerate(out["log_s_list"]):
        res[f"log_s.{i}"] = ls.detach()
    monkeypatch.setattr(ops, "wgrad_rmh_group_slabs", inner)
    return res, {n: p.grad for n, p in dec.named_parameters()}


RES_SKIP_WEIGHT = re.compile(r"\.affine_param_predictor\.res_skip_layers\.\d+\.weight_[vg]$")


@pytest.mark.gpu
def test_decoder_grouped_against_per_layer_launches(golden, monkeypatch):
    """decoder_cfg2_small under f8x, forward + NLL + backward with the res/skip weight gradients grouped and, with
    RADMMM_WGRAD_GROUP=0, launched per layer: outputs, loss and every gradient that is not a res/skip weight_v / weight_g are
    bit-equal.  The res/skip gradients are bit-equal where the grouped split factor is the per-conv one -- at this size it
    is, the 192 rows cap both at 1 -- and otherwise within the 5e-4 bars of the parity tests."""
    from rad_mmm_amd import ops
    on_calls, off_calls = [], []
    r_on, g_on = _decoder_step(golden, "1", monkeypatch, on_calls)
    r_off, g_off = _decoder_step(golden, "0", monkeypatch, off_calls)
    assert on_calls and not off_calls                        # the grouped launch ran, and the switch turns it off
    assert r_on.keys() == r_off.keys() and g_on.keys() == g_off.keys()
    for k in r_on:
        assert torch.equal(r_on[k], r_off[k]), k
    rows = int(golden("decoder_cfg2_small.npz")["B"]) * int(golden("decoder_cfg2_small.npz")["T"])
    same_s = all(S == ops.pick_splits(n_jobs, rows, 256) == ops.pick_splits(1, rows, 256) for n_jobs, S in on_calls)
    n_res, worst = 0, 0.0
    for n in g_on:
        if RES_SKIP_WEIGHT.search(n):
            n_res += 1
            a, b = g_on[n].double(), g_off[n].double()
            l2 = float((a - b).norm() / b.norm())
            mx = float((a - b).abs().max() / b.abs().max())
            worst = max(worst, l2, mx)
            if same_s:
                assert torch.equal(g_on[n], g_off[n]), n
            assert l2 < 5e-4 and mx < 5e-4, (n, l2, mx)
        else:
            assert torch.equal(g_on[n], g_off[n]), n
    print(f"grouped vs per-layer: {n_res} res/skip gradients, jobs / splits per grouped launch {sorted(set(on_calls))}, worst rel {worst:.2e}")
    assert n_res > 0 and same_s
