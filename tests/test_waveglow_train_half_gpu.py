"""GPU checks of WaveGlow training on the f16 matrix cores (rad_mmm_amd/waveglow.py train_precision "h3"): the two
gradient producers that write a scaled split pair in the pass that computes the value (radmmm_wg_coupling_bwd_split,
radmmm_wg_gate_bwd_split) bit for bit against their fp32 twins and radmmm_split_f16; radmmm_rowgemm_h3 and radmmm_wgrad_rm
at the backward pass's shapes against float64 of the operands as stored, with the bar derived from the formats; the step
end to end against the reference's float64 gradients and the float64 restatement at 4x the fp32 tests' bars (a
three-product operand carries 2^-22 relative, an fp32 MFMA operand 2^-24); and the properties the fp32 step has
(repeatable bits, device lengths, NaN past the lengths, chunking, no device -> host synchronisation, three Adam steps).

Measured on an MI355X (the tests print each figure): rowgemm_h3 worst error / bound 0.024, wgrad_rm 0.001; worst measured /
bar 0.086 on the reference fixture (loss 2.7e-9 from float64), 0.048 on the ragged batch, 0.049 at the shipped WN size (at
most 2.0e-6, upsample.weight) -- all inside the fp32 bars themselves; chunks of 2 items 2.0e-7; three Adam steps 9.3e-8
from the restatement's losses; grad_scale auto / 2^12: finite, not saturated, 2.7e-3 relative L2 from the automatic step;
auto x 2^10: grad_saturated() False, 6.6e-7."""
import re

import pytest
import torch

from _waveglow_bwd_ref import grads_ref, leaves_of, loss_ref, rel_l2
from _waveglow_ref import HOP, SHIPPED_WN, load_fixture, random_state

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
RAGGED = [9, 1, 5, 3, 2]
LENS, TG = [37, 32, 1, 300], 300
R = len(LENS) * TG
C = 32
SCALES = [1.0, 2.0 ** 17]


def _lib():
    from rad_mmm_amd._lib import check, lib, ptr, stream
    return check, lib, ptr, stream()


def _mask(lens=LENS, T=TG):
    return (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).reshape(-1)


def _lens(lens=LENS):
    return torch.tensor(lens, dtype=torch.int32, device=DEV)


def _poisoned(g, *shape, mag=1.0):
    x = mag * torch.randn(*shape, generator=g)
    x[~_mask()] = float("nan")                  # rows past a length: never read
    return x


def _split(x, cols, scale, ldh):
    from rad_mmm_amd import ops
    return ops.split_f16(x.contiguous(), cols, scale, ldh, 3)


def _pair(rows, ld):
    return (torch.full((rows, ld), 7.0, device=DEV, dtype=torch.float16),
            torch.full((rows, ld), 7.0, device=DEV, dtype=torch.float16))


def _flag():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


# ---- 1. the two new kernels: the twin's fp32 bits, radmmm_split_f16's pair bits, zeros, the flag ---------------------

@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("c,ldx", [(4, 8), (6, 8), (8, 8), (8, 9)])
def test_coupling_bwd_split_kernel_is_its_twin_plus_the_pair(c, ldx, scale):
    check, lib, ptr, s = _lib()
    g = torch.Generator().manual_seed(140 + c + ldx)
    nh, col0 = c // 2, ldx - c
    mask, lens = _mask().to(DEV), _lens()
    pad = 16                                    # the pair: the right half of [R, 2 C + pad], values then `pad` zeros
    S, Xs = _poisoned(g, R, C).to(DEV), _poisoned(g, R, ldx).to(DEV)
    dX0 = _poisoned(g, R, ldx, mag=1e-3)
    We, be = (0.05 * torch.randn(c, C, generator=g)).to(DEV), (0.05 * torch.randn(c, generator=g)).to(DEV)
    row = TG + 5                                # a valid row of item 1 for the planted value
    for rows_mode in (False, True):
        gls = (_poisoned(g, R, nh, mag=1e-3) if rows_mode else torch.tensor([-1e-3])).to(DEV)
        for planted in (False, True):
            dXin = dX0.clone()
            if planted:
                dXin[row, col0 + nh] = 1e30
            outs = []
            for split in (False, True):
                dX = dXin.clone().to(DEV)
                dO = torch.full((R, c), 7.0, device=DEV)
                dS = torch.full((R, 2 * C), 7.0, device=DEV)
                args = (ptr(S), C, ptr(We), ptr(be), ptr(Xs), ldx, ptr(dX), ldx, col0, nh, C, ptr(gls),
                        nh if rows_mode else 0, ptr(dO), ptr(dS[:, C:]), 2 * C)
                if not split:
                    check(lib.radmmm_wg_coupling_bwd(*args, ptr(lens), R, TG, s), "wg_coupling_bwd")
                else:
                    Ph, Pl = _pair(R, 2 * C + pad)
                    flag = _flag()
                    check(lib.radmmm_wg_coupling_bwd_split(*args, ptr(Ph[:, C:]), ptr(Pl[:, C:]), 2 * C + pad, C + pad,
                                                           scale, ptr(flag), ptr(lens), R, TG, s), "wg_coupling_bwd_split")
                outs.append((dX, dO, dS))
            (dX_t, dO_t, dS_t), (dX_s, dO_s, dS_s) = outs
            assert torch.isfinite(dS_t).all() and torch.isfinite(dO_t).all()
            assert torch.equal(dO_s, dO_t) and torch.equal(dS_s, dS_t)
            assert torch.equal(dX_s.view(torch.int32), dX_t.view(torch.int32))      # NaN tails in front included
            wh, wl = _split(dS_t[:, C:], C, scale, C + pad)
            assert torch.equal(Ph[:, C:], wh) and torch.equal(Pl[:, C:], wl)
            assert bool((Ph[:, :C] == 7.0).all()) and bool((Pl[:, :C] == 7.0).all())   # the left half is not this kernel's
            assert not Ph[:, 2 * C:].any() and not Pl[:, 2 * C:].any()                 # padding columns
            assert not Ph[~mask][:, C:].any() and not Pl[~mask][:, C:].any()           # rows past a length
            assert bool((Ph[mask][:, C:2 * C] != 0).any())
            assert int(flag.item()) == (1 if planted else 0), (rows_mode, planted, scale)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("layout", ["slice", "padded"])
def test_gate_bwd_split_kernel_is_its_twin_plus_the_pair(layout, scale):
    check, lib, ptr, s = _lib()
    g = torch.Generator().manual_seed(160)
    L, i = 3, 1
    mask, lens = _mask().to(DEV), _lens()
    A, cond = _poisoned(g, R, 2 * C).to(DEV), _poisoned(g, R, 2 * C * L).to(DEV)
    gy0 = _poisoned(g, R, C, mag=1e-3)
    # slice: columns [2 C i, 2 C (i + 1)) of a [R, 2 C L] pair, nothing else written; padded: [R, 2 C + 8], zeros behind
    ldp, off, pcols = (2 * C * L, 2 * C * i, 2 * C) if layout == "slice" else (2 * C + 8, 0, 2 * C + 8)
    for planted in (False, True):
        gy = gy0.clone()
        if planted:
            gy[5, 3] = 1e30
        gy = gy.to(DEV)
        twin = torch.full((R, 2 * C * L), 7.0, device=DEV)
        check(lib.radmmm_wg_gate_bwd(ptr(A), 2 * C, ptr(cond), 2 * C * L, 2 * C * i, ptr(gy), C, ptr(twin[:, 2 * C * i:]),
                                     2 * C * L, C, ptr(lens), R, TG, s), "wg_gate_bwd")
        dcond = torch.full((R, 2 * C * L), 7.0, device=DEV)
        Ph, Pl = _pair(R, ldp)
        flag = _flag()
        check(lib.radmmm_wg_gate_bwd_split(ptr(A), 2 * C, ptr(cond), 2 * C * L, 2 * C * i, ptr(gy), C,
                                           ptr(dcond[:, 2 * C * i:]), 2 * C * L, ptr(Ph[:, off:]), ptr(Pl[:, off:]), ldp,
                                           pcols, C, scale, ptr(flag), ptr(lens), R, TG, s), "wg_gate_bwd_split")
        assert torch.isfinite(twin).all() and torch.equal(dcond, twin)
        wh, wl = _split(twin[:, 2 * C * i:2 * C * (i + 1)], 2 * C, scale, pcols)
        assert torch.equal(Ph[:, off:off + pcols], wh) and torch.equal(Pl[:, off:off + pcols], wl)
        rest = torch.ones(ldp, dtype=torch.bool)
        rest[off:off + pcols] = False
        assert bool((Ph[:, rest] == 7.0).all()) and bool((Pl[:, rest] == 7.0).all())
        assert not Ph[:, off + 2 * C:off + pcols].any() and not Pl[:, off + 2 * C:off + pcols].any()
        assert not Ph[~mask][:, off:off + pcols].any() and not Pl[~mask][:, off:off + pcols].any()
        assert bool((Ph[mask][:, off:off + 2 * C] != 0).any())
        assert int(flag.item()) == (1 if planted else 0), (planted, scale)


# ---- 2. radmmm_rowgemm_h3 at the backward pass's shapes, narrow and wide kernel --------------------------------------
# Reference: float64 of the operands as stored (hi + lo, scales taken out).  Bar (tests/test_waveglow_half_gpu.py):
# |got - ref| <= (3 n 2^-24 + 2^-22) sum|a||w| per element, n = taps * K.
G_SCALE = 2.0 ** 17
NARROW = (3, 96, [96, 40, 1])                   # ceil(M / 128) * ceil(N / 256) < 128 workgroups: the narrow kernel
WIDE = (3, 5440, [5440, 1300, 1])               # 16 320 rows: 128 workgroups at N <= 256, the wide kernel
# (K, N, taps, dil, data gradient of an in_layer: sign -1 + add + postmask + Ch / Cl)
DGRAD_SHAPES = [(2 * C, C, 1, 1, False), (C, C, 1, 1, False), (2 * C, C, 3, 1, True), (2 * C, C, 3, 8, True),
                (2 * C * 4, 64, 1, 1, False)]


def _shifted64(A, W, B, Tg, dil, sign):
    """sum_tap A[r + sign (tap - taps // 2) dil] @ W[tap].T in float64, the shifted frame inside its item's [0, Tg)"""
    taps, N, K = W.shape
    out = torch.zeros(B, Tg, N, dtype=torch.float64)
    A3 = A.view(B, Tg, K)
    for tap in range(taps):
        sh = sign * (tap - taps // 2) * dil
        lo, hi = max(0, -sh), min(Tg, Tg - sh)
        if hi > lo:
            out[:, lo:hi] += A3[:, lo + sh:hi + sh] @ W[tap].T
    return out.view(B * Tg, N)


def _dgrad_case(K, N, taps, dil, in_layer, B, Tg, lens_l):
    from rad_mmm_amd import ops
    from rad_mmm_amd._lib import rowgemm_h3
    g = torch.Generator().manual_seed(K + N + 7 * taps + dil)
    M = B * Tg
    valid = _mask(lens_l, Tg)
    A = 1e-4 * torch.randn(M, K, generator=g)
    A[~valid] = 0.0                             # a gradient operand: its producer wrote zeros past every length
    W = torch.randn(taps, N, K, generator=g) / float(taps * K) ** 0.5
    lda = 2 * C if K == C else K                # K = C: the right half of a [M, 2 C] pair (the last layer's d S)
    Ah, Al = _pair(M, lda)
    h, l = _split(A.to(DEV), K, G_SCALE, K)
    Ah[:, lda - K:], Al[:, lda - K:] = h, l
    Wh, Wl = _split(W.view(taps * N, K).to(DEV), K, ops.W_SCALE, K)
    a64 = (h.double().cpu() + l.double().cpu()) / G_SCALE
    w64 = ((Wh.double().cpu() + Wl.double().cpu()) / ops.W_SCALE).view(taps, N, K)
    lens = _lens(lens_l)
    ldc = 2 * C if in_layer else N
    Cd = torch.full((M, ldc), 7.0, device=DEV)
    kw = dict(Ah=Ah[:, lda - K:], Al=Al[:, lda - K:], lda_h=lda, Bh=Wh, Bl=Wl, ldb_h=K, b_tap_stride_h=N * K,
              acc_scale=1.0 / (G_SCALE * ops.W_SCALE), nprod=3, C=Cd, ldc=ldc, M=M, N=N, K=K, taps=taps, dil=dil, T=Tg,
              lens=lens)
    sign = -1 if in_layer else 1
    add = 1e-4 * torch.randn(M, N, generator=g)
    if in_layer:                                # fp32 in place in the left half of [d H | d S], the pair beside it
        Cd[:, :N] = add.to(DEV)
        Ch, Cl = _pair(M, 2 * C)
        flag = _flag()
        kw.update(sign=-1, a_mask_mode=0, add=Cd, ldadd=ldc, postmask=1, Ch=Ch, Cl=Cl, ldch=2 * C, ch_scale=G_SCALE,
                  sat_flag=flag)
    elif N == 64:                               # cond_layer's data gradient: added to the previous flow's
        addd = add.to(DEV)
        kw.update(add=addd, ldadd=N)
    rowgemm_h3(**kw)
    ref = _shifted64(a64, w64, B, Tg, dil, sign)
    mag = _shifted64(a64.abs(), w64.abs(), B, Tg, dil, sign)
    if in_layer or N == 64:
        ref = ref + add.double()
    if in_layer:
        ref, mag = ref * valid[:, None], mag * valid[:, None]
    n = taps * K
    bound = (3 * n * 2.0 ** -24 + 2.0 ** -22) * mag
    got = Cd[:, :N]
    err = (got.double().cpu() - ref).abs()
    assert torch.isfinite(got).all()
    some = mag > 0
    if in_layer:
        assert not got.cpu()[~valid].any()      # postmask: exact zeros past every length
        wh, wl = _split(got, N, G_SCALE, N)
        assert torch.equal(Ch[:, :N], wh) and torch.equal(Cl[:, :N], wl)
        assert bool((Ch[:, N:] == 7.0).all()) and bool((Cd[:, N:] == 7.0).all()) and int(flag.item()) == 0
    ratio = (err[some] / bound[some]).max().item()
    print(f"rowgemm_h3 backward shape K {K} N {N} taps {taps} dil {dil} sign {sign} M {M}: worst error / bound "
          f"{ratio:.3f} (max-abs error {err.max().item():.3e})")
    assert ratio <= 1.0


@pytest.mark.parametrize("K,N,taps,dil,in_layer", DGRAD_SHAPES)
def test_rowgemm_h3_at_the_backward_shapes(K, N, taps, dil, in_layer):
    _dgrad_case(K, N, taps, dil, in_layer, *NARROW)


@pytest.mark.parametrize("K,N,taps,dil,in_layer", DGRAD_SHAPES)
def test_rowgemm_h3_at_the_backward_shapes_on_the_wide_kernel(K, N, taps, dil, in_layer):
    _dgrad_case(K, N, taps, dil, in_layer, *WIDE)


# ---- 3. radmmm_wgrad_rm at WaveGlow's shapes with lengths ------------------------------------------------------------

@pytest.mark.parametrize("Mc,Nc,taps,dil", [(2 * C, C, 1, 1), (C, C, 1, 1), (2 * C, C, 3, 8), (2 * C * 4, 64, 1, 1)])
def test_wgrad_rm_at_waveglow_shapes_with_lengths(Mc, Nc, taps, dil):
    from rad_mmm_amd import ops
    g = torch.Generator().manual_seed(300 + Mc + Nc + taps)
    B = len(LENS)
    mask, lens = _mask(), _lens()
    GY = 1e-4 * torch.randn(R, Mc, generator=g)
    GY[~mask] = 0.0                             # a gradient pair: zeros past every length
    X = torch.randn(R, Nc, generator=g)
    ldg = 2 * C if Mc == C else (2 * C * 4 if taps == 3 else Mc)      # a column slice of a wider pair, as the step's
    Gh, Gl = _pair(R, ldg)
    h, l = _split(GY.to(DEV), Mc, G_SCALE, Mc)
    Gh[:, ldg - Mc:], Gl[:, ldg - Mc:] = h, l
    Xh, Xl = _split(X.to(DEV), Nc, 1.0, Nc)
    gy64 = (h.double().cpu() + l.double().cpu()) / G_SCALE
    x64 = Xh.double().cpu() + Xl.double().cpu()
    Xh[~mask.to(DEV)] = float("nan")            # x rows past a length are masked: never fetched
    Xl[~mask.to(DEV)] = float("nan")
    P = ops.wgrad_rm_slabs((Gh[:, ldg - Mc:], Gl[:, ldg - Mc:]), (Xh, Xl), B, TG, Mc, Nc, taps, dil, 1.0 / G_SCALE, lens)
    got = P.sum(0).double().cpu()
    ref, mag = torch.zeros(taps, Mc, Nc, dtype=torch.float64), torch.zeros(taps, Mc, Nc, dtype=torch.float64)
    for b, n in enumerate(LENS):
        gb, xb = gy64[b * TG:b * TG + n], x64[b * TG:b * TG + n]
        for tap in range(taps):
            sh = (tap - taps // 2) * dil
            lo, hi = max(0, -sh), min(n, n - sh)
            if hi > lo:
                ref[tap] += gb[lo:hi].T @ xb[lo + sh:hi + sh]
                mag[tap] += gb[lo:hi].abs().T @ xb[lo + sh:hi + sh].abs()
    n_rows = sum(LENS)
    bound = (3 * n_rows * 2.0 ** -24 + 2.0 ** -22) * mag
    err = (got - ref).abs()
    assert torch.isfinite(P).all() and bool((mag > 0).all())
    ratio = (err / bound).max().item()
    print(f"wgrad_rm Mc {Mc} Nc {Nc} taps {taps} dil {dil}, {P.shape[0]} slabs: worst error / bound {ratio:.3f} "
          f"(max-abs error {err.max().item():.3e})")
    assert ratio <= 1.0


# ---- 4. .. 11. the step as a whole -----------------------------------------------------------------------------------

def _train_model(cfg, sd, weight_norm=True, mode="h3"):
    from rad_mmm_amd.waveglow import WaveGlow
    m = WaveGlow(**cfg)
    if weight_norm:
        m.apply_weight_norm()
    m.load_state_dict(sd)
    m.train_precision = mode
    return m.to(DEV).train()


def _grads(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def _step(m, mel, audio, lens=None, **kw):
    m.zero_grad(set_to_none=True)
    loss = m.nll_loss(mel, audio, lens, **kw)
    loss.backward()
    return loss.detach(), _grads(m)


def _same_bits(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


def _bars(bwd):
    """4 x the fp32 test's bars"""
    return {k[len("f32_vs_f64/"):]: 4 * max(10 * float(v), 1e-6) for k, v in bwd.items() if k.startswith("f32_vs_f64/")}


def _class_bars(bwd, names):
    bars = _bars(bwd)
    by_class = {}
    for k, v in bars.items():
        c = re.sub(r"^(WN|convinv)\.\d+\.", r"\1.*.", k)
        by_class[c] = max(by_class.get(c, 0.0), v)
    return {k: bars.get(k, by_class[re.sub(r"^(WN|convinv)\.\d+\.", r"\1.*.", k)]) for k in names}


@pytest.fixture(scope="module")
def tiny(golden):
    """the two fixtures, the weight-normed model under train_precision "h3", the equal-length batch, one step on it"""
    fwd, bwd = golden("waveglow_fwd_tiny.npz"), golden("waveglow_bwd_tiny.npz")
    cfg, sd = load_fixture(fwd)
    m = _train_model(cfg, sd)
    n = int(fwd["eq_T"])
    mel = torch.from_numpy(fwd["mel"][:, :, :n].copy()).to(DEV)
    audio = torch.from_numpy(fwd["audio"][:, :n * HOP].copy()).to(DEV)
    loss, grads = _step(m, mel, audio)
    return fwd, bwd, cfg, sd, m, mel, audio, loss, grads


@pytest.fixture(scope="module")
def ragged(tiny):
    """the fp32 test's ragged batch, one "h3" step on it and the float64 restatement's gradients"""
    fwd, bwd, cfg, sd, m = tiny[:5]
    g = torch.Generator().manual_seed(19)
    T = max(RAGGED)
    mel = torch.randn(len(RAGGED), 8, T, generator=g) - 2.0
    audio = 0.3 * torch.randn(len(RAGGED), T * HOP, generator=g)
    ref_loss, ref = grads_ref(sd, cfg, mel, audio, RAGGED)
    mel, audio = mel.to(DEV), audio.to(DEV)
    loss, grads = _step(m, mel, audio, RAGGED)
    return mel, audio, loss, grads, ref_loss, ref


def _compare(what, grads, ref, bars):
    worst, bad = 0.0, []
    for k in sorted(bars):
        err = rel_l2(grads[k].cpu().numpy(), ref(k))
        worst = max(worst, err / bars[k])
        print(f"{what} {k}: relative L2 {err:.3e} (bar {bars[k]:.3e})")
        if not err <= bars[k]:
            bad.append((k, err, bars[k]))
        assert torch.isfinite(grads[k]).all(), k
    print(f"{what}: worst measured / bar {worst:.3f}")
    assert not bad, bad


def test_h3_gradients_match_the_reference_fixture(tiny):
    fwd, bwd, cfg, sd, m, mel, audio, loss, grads = tiny
    bar = 4 * max(10 * float(fwd["f32_vs_f64_loss"]), 1e-6)
    d = abs(float(loss) - float(bwd["loss64"]))
    print(f"h3 loss {float(loss):.9f}, {d:.3e} from the reference's float64 (bar {bar:.3e}, measured / bar {d / bar:.3f})")
    assert loss.dtype == torch.float64 and d <= bar
    bars = _bars(bwd)
    assert set(grads) == set(sd) and set(grads) >= set(bars) and mel.grad is None and audio.grad is None
    _compare("h3 nll_loss", grads, lambda k: bwd["grad/" + k], bars)


def test_h3_reference_training_lines(tiny):
    from rad_mmm_amd.waveglow import WaveGlowLoss
    fwd, bwd, cfg, sd, m, mel, audio, loss1, grads1 = tiny
    m.zero_grad(set_to_none=True)
    out = m((mel, audio))
    assert out[0].grad_fn is not None
    loss = WaveGlowLoss(1.0)(out)
    loss.backward()
    grads = _grads(m)
    assert abs(float(loss.detach()) - float(loss1)) <= 1e-9
    _compare("h3 forward + WaveGlowLoss", grads, lambda k: bwd["grad/" + k], _bars(bwd))


def test_h3_ragged_batch(tiny, ragged):
    fwd, bwd = tiny[:2]
    mel, audio, loss, grads, ref_loss, ref = ragged
    bar = 4 * max(10 * float(fwd["f32_vs_f64_loss"]), 1e-6)
    d = abs(float(loss) - ref_loss)
    print(f"h3 ragged loss {float(loss):.9f}, {d:.3e} from the restatement (bar {bar:.3e}, measured / bar {d / bar:.3f})")
    assert d <= bar
    assert set(grads) == set(ref)
    _compare("h3 ragged", grads, lambda k: ref[k].numpy(), _class_bars(bwd, ref))


def test_h3_bits_are_repeatable_and_tails_lengths_and_nan_do_not_matter(tiny, ragged):
    m = tiny[4]
    mel, audio, loss, grads, _, _ = ragged
    loss2, again = _step(m, mel, audio, RAGGED)                                  # two steps: the same bits
    assert torch.equal(loss, loss2) and _same_bits(grads, again)
    dl = torch.tensor(RAGGED, dtype=torch.int32, device=DEV)                     # device lengths: the same bits
    loss3, dev = _step(m, mel, audio, dl)
    assert torch.equal(loss, loss3) and _same_bits(grads, dev)
    pa, pm = audio.clone(), mel.clone()
    for b, n in enumerate(RAGGED):
        pa[b, n * HOP:] = float("nan")
        pm[b, :, n:] = float("nan")
    loss4, nan = _step(m, pm, pa, RAGGED)                                        # what lies past a length reaches nothing
    assert torch.equal(loss, loss4) and _same_bits(grads, nan)
    assert m.grad_saturated() is False


def test_the_mode_is_really_taken(tiny, ragged):
    fwd, bwd, cfg, sd, m = tiny[:5]
    mel, audio, loss, grads, _, _ = ragged
    never = _train_model(cfg, sd, mode="fp32")
    loss32, grads32 = _step(never, mel, audio, RAGGED)
    assert not torch.equal(loss, loss32)
    differ = [k for k in grads if not torch.equal(grads[k], grads32[k])]
    print(f"h3 against fp32: {len(differ)} of {len(grads)} gradients differ in their bits")
    assert len(differ) > len(grads) // 2 and any("in_layers" in k for k in differ) and any("cond_layer" in k for k in differ)
    lossp, gradsp = _step(m, mel, audio, RAGGED, precision="fp32")               # per call
    assert torch.equal(lossp, loss32) and _same_bits(gradsp, grads32)
    m.train_precision = "fp32"                                                   # and by the attribute
    try:
        lossb, back = _step(m, mel, audio, RAGGED)
    finally:
        m.train_precision = "h3"
    assert torch.equal(lossb, loss32) and _same_bits(back, grads32)
    lossh, gradsh = _step(never, mel, audio, RAGGED, precision="h3")
    assert torch.equal(lossh, loss) and _same_bits(gradsh, grads)


@pytest.mark.parametrize("mode", ["fp32", "h3"])
def test_train_step_event_families(tiny, mode):
    """the per-family device event lists of one step (tools/waveglow_bench.py --train reads them), counted from the
    config: the forward's families once per flow / layer (the recomputation is not timed by family), the backward's
    bwd_* families, the conditioning in both passes (one chunk)"""
    cfg, m, mel, audio = tiny[2], tiny[4], tiny[5], tiny[6]
    F, L = cfg["n_flows"], cfg["WN_config"]["n_layers"]
    m._train_events = events = {}
    try:
        _step(m, mel, audio, precision=mode)
    finally:
        m._train_events = None
    assert events.pop("rows") == mel.shape[0] * mel.shape[2] * HOP // cfg["n_group"]
    want = {"upsample": 2, "group_audio": 1, "mix_fwd": F, "start": F, "cond_layer": F, "in_layers": F * L, "gate": F * L,
            "res_skip_gemm": F * L, "res_skip_update": F * L, "end_coupling_fwd": F, "nll_parts": 1,
            "bwd_recompute": F, "bwd_coupling": F, "bwd_start": F, "bwd_cond_layer": F, "bwd_mix": F,
            "bwd_res_skip": F * L, "bwd_gate": F * L, "bwd_in_layers": F * L, "bwd_upsample": 1}
    if mode == "h3":
        want["split_cond"] = 2                          # the conditioning rows are split in the forward and in the backward
    assert {k: len(v) for k, v in events.items()} == want


def test_h3_chunked_step(tiny, ragged):
    m = tiny[4]
    mel, audio, loss, grads, _, _ = ragged
    m._train_chunk_items = 2
    try:
        loss2, chunked = _step(m, mel, audio, RAGGED)
    finally:
        m._train_chunk_items = None
    worst = max(rel_l2(chunked[k].cpu().numpy(), grads[k].cpu().numpy()) for k in grads)
    print(f"h3 chunks of 2 items: worst relative L2 {worst:.3e}, loss {abs(float(loss2) - float(loss)):.3e}")
    assert worst <= 1e-6 and abs(float(loss2) - float(loss)) <= 1e-12


def test_h3_shipped_wn_size_against_fp64_restatement():
    # n_channels 256, n_layers 8, K = 640: one item of 2 frames = 64 group steps, two flows.  Bar: the fp32 test's 1e-5 x 4
    cfg = dict(n_mel_channels=80, n_flows=2, n_group=8, n_early_every=4, n_early_size=2, WN_config=SHIPPED_WN)
    sd = random_state(cfg, 7)
    m = _train_model(cfg, sd, weight_norm=False)
    g = torch.Generator().manual_seed(8)
    T = 2
    mel = torch.randn(1, 80, T, generator=g) - 2.0
    audio = 0.3 * torch.randn(1, T * HOP, generator=g)
    ref_loss, ref = grads_ref(sd, cfg, mel, audio, [T])
    loss, grads = _step(m, mel.to(DEV), audio.to(DEV), [T])
    print(f"h3 shipped WN size: loss {float(loss):.7f} against {ref_loss:.7f}")
    _compare("h3 shipped WN size", grads, lambda k: ref[k].numpy(), {k: 4e-5 for k in ref})
    assert m.grad_saturated() is False


def test_h3_no_device_to_host_sync_with_host_lengths(tiny):
    fwd, _, _, _, m = tiny[:5]
    mel, audio = torch.from_numpy(fwd["mel"]).to(DEV), torch.from_numpy(fwd["audio"]).to(DEV)
    _step(m, mel, audio, [7, 4])                             # warm
    torch.cuda.synchronize()
    m.zero_grad(set_to_none=True)
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = m.nll_loss(mel, audio, [7, 3])
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert loss.is_cuda and torch.isfinite(loss) and all(torch.isfinite(p.grad).all() for p in m.parameters())


def test_h3_three_adam_steps(tiny):
    fwd, bwd, cfg, sd, _, mel, audio = tiny[:7]
    n = mel.shape[2]
    leaves = leaves_of(sd)
    opt = torch.optim.Adam(list(leaves.values()), lr=1e-4)
    want = []
    for _ in range(3):
        opt.zero_grad()
        loss = loss_ref(leaves, cfg, mel.cpu(), audio.cpu(), [n, n])
        loss.backward()
        opt.step()
        want.append(float(loss.detach()))
    runs = []
    for _ in range(2):
        m = _train_model(cfg, sd)
        opt = torch.optim.Adam(m.parameters(), lr=1e-4)
        losses = []
        for _ in range(3):
            opt.zero_grad()
            loss = m.nll_loss(mel, audio)
            loss.backward()
            opt.step()
            losses.append(loss.detach())
        runs.append((torch.stack(losses), {k: v.detach().clone() for k, v in m.state_dict().items()}))
    bar = 4 * 10 * max(10 * float(fwd["f32_vs_f64_loss"]), 1e-6)
    got = runs[0][0].tolist()
    worst = max(abs(a - b) for a, b in zip(got, want))
    print(f"h3 three Adam steps: losses {got} against {want} (bar {bar:.3e}, worst / bar {worst / bar:.3f})")
    assert want[2] < want[0]
    assert worst <= bar
    assert torch.equal(runs[0][0], runs[1][0]) and _same_bits(runs[0][1], runs[1][1])


def test_grad_scale_overrides(tiny):
    from rad_mmm_amd.waveglow import auto_grad_scale
    fwd, bwd, cfg, sd, m, mel, audio, loss, grads = tiny
    auto = auto_grad_scale(mel.shape[0] * mel.shape[2] * HOP)
    m.grad_saturated()                                       # clear whatever an earlier test left
    try:
        m.grad_scale = auto / 2.0 ** 12                      # the hi planes go subnormal: still finite, nothing clamps
        loss_lo, lo = _step(m, mel, audio)
        assert torch.equal(loss_lo, loss)                    # the forward does not see the scale
        assert all(torch.isfinite(v).all() for v in lo.values()) and m.grad_saturated() is False
        assert not _same_bits(lo, grads)                     # the override is taken
        worst = max(rel_l2(lo[k].cpu().numpy(), grads[k].cpu().numpy()) for k in grads)
        m.grad_scale = auto * 2.0 ** 10
        _, hi = _step(m, mel, audio)
        sat = m.grad_saturated()
        worst_hi = max(rel_l2(hi[k].cpu().numpy(), grads[k].cpu().numpy()) for k in grads
                       if torch.isfinite(hi[k]).all())
        print(f"grad_scale auto = 2^{int(auto).bit_length() - 1}: auto / 2^12 worst relative L2 to the automatic step "
              f"{worst:.3e}, not saturated; auto x 2^10: grad_saturated() {sat}, worst relative L2 {worst_hi:.3e}")
        assert isinstance(sat, bool) and m.grad_saturated() is False       # read once, then clear
    finally:
        m.grad_scale = None
    _, back = _step(m, mel, audio)
    assert _same_bits(back, grads)
