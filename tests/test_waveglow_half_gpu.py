"""GPU checks of WaveGlow.infer's 16-bit GEMM modes "h3" and "f16" (rad_mmm_amd/waveglow.py `precision`): the three
kernels that write a GEMM's split operand in the pass that computes the value, bit for bit against their fp32 twins and
radmmm_split_f16; radmmm_rowgemm_h3 at WaveGlow's shapes against float64 of the operands as stored, with bars derived
from the formats; both modes end to end against the fp64 restatement (tests/_waveglow_ref.py) and its emulation of the
operand rounding (tests/_waveglow_half_ref.py); and the properties the fp32 path has (repeatable bits, zero tails, device
lengths, NaN past the lengths, batch invariance).

Measured on an MI355X (the tests print each figure): the GEMM's worst error / bar 0.026 (one product) and 0.013 (three);
"h3" 8.9e-7 / 1.1e-6 max-abs on the tiny fixture and 2.9e-6 max-abs, 4.4e-7 rel-L2 at the shipped WN size; "f16" rel-L2
against exact 5.75e-5 / 5.77e-5 (emulation 5.80e-5 / 5.63e-5) on the tiny items and 3.74e-4 / 3.34e-4 (emulation 3.81e-4 /
3.60e-4) at the shipped WN size; an item in a batch against the item alone: 0 in both modes."""
import numpy as np
import pytest
import torch

from _waveglow_ref import HOP, TINY, load_fixture, noise_channels, random_state
from _waveglow_half_ref import item_refs, rel_l2, shipped_case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MODES = ("h3", "f16")


def _lib():
    from rad_mmm_amd._lib import check, lib, ptr, stream
    return check, lib, ptr, stream()


def _model(cfg, sd):
    from rad_mmm_amd.waveglow import WaveGlow
    m = WaveGlow(**cfg)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


# ---- 1. the three split-writing kernels, exact -----------------------------------------------------------------------
K_LENS, K_TG = [40, 17, 1], 40


def _spread(g, *shape):
    """values from fp16's subnormal range up to about 1e3, both signs"""
    mag = 10.0 ** (torch.rand(*shape, generator=g) * 11.0 - 8.0)
    return (mag * (torch.randint(0, 2, shape, generator=g) * 2 - 1)).float()


def _valid_rows(lens, T):
    return (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).reshape(-1)


def _nan_tails(x, valid):
    x = x.clone()
    x[~valid] = float("nan")
    return x


def _split(x, C, ldp):
    from rad_mmm_amd import ops
    return ops.split_f16(x, C, 1.0, ldp, 3)


def _pair(R, ldp):
    return (torch.full((R, ldp), 7.0, device=DEV, dtype=torch.float16),
            torch.full((R, ldp), 7.0, device=DEV, dtype=torch.float16))


def _check_pair(Ph, Pl, want, C, valid, with_lo):
    """the pair against radmmm_split_f16 of the twin's fp32 output; tails and padding columns exactly zero"""
    wh, wl = _split(want, C, Ph.shape[1])
    assert torch.equal(Ph, wh)
    assert not Ph[:, C:].any() and not Ph[~valid.to(DEV)].any()
    assert bool((Ph[valid.to(DEV)][:, :C] != 0).any())
    if with_lo:
        assert torch.equal(Pl, wl)
        assert not Pl[:, C:].any() and not Pl[~valid.to(DEV)].any()
    else:
        assert bool((Pl == 7.0).all())                  # the lo array was not passed: nothing may have written it


@pytest.mark.parametrize("with_lo", [True, False])
@pytest.mark.parametrize("C", [32, 256])
def test_start_split_kernel_is_its_twin_plus_the_pair(C, with_lo):
    check, lib, ptr, s = _lib()
    g = torch.Generator().manual_seed(100 + C)
    R, ng, ldp = len(K_LENS) * K_TG, 8, C + 8
    valid = _valid_rows(K_LENS, K_TG)
    lens = torch.tensor(K_LENS, dtype=torch.int32, device=DEV)
    X = _nan_tails(_spread(g, R, ng), valid).to(DEV)
    for nh in (2, 3, 4):
        col0 = ng - 2 * nh
        W, b = _spread(g, C, nh).to(DEV), _spread(g, C).to(DEV)
        H0 = torch.full((R, C), 7.0, device=DEV)
        check(lib.radmmm_wg_start(ptr(X), ng, col0, nh, ptr(W), ptr(b), ptr(H0), C, C, ptr(lens), R, K_TG, s), "wg_start")
        H = torch.full((R, C), 7.0, device=DEV)
        Ph, Pl = _pair(R, ldp)
        check(lib.radmmm_wg_start_split(ptr(X), ng, col0, nh, ptr(W), ptr(b), ptr(H), C, ptr(Ph),
                                        ptr(Pl) if with_lo else None, ldp, C, ptr(lens), R, K_TG, s), "wg_start_split")
        assert torch.isfinite(H0).all() and torch.equal(H, H0)
        _check_pair(Ph, Pl, H0, C, valid, with_lo)


@pytest.mark.parametrize("with_lo", [True, False])
@pytest.mark.parametrize("C", [32, 256])
def test_gate_split_kernel_is_its_twin_as_a_pair(C, with_lo):
    check, lib, ptr, s = _lib()
    g = torch.Generator().manual_seed(200 + C)
    R, L, i, ldp = len(K_LENS) * K_TG, 3, 2, C + 8
    valid = _valid_rows(K_LENS, K_TG)
    lens = torch.tensor(K_LENS, dtype=torch.int32, device=DEV)
    a = _nan_tails(_spread(g, R, 2 * C), valid).to(DEV)
    a[:, :C] *= 1e-3                                     # tanh's argument also where tanh is not saturated
    cond = _nan_tails(_spread(g, R, 2 * C * L) * 1e-2, valid).to(DEV)
    y = torch.full((R, C), 7.0, device=DEV)
    check(lib.radmmm_wg_gate(ptr(a), 2 * C, ptr(cond), 2 * C * L, 2 * C * i, ptr(y), C, C, ptr(lens), R, K_TG, s), "wg_gate")
    Ph, Pl = _pair(R, ldp)
    check(lib.radmmm_wg_gate_split(ptr(a), 2 * C, ptr(cond), 2 * C * L, 2 * C * i, ptr(Ph), ptr(Pl) if with_lo else None,
                                   ldp, C, ptr(lens), R, K_TG, s), "wg_gate_split")
    assert torch.isfinite(y).all()
    _check_pair(Ph, Pl, y, C, valid, with_lo)


@pytest.mark.parametrize("with_lo", [True, False])
@pytest.mark.parametrize("C", [32, 256])
def test_res_skip_split_kernel_is_its_twin_plus_the_pair(C, with_lo):
    check, lib, ptr, s = _lib()
    g = torch.Generator().manual_seed(300 + C)
    R, ldp = len(K_LENS) * K_TG, C + 8
    valid = _valid_rows(K_LENS, K_TG)
    lens = torch.tensor(K_LENS, dtype=torch.int32, device=DEV)
    rs, H0, S0 = (_nan_tails(_spread(g, R, n), valid).to(DEV) for n in (2 * C, C, C))
    for first, last in ((1, 0), (0, 0), (0, 1), (1, 1)):
        Ht, St = H0.clone(), S0.clone()
        check(lib.radmmm_wg_res_skip(ptr(rs), 2 * C, ptr(Ht), C, ptr(St), C, C, first, last, ptr(lens), R, K_TG, s),
              "wg_res_skip")
        H, S = H0.clone(), S0.clone()
        Ph, Pl = _pair(R, ldp)
        check(lib.radmmm_wg_res_skip_split(ptr(rs), 2 * C, ptr(H), C, ptr(S), C, ptr(Ph), ptr(Pl) if with_lo else None, ldp,
                                           C, first, last, ptr(lens), R, K_TG, s), "wg_res_skip_split")
        assert torch.isfinite(St).all() and torch.equal(S, St)
        if last:                                        # H and the pair are not touched (the NaN tails of H0 included)
            assert torch.equal(H.view(torch.int32), H0.view(torch.int32))
            assert bool((Ph == 7.0).all()) and bool((Pl == 7.0).all())
        else:
            assert torch.isfinite(Ht).all() and torch.equal(H, Ht)
            _check_pair(Ph, Pl, Ht, C, valid, with_lo)
    # with last the kernel takes no H and no pair at all (St: the twin's S of the loop's last case, first = last = 1)
    S = S0.clone()
    check(lib.radmmm_wg_res_skip_split(ptr(rs), 2 * C, None, 0, ptr(S), C, None, None, 0, C, 1, 1, ptr(lens), R, K_TG, s),
          "wg_res_skip_split")
    assert torch.equal(S, St)


# ---- 2. radmmm_rowgemm_h3 at WaveGlow's shapes against float64 of the operands as stored ----------------------------
# Bars (products of two fp16 values are exact in fp32; n = taps * K terms are added in fp32, unit roundoff 2^-24):
#   nprod 1: |got - ref| <= n 2^-24 sum|a||w| per element, ref = the float64 product of the hi operands
#   nprod 3: |got - ref| <= (3 n 2^-24 + 2^-22) sum|a||w|, ref = the float64 product of the (hi + lo) operands: three
#            times the terms, and the dropped lo.lo term, |lo| <= 2^-11 |hi + lo| on both sides
G_B, G_TG, G_LENS = 3, 96, [96, 40, 1]
GEMM_SHAPES = [(256, 512, 3, 1), (256, 512, 3, 64), (256, 512, 3, 128), (256, 512, 1, 1), (256, 256, 1, 1),
               (640, 4096, 1, 1), (32, 64, 3, 8), (64, 256, 1, 1)]
# the same GEMM where the launcher takes the wide-tile kernel (ceil(M / 128) * ceil(N / 256) >= 128 workgroups): the
# benchmark's and every long utterance's path, which the small cases above never reach
W_B, W_TG, W_LENS = 3, 2752, [2752, 1300, 1]
GEMM_SHAPES_WIDE = [(256, 512, 3, 64), (256, 512, 1, 1), (640, 1024, 1, 1)]


def _conv_rows64(A, W, lens, Tg, dil):
    """sum_tap Am[r + (tap - taps // 2) * dil] @ W[tap].T in float64 for every row; Am = A inside its item's length,
    else 0 (a_mask_mode 1 masks the SOURCE frame: an output row past the length still sums the taps that reach back)"""
    taps, N, _ = W.shape
    out = torch.zeros(A.shape[0], N, dtype=torch.float64)
    for b, n in enumerate(lens):
        Ab = A[b * Tg:b * Tg + n]
        for tap in range(taps):
            s = (tap - taps // 2) * dil
            lo, hi = max(0, -s), min(Tg, n - s)         # output frames t of the item with 0 <= t + s < n
            if hi > lo:
                out[b * Tg + lo:b * Tg + hi] += Ab[lo + s:hi + s] @ W[tap].T
    return out


def _gemm_case(K, N, taps, dil, nprod, B, Tg, lens_l):
    from rad_mmm_amd import ops
    from rad_mmm_amd._lib import rowgemm_h3
    g = torch.Generator().manual_seed(K + N + 7 * taps + dil)
    M = B * Tg
    valid = _valid_rows(lens_l, Tg)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(taps, N, K, generator=g) / float(np.sqrt(taps * K))
    bias = 0.1 * torch.randn(N, generator=g)
    Ah, Al = ops.split_f16(A.to(DEV), K, 1.0, K, 3)
    Wh, Wl = ops.split_f16(W.view(taps * N, K).to(DEV), K, ops.W_SCALE, K, 3)
    a64 = Ah.double().cpu() + (Al.double().cpu() if nprod == 3 else 0.0)
    w64 = ((Wh.double().cpu() + (Wl.double().cpu() if nprod == 3 else 0.0)) / ops.W_SCALE).view(taps, N, K)
    Ah[~valid.to(DEV)] = float("nan")                   # rows past a length are masked A rows: never fetched
    Al[~valid.to(DEV)] = float("nan")
    if nprod == 1:                                      # single-product mode: the hi arrays stand in for both pointers
        Al, Wl = Ah, Wh
    lens = torch.tensor(lens_l, dtype=torch.int32, device=DEV)
    C = torch.full((M, N), 7.0, device=DEV)
    rowgemm_h3(Ah=Ah, Al=Al, lda_h=K, Bh=Wh, Bl=Wl, ldb_h=K, b_tap_stride_h=N * K, acc_scale=1.0 / ops.W_SCALE, nprod=nprod,
               C=C, ldc=N, M=M, N=N, K=K, taps=taps, dil=dil, T=Tg, lens=lens, a_mask_mode=1, bias=bias.to(DEV))
    ref = _conv_rows64(a64, w64, lens_l, Tg, dil) + bias.double()
    mag = _conv_rows64(a64.abs(), w64.abs(), lens_l, Tg, dil)
    n = taps * K
    bound = (n * 2.0 ** -24 if nprod == 1 else 3 * n * 2.0 ** -24 + 2.0 ** -22) * mag
    err = (C.double().cpu() - ref).abs()
    assert torch.isfinite(C).all()
    some = mag > 0
    assert not err[~some].any()                         # every tap masked: the bias alone, exactly
    ratio = (err[some] / bound[some]).max().item()
    print(f"rowgemm_h3 nprod {nprod} K {K} N {N} taps {taps} dil {dil} M {M}: worst error / bound {ratio:.3f} "
          f"(max-abs error {err.max().item():.3e})")
    assert ratio <= 1.0


@pytest.mark.parametrize("nprod", [1, 3])
@pytest.mark.parametrize("K,N,taps,dil", GEMM_SHAPES)
def test_rowgemm_h3_at_waveglow_shapes(K, N, taps, dil, nprod):
    _gemm_case(K, N, taps, dil, nprod, G_B, G_TG, G_LENS)


@pytest.mark.parametrize("nprod", [1, 3])
@pytest.mark.parametrize("K,N,taps,dil", GEMM_SHAPES_WIDE)
def test_rowgemm_h3_at_waveglow_shapes_on_the_wide_kernel(K, N, taps, dil, nprod):
    _gemm_case(K, N, taps, dil, nprod, W_B, W_TG, W_LENS)


# ---- 3. / 4. end to end --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(golden):
    """the reference's recorded fixture + per item the exact fp64 restatement and its f16 emulation"""
    d = golden("waveglow_tiny.npz")
    cfg, sd = load_fixture(d)
    mel = torch.from_numpy(d["mel"])
    noise = [torch.from_numpy(d[f"noise{i}"]) for i in range(3)]
    lens, sigma = d["lens"].tolist(), float(d["sigma"])
    refs = item_refs(sd, cfg, mel, lens, noise, sigma, ("exact", "f16"))
    return dict(d=d, cfg=cfg, model=_model(cfg, sd), mel=mel.to(DEV), noise=[z.to(DEV) for z in noise], lens=lens,
                sigma=sigma, refs=refs)


@pytest.fixture(scope="module")
def shipped():
    cfg, sd, mel, lens, noise, sigma = shipped_case()
    refs = item_refs(sd, cfg, mel, lens, noise, sigma, ("exact", "f16"))
    return dict(cfg=cfg, model=_model(cfg, sd), mel=mel.to(DEV), noise=[z.to(DEV) for z in noise], lens=lens, sigma=sigma,
                refs=refs)


def _infer(case, mode, **kw):
    return case["model"].infer(case["mel"], case["lens"], sigma=case["sigma"], noise=case["noise"], precision=mode, **kw)


def _alone(case, b, mode):
    n, per = case["lens"][b], HOP // case["cfg"]["n_group"]
    return case["model"].infer(case["mel"][b:b + 1, :, :n], [n], sigma=case["sigma"],
                               noise=[z[b:b + 1, :, :n * per] for z in case["noise"]], precision=mode)[0]


def test_h3_matches_the_reference_fixture(tiny):
    d, lens = tiny["d"], tiny["lens"]
    y = _infer(tiny, "h3").cpu().numpy()
    assert y.shape == d["audio"].shape
    for b, n in enumerate(lens):
        ref = d["audio"][b, :n * HOP]
        err = np.abs(y[b, :n * HOP] - ref).max()
        print(f"h3 item {b} ({n} frames): max-abs {err:.3e} (|ref| max {np.abs(ref).max():.3f})")
        assert err <= 1e-4 * max(1.0, np.abs(ref).max())
        assert not y[b, n * HOP:].any()


def test_h3_at_the_shipped_wn_size_against_fp64_restatement(shipped):
    y = _infer(shipped, "h3").cpu().double()
    for b, n in enumerate(shipped["lens"]):
        ref = shipped["refs"][b]["exact"]
        diff = y[b, :n * HOP] - ref
        mx, rel = diff.abs().max().item(), (diff.norm() / ref.norm()).item()
        print(f"h3 shipped WN size item {b}: max-abs {mx:.3e} rel-L2 {rel:.3e} (|ref| max {ref.abs().max():.3f})")
        assert mx <= 1e-4 and rel <= 1e-5
        assert not y[b, n * HOP:].any()


def test_h3_batch_invariance(tiny):
    _, cfg, m = tiny["d"], tiny["cfg"], tiny["model"]
    g = torch.Generator().manual_seed(9)
    T, lens = 9, [9, 1, 5, 3, 2]
    per = HOP // cfg["n_group"]
    mel = (torch.randn(len(lens), 8, T, generator=g) - 2.0).to(DEV)
    noise = [torch.randn(len(lens), ch, T * per, generator=g).to(DEV) for ch in noise_channels(cfg)]
    y = m.infer(mel, lens, sigma=0.8, noise=noise, precision="h3")
    worst = 0.0
    for b, n in enumerate(lens):
        alone = m.infer(mel[b:b + 1, :, :n], [n], sigma=0.8, noise=[z[b:b + 1, :, :n * per] for z in noise],
                        precision="h3")[0]
        worst = max(worst, (y[b, :n * HOP] - alone).abs().max().item())
    print(f"h3: batched vs alone max-abs {worst:.3e}")
    assert worst <= 1e-6


@pytest.mark.parametrize("which", ["tiny", "shipped"])
def test_f16_error_is_the_emulations(which, request):
    """per item the rel-L2 error of the HIP output against the exact fp64 restatement lies within a factor 3 of the fp64
    emulation's: above, the mode would be less accurate than its definition; below, it would not be the mode at all
    (the fp32 path sits near 5e-7).  A factor and no tight match: the network amplifies single rounding flips."""
    case = request.getfixturevalue(which)
    y = _infer(case, "f16").cpu().double()
    for b, n in enumerate(case["lens"]):
        ref, emu = case["refs"][b]["exact"], case["refs"][b]["f16"]
        e_emu, e_hip = rel_l2(emu, ref), rel_l2(y[b, :n * HOP], ref)
        alone = _alone(case, b, "f16").cpu().double()
        e_alone = rel_l2(y[b, :n * HOP], alone)
        print(f"f16 {which} item {b}: rel-L2 against exact: HIP {e_hip:.3e}, emulation {e_emu:.3e} (ratio "
              f"{e_hip / e_emu:.2f}); in batch against alone {e_alone:.3e}")
        assert e_emu / 3.0 <= e_hip <= 3.0 * e_emu
        assert e_alone <= 3.0 * e_emu
        assert not y[b, n * HOP:].any()


# ---- 5. properties, both modes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_bits_are_repeatable_and_tails_lengths_and_nan_do_not_matter(tiny, mode):
    m, lens = tiny["model"], tiny["lens"]
    y = _infer(tiny, mode)
    assert torch.equal(_infer(tiny, mode), y)                                  # two identical calls
    assert torch.isfinite(y).all()
    for b, n in enumerate(lens):
        assert not y[b, n * HOP:].any() and y[b, :n * HOP].abs().max() > 0      # samples past each length exactly 0
    dl = torch.tensor(lens, dtype=torch.int32, device=DEV)                     # device lengths
    assert torch.equal(m.infer(tiny["mel"], dl, sigma=tiny["sigma"], noise=tiny["noise"], precision=mode), y)
    mel = tiny["mel"].clone()
    for b, n in enumerate(lens):
        mel[b, :, n:] = float("nan")                                           # NaN in mel past the lengths
    assert torch.equal(m.infer(mel, lens, sigma=tiny["sigma"], noise=tiny["noise"], precision=mode), y)
    m.precision = mode                                                         # the attribute is the default of a call
    try:
        assert torch.equal(m.infer(tiny["mel"], lens, sigma=tiny["sigma"], noise=tiny["noise"]), y)
    finally:
        m.precision = "fp32"
    assert not torch.equal(_infer(tiny, "fp32"), y)                            # and the mode is not the fp32 path


def test_fp32_is_the_default_path(tiny):
    m = tiny["model"]
    assert m.precision == "fp32"
    kw = dict(sigma=tiny["sigma"], noise=tiny["noise"])
    plain = m.infer(tiny["mel"], tiny["lens"], **kw)
    assert torch.equal(m.infer(tiny["mel"], tiny["lens"], precision="fp32", **kw), plain)
    assert torch.equal(m.infer(tiny["mel"], tiny["lens"], precision=None, **kw), plain)


@pytest.mark.parametrize("mode", ("fp32",) + MODES)
def test_infer_event_families(tiny, mode):
    """the per-family device event lists tools/waveglow_bench.py reads, which also witness the launch structure: one
    (start, end) pair per bracketed launch family and flow / layer, counted from the config (one chunk)"""
    m, cfg = tiny["model"], tiny["cfg"]
    F, L = cfg["n_flows"], cfg["WN_config"]["n_layers"]
    B, _, T = tiny["mel"].shape
    events = {}
    m._run(tiny["mel"], torch.tensor(tiny["lens"], dtype=torch.int32, device=DEV), tiny["sigma"], tiny["noise"], events,
           precision=mode)
    assert events.pop("rows") == B * T * HOP // cfg["n_group"]
    want = {"upsample": 1, "start": F, "cond_layer": F, "in_layers": F * L, "gate": F * L, "res_skip_gemm": F * L,
            "res_skip_update": F * L, "end_coupling": F, "ungroup": 1}
    if mode != "fp32":
        want["split_cond"] = 1                          # one split pass over the conditioning rows for all flows
    assert {k: len(v) for k, v in events.items()} == want


def test_split_weights_are_cached_with_the_fold(tiny):
    m = tiny["model"]
    _infer(tiny, "h3")
    f = m._fold()
    sw = f["split"]["h3"]
    _infer(tiny, "h3")
    assert m._fold() is f and f["split"]["h3"] is sw    # split once per fold and mode
    with torch.no_grad():
        m.WN[0].end.bias.add_(0.0)                      # a parameter's version changes: the fold goes, the splits with it
    assert m._fold() is not f and "split" not in m._fold()
    _infer(tiny, "fp32")
    assert "split" not in m._fold()                     # the fp32 path splits no weight


def test_vocode_waveglow_on_an_f16_model():
    from rad_mmm_amd.waveglow import WaveGlowDenoiser, vocode_waveglow
    cfg = dict(TINY, n_flows=4)
    m = _model(cfg, random_state(cfg, 3))
    den = WaveGlowDenoiser(m).to(DEV)
    mels = (torch.randn(3, 8, 7, generator=torch.Generator().manual_seed(5)) - 2.0).to(DEV)
    lens = [7, 3, 5]                                   # the denoiser's reflect pad needs >= 3 frames per item
    torch.manual_seed(21)
    ref, _ = vocode_waveglow(m, den, mels, lens)                                # fp32: also fills the denoiser's bias
    bias = den.bias_spec.clone()
    m.precision = "f16"
    den2 = WaveGlowDenoiser(m).to(DEV)
    torch.manual_seed(21)
    audio, s_lens = vocode_waveglow(m, den2, mels, lens)
    assert torch.equal(den2.bias_spec, bias)            # the bias spectrum comes from the fp32 path in every mode
    assert s_lens.tolist() == [n * HOP for n in lens]
    torch.manual_seed(21)
    assert torch.equal(vocode_waveglow(m, den2, mels, lens, precision="fp32")[0], ref)
    a = audio.cpu()
    assert not torch.equal(a, ref.cpu())
    for b, n in enumerate(lens):
        assert abs(a[b, :n * HOP].abs().max().item() - 1.0) <= 1e-6
        assert not a[b, n * HOP:].any()
