"""GPU checks of the batched WaveGlow vocoder (rad_mmm_amd/waveglow.py, csrc/waveglow.hip): infer and the denoiser
against the reference's recorded outputs (tests/golden/waveglow_*.npz), batch invariance, the new kernels directly against
float64, one case at the shipped WN size against the fp64 restatement, the absence of device -> host synchronisation
with host lengths, and TTSTrainingStep.vocode_mels with a WaveGlow pair."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from _waveglow_ref import (HOP, SHIPPED_WN, TINY, group_cond_ref, infer_ref, load_fixture, noise_channels, random_state)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _model(cfg, sd):
    from rad_mmm_amd.waveglow import WaveGlow
    m = WaveGlow(**cfg)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def tiny(golden):
    d = golden("waveglow_tiny.npz")
    cfg, sd = load_fixture(d)
    noise = [torch.from_numpy(d[f"noise{i}"]).to(DEV) for i in range(3)]
    return d, cfg, _model(cfg, sd), noise


def test_infer_matches_reference_fixture(tiny):
    d, cfg, m, noise = tiny
    lens = d["lens"].tolist()
    y = m.infer(torch.from_numpy(d["mel"]).to(DEV), lens, sigma=float(d["sigma"]), noise=noise).cpu().numpy()
    assert y.shape == d["audio"].shape
    for b, n in enumerate(lens):
        ref = d["audio"][b, :n * HOP]
        err = np.abs(y[b, :n * HOP] - ref).max()
        print(f"item {b} ({n} frames): max-abs {err:.3e} (|ref| max {np.abs(ref).max():.3f})")
        assert err <= 1e-4 * max(1.0, np.abs(ref).max())
        assert not y[b, n * HOP:].any()


def test_batch_invariance_and_zero_tails(tiny):
    _, cfg, m, _ = tiny
    g = torch.Generator().manual_seed(9)
    T = 9
    lens = [T, 1, 5, 3, 2]
    per = HOP // cfg["n_group"]
    mel = (torch.randn(len(lens), 8, T, generator=g) - 2.0).to(DEV)
    noise = [torch.randn(len(lens), ch, T * per, generator=g).to(DEV) for ch in noise_channels(cfg)]
    y = m.infer(mel, lens, sigma=0.8, noise=noise)
    dl = torch.tensor(lens, dtype=torch.int32, device=DEV)              # device lengths: the same result
    assert torch.equal(m.infer(mel, dl, sigma=0.8, noise=noise), y)
    worst = 0.0
    for b, n in enumerate(lens):
        alone = m.infer(mel[b:b + 1, :, :n], [n], sigma=0.8, noise=[z[b:b + 1, :, :n * per] for z in noise])[0]
        worst = max(worst, (y[b, :n * HOP] - alone).abs().max().item())
        assert not y[b, n * HOP:].any()
    print(f"waveglow: batched vs alone max-abs {worst:.3e}")
    assert worst <= 1e-6
    drawn = m.infer(mel, lens, sigma=0.8)                               # noise drawn on the device
    assert torch.isfinite(drawn).all() and not drawn[1, HOP:].any() and drawn[1, :HOP].abs().max() > 0


def test_denoiser_matches_reference_fixture(golden):
    from rad_mmm_amd.waveglow import WaveGlowDenoiser
    d = golden("waveglow_denoiser.npz")
    cfg, sd = load_fixture(d)
    den = WaveGlowDenoiser(_model(cfg, sd)).to(DEV)
    lens = d["lens"].tolist()
    audio = torch.from_numpy(d["audio"]).to(DEV)
    for tag, strength in (("s0p1", 0.1), ("s0p001", 0.001)):
        y = den(audio, strength, lens)[:, 0].cpu().numpy()
        if tag == "s0p1":
            berr = rel_err(den.bias_spec.cpu().numpy(), d["bias_spec"])
            print(f"bias_spec rel max {berr:.3e}")
            assert berr <= 1e-5
        for b, n in enumerate(lens):
            mm = n // HOP * HOP
            ref = d["out_" + tag][b, :mm]
            err = np.abs(y[b, :mm] - ref).max()
            print(f"denoiser {tag} item {b}: max-abs {err:.3e} (|ref| max {np.abs(ref).max():.3f})")
            assert err <= 1e-4 * max(1.0, np.abs(ref).max())
            assert not y[b, mm:].any()
    with pytest.raises(ValueError):
        WaveGlowDenoiser(den.generator, mode="normal")


# ---- the kernels of csrc/waveglow.hip directly, against float64 ---------------------------------------------------
# Bars: 1e-6 * max|ref| (conftest.rel_err), the convention of the direct tests of fp32 elementwise kernels here.

def _lib():
    from rad_mmm_amd._lib import check, lib, ptr, stream
    return check, lib, ptr, stream()


def _rows_mask(lens, T):
    return (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).reshape(-1)


LENS, TG = [37, 32, 1, 5], 37           # group steps; 32 = one frame, 5 < the largest dilation of any WN here


def test_gate_kernel_on_a_conditioning_slice():
    check, lib, ptr, s = _lib()
    g = torch.Generator().manual_seed(1)
    C, L, i = 12, 3, 2                                  # slice offset 2*C*i = 48 of 72 conditioning columns
    R = len(LENS) * TG
    a = 2.0 * torch.randn(R, 2 * C, generator=g)
    cond = 2.0 * torch.randn(R, 2 * C * L, generator=g)
    lens = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    y = torch.full((R, C), 7.0, device=DEV)
    ad, cd = a.to(DEV), cond.to(DEV)
    check(lib.radmmm_wg_gate(ptr(ad), 2 * C, ptr(cd), 2 * C * L, 2 * C * i, ptr(y), C, C, ptr(lens), R, TG, s), "wg_gate")
    x = a.double() + cond[:, 2 * C * i:2 * C * (i + 1)].double()
    ref = torch.tanh(x[:, :C]) * torch.sigmoid(x[:, C:]) * _rows_mask(LENS, TG)[:, None]
    err = rel_err(y.cpu().numpy(), ref.numpy())
    print(f"gate: rel {err:.3e}")
    assert err <= 1e-6
    assert not y.cpu()[~_rows_mask(LENS, TG)].any()


@pytest.mark.parametrize("c", [4, 6, 8])
def test_end_coupling_inverse_mix_kernel(c):
    check, lib, ptr, s = _lib()
    g = torch.Generator().manual_seed(10 + c)
    C, ng, nh = 72, 8, c // 2                           # C = 72: a column tail past the 64 of one pass
    col0 = ng - c
    R = len(LENS) * TG
    S = torch.randn(R, C, generator=g)
    We, be = 0.05 * torch.randn(c, C, generator=g), 0.05 * torch.randn(c, generator=g)
    W = torch.linalg.qr(torch.randn(c, c, generator=g))[0] + 0.1 * torch.randn(c, c, generator=g)
    Winv = torch.linalg.inv(W.double()).float().contiguous()       # linalg.inv may return column-major strides
    X0 = torch.randn(R, ng, generator=g)
    X = X0.clone().to(DEV)
    lens = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    Sd, Wd, bd, Wid = S.to(DEV), We.to(DEV), be.to(DEV), Winv.to(DEV)
    check(lib.radmmm_wg_end_coupling(ptr(Sd), C, ptr(Wd), ptr(bd), ptr(Wid), ptr(X), ng, col0, nh, C, ptr(lens), R, TG,
                                     s), "wg_end_coupling")
    o = S.double() @ We.double().T + be.double()
    x = X0[:, col0:].double()
    z = torch.cat([x[:, :nh], (x[:, nh:] - o[:, :nh]) * torch.exp(-o[:, nh:])], 1)
    ref = (z @ Winv.double().T) * _rows_mask(LENS, TG)[:, None]
    got = X.cpu()
    err = rel_err(got[:, col0:].numpy(), ref.numpy())
    print(f"end + coupling + mix, c = {c}: rel {err:.3e}")
    assert err <= 1e-6
    assert torch.equal(got[:, :col0], X0[:, :col0])     # the columns in front of the live channels are not touched
    assert not got[~_rows_mask(LENS, TG)][:, col0:].any()


def test_group_and_ungroup_kernels_with_ragged_lengths():
    check, lib, ptr, s = _lib()
    g = torch.Generator().manual_seed(3)
    n_mel, ng, B = 5, 8, len(LENS)
    tail = 3 * ng * n_mel                               # a longer source item: what the trim leaves unread
    stride = TG * ng * n_mel + tail
    up = torch.randn(B, stride, generator=g)
    ldr = 44                                            # n_mel * ng = 40 columns + 4 of padding
    lens = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    rows = torch.full((B * TG, ldr), 7.0, device=DEV)
    upd = up.to(DEV)
    check(lib.radmmm_wg_group_cond(ptr(upd), stride, ptr(rows), ldr, ptr(lens), B, TG, n_mel, ng, s), "group")
    src = up[:, :TG * ng * n_mel].reshape(B, TG * ng, n_mel).permute(0, 2, 1)          # [B, n_mel, samples]
    ref = src.unfold(2, ng, ng).permute(0, 2, 1, 3).contiguous().view(B, TG, -1)      # glow.py:257-258, rows [B, Tg, C]
    mask = _rows_mask(LENS, TG)
    ref = ref.reshape(B * TG, -1) * mask[:, None]
    got = rows.cpu()
    assert torch.equal(got[:, :n_mel * ng], ref) and not got[:, n_mel * ng:].any()

    for c, ch in ((4, 4), (6, 2)):                      # the initial draw, then an early re-attachment in front of it
        z = torch.randn(B, ch, TG, generator=g)
        X = torch.full((B * TG, ng), 7.0, device=DEV)
        col0 = ng - c
        zd = z.to(DEV)
        check(lib.radmmm_wg_noise_rows(ptr(zd), 0.8, ptr(X), ng, col0, ch, ptr(lens), B, TG, s), "noise")
        want = torch.full((B * TG, ng), 7.0)
        want[:, col0:col0 + ch] = (torch.tensor(0.8) * z).permute(0, 2, 1).reshape(B * TG, ch) * mask[:, None]
        assert torch.equal(X.cpu(), want)

    X = torch.randn(B * TG, ng, generator=g)
    lda = TG * ng + 8
    audio = torch.full((B, lda), 7.0, device=DEV)
    Xd = X.to(DEV)
    check(lib.radmmm_wg_ungroup(ptr(Xd), ng, 0, ng, ptr(audio), lda, ptr(lens), B, TG, s), "ungroup")
    want = (X * mask[:, None]).reshape(B, TG * ng)
    assert torch.equal(audio.cpu()[:, :TG * ng], want) and bool((audio.cpu()[:, TG * ng:] == 7.0).all())


def test_start_and_res_skip_kernels():
    check, lib, ptr, s = _lib()
    g = torch.Generator().manual_seed(4)
    C, ng, R = 12, 8, len(LENS) * TG
    lens = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    mask = _rows_mask(LENS, TG)[:, None]
    X = torch.randn(R, ng, generator=g)
    Xd = X.to(DEV)
    for nh in (2, 3, 4):
        col0 = ng - 2 * nh
        W, b = torch.randn(C, nh, generator=g), torch.randn(C, generator=g)
        H = torch.full((R, C), 7.0, device=DEV)
        Wd, bd = W.to(DEV), b.to(DEV)
        check(lib.radmmm_wg_start(ptr(Xd), ng, col0, nh, ptr(Wd), ptr(bd), ptr(H), C, C, ptr(lens), R, TG, s), "wg_start")
        ref = (X[:, col0:col0 + nh].double() @ W.double().T + b.double()) * mask
        err = rel_err(H.cpu().numpy(), ref.numpy())
        print(f"start, n_half = {nh}: rel {err:.3e}")
        assert err <= 1e-6
    rs, H0, S0 = (torch.randn(R, n, generator=g) for n in (2 * C, C, C))
    rsd = rs.to(DEV)
    for first, last in ((1, 0), (0, 0), (0, 1), (1, 1)):
        H, S = H0.clone().to(DEV), S0.clone().to(DEV)
        check(lib.radmmm_wg_res_skip(ptr(rsd), 2 * C, ptr(H), C, ptr(S), C, C, first, last, ptr(lens), R, TG, s),
              "wg_res_skip")
        base = torch.zeros_like(S0) if first else S0
        if last:
            assert torch.equal(H.cpu(), H0) and torch.equal(S.cpu(), (base + rs[:, :C]) * mask)
        else:
            assert torch.equal(H.cpu(), (H0 + rs[:, :C]) * mask) and torch.equal(S.cpu(), (base + rs[:, C:]) * mask)


def test_grouped_conditioning_of_a_ragged_batch(tiny):
    # upsample GEMM + grouping against conv_transpose1d + unfold of each item alone (fp64), zeros past each length
    d, cfg, m, _ = tiny
    _, sd = load_fixture(d)
    from rad_mmm_amd._lib import check, lib, ptr, rowgemm, stream
    mel = torch.from_numpy(d["mel"])
    B, n_mel, T = mel.shape
    lens, ng = d["lens"].tolist(), cfg["n_group"]
    per = HOP // ng
    f = m._fold()
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    xm = torch.empty(B * T, n_mel, device=DEV)
    meld = mel.to(DEV)
    check(lib.radmmm_squeeze_rows(ptr(meld), ptr(xm), B, n_mel, T, 1, n_mel, 0, stream()), "squeeze_rows")
    Wp, bp = f["up"]
    up = torch.empty(B * T, HOP * n_mel, device=DEV)
    rowgemm(A=xm, lda=n_mel, B=Wp, ldb=Wp.shape[2], b_tap_stride=Wp.stride(0), C=up, ldc=HOP * n_mel, M=B * T,
            N=HOP * n_mel, K=n_mel, taps=Wp.shape[0], dil=1, T=T, lens=lens_d, a_mask_mode=1, bias=bp, postmask=1)
    rows = torch.empty(B * T * per, n_mel * ng, device=DEV)
    lens_g = lens_d * per
    check(lib.radmmm_wg_group_cond(ptr(up), T * HOP * n_mel, ptr(rows), n_mel * ng, ptr(lens_g), B, T * per, n_mel, ng,
                                   stream()), "wg_group_cond")
    rows = rows.cpu().reshape(B, T * per, -1)
    folded = {k: v.cpu() for k, v in m.state_dict().items()}
    for b, n in enumerate(lens):
        ref = group_cond_ref(folded, cfg, mel[b:b + 1, :, :n])[0].T
        err = rel_err(rows[b, :n * per].numpy(), ref.numpy())
        print(f"conditioning item {b}: rel {err:.3e}")
        assert err <= 1e-5                  # a K = 4 * n_mel fp32 MFMA sum, not an elementwise kernel
        assert not rows[b, n * per:].any()


def test_shipped_wn_size_against_fp64_restatement():
    # n_channels 256, n_layers 8: dilation 128 and K = 768; item 1 has 96 group steps, fewer than the largest dilation
    cfg = dict(n_mel_channels=80, n_flows=2, n_group=8, n_early_every=4, n_early_size=2, WN_config=SHIPPED_WN)
    sd = random_state(cfg, 7)
    m = _model(cfg, sd)
    g = torch.Generator().manual_seed(8)
    B, T, lens = 2, 12, [12, 3]
    per = HOP // 8
    mel = torch.randn(B, 80, T, generator=g) - 2.0
    noise = [torch.randn(B, 8, T * per, generator=g)]
    y = m.infer(mel.to(DEV), lens, sigma=0.9, noise=[z.to(DEV) for z in noise]).cpu().double()
    for b, n in enumerate(lens):
        ref = infer_ref(sd, cfg, mel[b:b + 1, :, :n], 0.9, [z[b:b + 1, :, :n * per] for z in noise])[0]
        diff = y[b, :n * HOP] - ref
        mx, rel = diff.abs().max().item(), (diff.norm() / ref.norm()).item()
        print(f"shipped WN size item {b}: max-abs {mx:.3e} rel-L2 {rel:.3e} (|ref| max {ref.abs().max():.3f})")
        assert mx <= 1e-4 and rel <= 1e-5
        assert not y[b, n * HOP:].any()


def test_no_device_to_host_sync_with_host_lengths(golden):
    from rad_mmm_amd.waveglow import WaveGlowDenoiser, vocode_waveglow
    cfg, sd = load_fixture(golden("waveglow_denoiser.npz"))
    m = _model(cfg, sd)
    den = WaveGlowDenoiser(m).to(DEV)
    mels = (torch.randn(2, 80, 10) - 2.0).to(DEV)
    vocode_waveglow(m, den, mels, [10, 8])                   # warm: weights folded, bias spectrum computed
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        audio, s_lens = vocode_waveglow(m, den, mels, [10, 6])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert s_lens.tolist() == [10 * HOP, 6 * HOP] and not s_lens.is_cuda
    a = audio.cpu()
    assert not a[1, 6 * HOP:].any()
    assert abs(a[1, :6 * HOP].abs().max().item() - 1.0) < 1e-6


def test_vocode_mels_dispatches_on_a_waveglow_pair(golden):
    from rad_mmm_amd.common import SequenceLength
    from rad_mmm_amd.tts_step import TTSTrainingStep
    from rad_mmm_amd.waveglow import WaveGlowDenoiser, vocode_waveglow
    cfg, sd = load_fixture(golden("waveglow_denoiser.npz"))
    m = _model(cfg, sd)
    den = WaveGlowDenoiser(m).to(DEV)
    step = TTSTrainingStep.__new__(TTSTrainingStep)          # vocode_mels uses nothing of the training modules
    torch.nn.Module.__init__(step)
    step.synth_vocoder = (m, den)
    lens = torch.tensor([6, 3, 9])
    mels = (torch.randn(3, 80, 9) - 2.0).to(DEV)
    torch.manual_seed(77)
    out = step.vocode_mels(mels, SequenceLength(lens.to(DEV), lens))
    torch.manual_seed(77)
    audio, s_lens = vocode_waveglow(m, den, mels, lens.tolist())
    assert s_lens.tolist() == (lens * HOP).tolist()
    audio = audio.cpu().numpy()
    for b, (a, n) in enumerate(zip(out, lens.tolist())):
        assert a.shape == (n * HOP,) and a.dtype == np.float32
        assert np.array_equal(a, audio[b, :n * HOP])
        assert abs(np.abs(a).max() - 1.0) < 1e-6
