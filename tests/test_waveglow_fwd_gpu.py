"""GPU checks of the WaveGlow forward direction (rad_mmm_amd/waveglow.py analyze / forward / WaveGlowLoss / noise_from_z,
the radmmm_wg_group_audio / wg_mix_fwd / wg_end_coupling_fwd / wg_nll_parts kernels of csrc/waveglow.hip): the
reference's recorded forward pass (tests/golden/waveglow_fwd_tiny.npz), the round trip through infer, ragged batches,
the new kernels directly against float64, one case at the shipped WN size against the float64 restatement, and the
absence of device -> host synchronisation with host lengths."""
import math

import numpy as np
import pytest
import torch

from conftest import rel_err
from _waveglow_fwd_ref import forward_ref, nll_ref
from _waveglow_ref import HOP, SHIPPED_WN, load_fixture, random_state

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _model(cfg, sd):
    from rad_mmm_amd.waveglow import WaveGlow
    m = WaveGlow(**cfg)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def tiny(golden):
    """the fixture, its model, and the float64 restatement's terms: per item alone, and for the equal-length batch"""
    d = golden("waveglow_fwd_tiny.npz")
    cfg, sd = load_fixture(d)
    mel, audio = torch.from_numpy(d["mel"]), torch.from_numpy(d["audio"])
    ref_nll = []
    for b, n in enumerate(d["lens"].tolist()):
        ref_nll.append(float(nll_ref(*forward_ref(sd, cfg, mel[b:b + 1, :, :n], audio[b:b + 1, :n * HOP]))))
    n = int(d["eq_T"])
    terms = [forward_ref(sd, cfg, mel[b:b + 1, :, :n], audio[b:b + 1, :n * HOP]) for b in range(2)]
    ref_eq = float(nll_ref(torch.cat([t[0] for t in terms], 0), [x for t in terms for x in t[1]], terms[0][2]))
    return d, cfg, _model(cfg, sd), ref_nll, ref_eq


RAGGED = [9, 1, 5, 3, 2]


@pytest.fixture(scope="module")
def ragged(tiny):
    """random audio (whatever lies past an item's length included) on the fixture model, analysed once"""
    _, cfg, m, _, _ = tiny
    g = torch.Generator().manual_seed(19)
    T = max(RAGGED)
    mel = (torch.randn(len(RAGGED), 8, T, generator=g) - 2.0).to(DEV)
    audio = (0.3 * torch.randn(len(RAGGED), T * HOP, generator=g)).to(DEV)
    return mel, audio, m.analyze(mel, audio, RAGGED)


def test_analyze_matches_reference_fixture(tiny):
    d, cfg, m, ref_nll, ref_eq = tiny
    lens = d["lens"].tolist()
    per = HOP // cfg["n_group"]
    mel, audio = torch.from_numpy(d["mel"]).to(DEV), torch.from_numpy(d["audio"]).to(DEV)
    out = m.analyze(mel, audio, lens)
    z = out["z"].cpu().numpy()
    assert z.shape == d["z"].shape and out["n_groups"].tolist() == [n * per for n in lens]
    bar = max(10 * float(d["f32_vs_f64_loss"]), 1e-6)
    for b, n in enumerate(lens):
        ref = d["z"][b, :, :n * per]
        err = np.abs(z[b, :, :n * per] - ref).max()
        enll = abs(float(out["nll"][b]) - ref_nll[b])
        print(f"item {b} ({n} frames): z max-abs {err:.3e} (|ref| max {np.abs(ref).max():.3f}), nll "
              f"{float(out['nll'][b]):.7f}, {enll:.3e} from the restatement (bar {bar:.3e})")
        assert err <= 1e-4 * max(1.0, np.abs(ref).max())
        assert enll <= bar
        assert not z[b, :, n * per:].any()
    eld = np.abs(out["log_det_W"].cpu().numpy() - d["logdet"]).max()
    print(f"log_det_W: {eld:.3e} from the reference's float32 logdet")
    assert eld <= 1e-6
    n = int(d["eq_T"])
    eq = m.analyze(mel[:, :, :n].contiguous(), audio[:, :n * HOP].contiguous())
    el = abs(float(eq["loss"]) - ref_eq)
    print(f"equal-length batch: loss {float(eq['loss']):.7f}, {el:.3e} from the restatement (bar {bar:.3e})")
    assert el <= bar


def test_forward_and_loss_have_the_reference_shapes(tiny):
    from rad_mmm_amd.waveglow import WaveGlowLoss
    d, cfg, m, _, ref_eq = tiny
    n = int(d["eq_T"])
    Tg = n * HOP // cfg["n_group"]
    mel = torch.from_numpy(d["mel"][:, :, :n].copy()).to(DEV)
    audio = torch.from_numpy(d["audio"][:, :n * HOP].copy()).to(DEV)
    z, log_s_list, log_det_W_list = m((mel, audio))
    assert tuple(z.shape) == (2, cfg["n_group"], Tg)
    assert [tuple(t.shape) for t in log_s_list] == [(2, c, Tg) for c in (4, 4, 3, 3, 2, 2)]
    assert len(log_det_W_list) == cfg["n_flows"] and all(t.dim() == 0 for t in log_det_W_list)
    want = 2 * Tg * d["logdet"]
    assert np.abs(np.array([float(t) for t in log_det_W_list]) - want).max() <= 1e-6 * 2 * Tg
    assert torch.equal(z, m.analyze(mel, audio)["z"])
    loss = float(WaveGlowLoss(1.0)((z, log_s_list, log_det_W_list)))
    bar = max(10 * float(d["f32_vs_f64_loss"]), 1e-6)
    print(f"WaveGlowLoss {loss:.7f}: {abs(loss - float(d['eq_loss'])):.3e} from the reference, "
          f"{abs(loss - ref_eq):.3e} from the restatement (bar {bar:.3e})")
    assert abs(loss - float(d["eq_loss"])) <= bar and abs(loss - ref_eq) <= bar


def test_infer_inverts_analyze(tiny, ragged):
    # bar: 4 x the reference's own float32 round trip: two float32 implementations with different summation orders,
    # each allowed the reference's own error twice
    d, cfg, m, _, _ = tiny
    mel, audio, out = ragged
    per = HOP // cfg["n_group"]
    back = m.infer(mel, RAGGED, sigma=1.0, noise=m.noise_from_z(out["z"]))
    worst, peak = 0.0, 0.0
    for b, n in enumerate(RAGGED):
        worst = max(worst, (back[b, :n * HOP] - audio[b, :n * HOP]).abs().max().item())
        peak = max(peak, audio[b, :n * HOP].abs().max().item())
        assert not back[b, n * HOP:].any() and not out["z"][b, :, n * per:].any()
    bar = 4 * float(d["roundtrip_f32"]) * max(1.0, peak)
    print(f"round trip infer(noise_from_z(analyze(audio))) - audio: max-abs {worst:.3e} at |audio| max {peak:.3f} "
          f"(bar {bar:.3e}, the reference's own float32 round trip {float(d['roundtrip_f32']):.3e})")
    assert worst <= bar


def test_ragged_batches(tiny, ragged):
    _, cfg, m, _, _ = tiny
    mel, audio, out = ragged
    per = HOP // cfg["n_group"]
    wz = wn = 0.0
    for b, n in enumerate(RAGGED):
        alone = m.analyze(mel[b:b + 1, :, :n].contiguous(), audio[b:b + 1, :n * HOP].contiguous(), [n])
        wz = max(wz, (out["z"][b, :, :n * per] - alone["z"][0]).abs().max().item())
        wn = max(wn, abs(float(out["nll"][b]) - float(alone["nll"][0])))
    print(f"waveglow forward: batched vs alone z max-abs {wz:.3e}, nll {wn:.3e}")
    assert wz <= 1e-6 and wn <= 1e-6
    keys = ("z", "log_s_sum", "nll", "loss", "n_groups")
    again = m.analyze(mel, audio, RAGGED)                                     # two runs: the same bits
    assert all(torch.equal(out[k], again[k]) for k in keys)
    dl = torch.tensor(RAGGED, dtype=torch.int32, device=DEV)                  # device lengths: the same bits
    dev = m.analyze(mel, audio, dl)
    assert all(torch.equal(out[k], dev[k]) for k in keys)
    poisoned = audio.clone()
    for b, n in enumerate(RAGGED):
        poisoned[b, n * HOP:] = float("nan")
    nan = m.analyze(mel, poisoned, RAGGED)                                    # what lies past a length reaches nothing
    assert all(torch.equal(out[k], nan[k]) for k in keys)
    assert torch.isfinite(out["nll"]).all() and torch.isfinite(out["loss"])


# ---- the new kernels of csrc/waveglow.hip directly, against float64 -------------------------------------------------
# Bars: 1e-6 * max|ref| (conftest.rel_err), the convention of the direct tests of the fp32 kernels of the other direction
# (tests/test_waveglow_gpu.py; sums of at most C = 32 products here, of 72 there).

def _lib():
    from rad_mmm_amd._lib import check, lib, ptr, stream
    return check, lib, ptr, stream()


def _rows_mask(lens, T):
    return (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).reshape(-1)


LENS, TG = [37, 32, 1, 300], 300        # group steps: 1200 rows = 75 passes of 16 rows and 4.7 blocks of 256 rows


@pytest.mark.parametrize("c,ldx", [(4, 8), (6, 8), (8, 8), (8, 9)])       # 16-, 8-, 16- and 4-byte accesses of the mix
def test_mix_and_forward_coupling_kernels(c, ldx):
    check, lib, ptr, s = _lib()
    g = torch.Generator().manual_seed(20 + c + ldx)
    C, nh = 32, c // 2
    col0 = ldx - c
    R = len(LENS) * TG
    mask = _rows_mask(LENS, TG)
    lens = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    W = (torch.linalg.qr(torch.randn(c, c, generator=g))[0] + 0.1 * torch.randn(c, c, generator=g)).contiguous()
    X0 = torch.randn(R, ldx, generator=g)
    X0[~mask] = float("nan")                           # rows past a length are written, never read
    X = X0.clone().to(DEV)
    Wd = W.to(DEV)
    check(lib.radmmm_wg_mix_fwd(ptr(X), ldx, col0, c, ptr(Wd), ptr(lens), R, TG, s), "wg_mix_fwd")
    mixed = (torch.nan_to_num(X0[:, col0:]).double() @ W.double().T) * mask[:, None]
    got = X.cpu()
    err = rel_err(got[:, col0:].numpy(), mixed.numpy())
    print(f"mix, c = {c}, ldx = {ldx}: rel {err:.3e}")
    assert err <= 1e-6
    assert torch.equal(got[:, :col0][mask], X0[:, :col0][mask])     # the columns in front are not touched
    assert not got[~mask][:, col0:].any()

    Xm = got.clone()                                   # the coupling is checked on the mix's own float32 output
    Xm[~mask] = 0.0
    ls = torch.full((R,), float("nan"), device=DEV)    # first = 1 must not read it
    ls_ref = torch.zeros(R, dtype=torch.float64)
    x_ref = Xm[:, col0:].double()
    Xd = Xm.clone().to(DEV)
    for call, first in enumerate((1, 0)):
        S = torch.randn(R, C, generator=g)
        We, be = 0.05 * torch.randn(c, C, generator=g), 0.05 * torch.randn(c, generator=g)
        logs = torch.full((R, nh), 7.0, device=DEV) if call == 0 else None     # with and without the log_s output
        Sd, Wed, bed = S.to(DEV), We.to(DEV), be.to(DEV)
        check(lib.radmmm_wg_end_coupling_fwd(ptr(Sd), C, ptr(Wed), ptr(bed), ptr(Xd), ldx, col0, nh, C, ptr(ls), first,
                                             ptr(logs), ptr(lens), R, TG, s), "wg_end_coupling_fwd")
        o = (S.double() @ We.double().T + be.double()) * mask[:, None]
        x_ref = torch.cat([x_ref[:, :nh], (torch.exp(o[:, nh:]) * x_ref[:, nh:] + o[:, :nh]) * mask[:, None]], 1)
        ls_ref = ls_ref + o[:, nh:].sum(1)
        if logs is not None:
            el = rel_err(logs.cpu().numpy(), o[:, nh:].numpy())
            print(f"  log_s output: rel {el:.3e}")
            assert el <= 1e-6 and not logs.cpu()[~mask].any()
        ex, es = rel_err(Xd.cpu()[:, col0:].numpy(), x_ref.numpy()), rel_err(ls.cpu().numpy(), ls_ref.numpy())
        print(f"  coupling call {call} (first = {first}): X rel {ex:.3e}, ls rel {es:.3e}")
        assert ex <= 1e-6 and es <= 1e-6
    got = Xd.cpu()
    assert torch.equal(got[:, :col0 + nh], Xm[:, :col0 + nh])       # X0 and the columns in front: not touched
    assert not got[~mask][:, col0 + nh:].any() and not ls.cpu()[~mask].any()


@pytest.mark.parametrize("ng,ldx,pad", [(8, 8, 8), (6, 7, 3)])             # 16-byte accesses; the scalar path
def test_group_audio_then_ungroup_is_the_identity(ng, ldx, pad):
    check, lib, ptr, s = _lib()
    g = torch.Generator().manual_seed(5)
    B = len(LENS)
    lda = TG * ng + pad
    audio = torch.randn(B, lda, generator=g)
    valid = (torch.arange(lda)[None, :] < (torch.tensor(LENS) * ng)[:, None])
    audio[~valid] = float("nan")                        # past each length and in the padding: never read
    lens = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    X = torch.full((B * TG, ldx), 7.0, device=DEV)
    ad = audio.to(DEV)
    check(lib.radmmm_wg_group_audio(ptr(ad), lda, ptr(X), ldx, ng, ptr(lens), B, TG, s), "wg_group_audio")
    want = torch.nan_to_num(audio[:, :TG * ng]).reshape(B * TG, ng)
    got = X.cpu()
    assert torch.equal(got[:, :ng], want) and bool((got[:, ng:] == 7.0).all())
    back = torch.full((B, lda), 7.0, device=DEV)
    check(lib.radmmm_wg_ungroup(ptr(X), ldx, 0, ng, ptr(back), lda, ptr(lens), B, TG, s), "wg_ungroup")
    back = back.cpu()
    assert torch.equal(back[valid], audio[valid]) and not back[:, :TG * ng][~valid[:, :TG * ng]].any()


@pytest.mark.parametrize("ng,ldx", [(8, 8), (6, 7)])
def test_nll_parts_kernel_against_fsum(ng, ldx):
    # item 0 has length 0 (every row lies past it), item 1 has 3001 rows: more than one row per thread and every wave of
    # the workgroup in play.  Bar: the worst case of a float64 sum of n terms, n * 2^-53 * sum|term| (the squares of
    # float32 values are exact in float64).
    check, lib, ptr, s = _lib()
    g = torch.Generator().manual_seed(6)
    lens_h, Tg = [0, 3001, 5], 3001
    B = len(lens_h)
    mask = _rows_mask(lens_h, Tg)
    X = torch.randn(B * Tg, ldx, generator=g)
    ls = torch.randn(B * Tg, generator=g)
    X[~mask] = float("nan")
    ls[~mask] = float("nan")
    X[:, ng:] = float("nan")                            # the columns past n_group are not part of z
    lens = torch.tensor(lens_h, dtype=torch.int32, device=DEV)
    parts = torch.full((B, 2), 7.0, dtype=torch.float64, device=DEV)
    Xd, lsd = X.to(DEV), ls.to(DEV)
    check(lib.radmmm_wg_nll_parts(ptr(Xd), ldx, ng, ptr(lsd), ptr(lens), B, Tg, ptr(parts), s), "wg_nll_parts")
    again = torch.full((B, 2), 7.0, dtype=torch.float64, device=DEV)
    check(lib.radmmm_wg_nll_parts(ptr(Xd), ldx, ng, ptr(lsd), ptr(lens), B, Tg, ptr(again), s), "wg_nll_parts")
    assert torch.equal(parts, again)
    parts = parts.cpu()
    for b, n in enumerate(lens_h):
        xs = [float(v) ** 2 for v in X[b * Tg:b * Tg + n, :ng].reshape(-1).tolist()]
        lt = [float(v) for v in ls[b * Tg:b * Tg + n].tolist()]
        wq, wl = math.fsum(xs), math.fsum(lt)
        bq, bl = len(xs) * 2.0 ** -53 * wq, len(lt) * 2.0 ** -53 * math.fsum(abs(v) for v in lt)
        eq, el = abs(float(parts[b, 0]) - wq), abs(float(parts[b, 1]) - wl)
        print(f"item {b} ({n} rows): sum z^2 {wq:.6f} off by {eq:.3e} (bar {bq:.3e}), sum ls {wl:.6f} off by {el:.3e} "
              f"(bar {bl:.3e})")
        assert eq <= bq and el <= bl
    assert parts[0].tolist() == [0.0, 0.0]


def test_shipped_wn_size_against_fp64_restatement():
    # n_channels 256, n_layers 8: dilation 128 and K = 768; one item of 2 frames = 64 group steps, fewer than the
    # largest dilation.  The bar of the same case in the other direction (tests/test_waveglow_gpu.py).
    cfg = dict(n_mel_channels=80, n_flows=2, n_group=8, n_early_every=4, n_early_size=2, WN_config=SHIPPED_WN)
    sd = random_state(cfg, 7)
    m = _model(cfg, sd)
    g = torch.Generator().manual_seed(8)
    T = 2
    mel = torch.randn(1, 80, T, generator=g) - 2.0
    audio = 0.3 * torch.randn(1, T * HOP, generator=g)
    out = m.analyze(mel.to(DEV), audio.to(DEV), [T])
    z = out["z"].cpu().double()
    ref, ls, ld = forward_ref(sd, cfg, mel, audio)
    diff = z - ref
    mx, rel = diff.abs().max().item(), (diff.norm() / ref.norm()).item()
    print(f"shipped WN size: z max-abs {mx:.3e} rel-L2 {rel:.3e} (|ref| max {ref.abs().max():.3f}); nll "
          f"{float(out['nll'][0]):.7f} against {float(nll_ref(ref, ls, ld)):.7f}")
    assert mx <= 1e-4 and rel <= 1e-5


def test_no_device_to_host_sync_with_host_lengths(tiny):
    d, cfg, m, _, _ = tiny
    mel, audio = torch.from_numpy(d["mel"]).to(DEV), torch.from_numpy(d["audio"]).to(DEV)
    m.analyze(mel, audio, [7, 4])                            # warm: weights folded
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = m.analyze(mel, audio, [7, 3])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert all(v.is_cuda for v in out.values())
    assert out["n_groups"].tolist() == [7 * 32, 3 * 32] and torch.isfinite(out["nll"]).all()
