"""CPU checks of the WaveGlow forward direction (audio -> latent): the float64 restatement (tests/_waveglow_fwd_ref.py)
replays the reference's recorded forward pass and losses (tests/golden/waveglow_fwd_tiny.npz), inverts exactly through
the restatement of infer, and the new entry points validate their arguments before any HIP call."""
import ctypes
import os

import numpy as np
import torch

from _waveglow_fwd_ref import forward_ref, nll_ref, noise_from_z_ref
from _waveglow_ref import HOP, TINY, infer_ref, load_fixture

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rad_mmm_amd", "libradmmm_hip.so")


def test_fp64_restatement_replays_the_forward_fixture(golden):
    # The fixture is the reference in float32, the restatement float64: the fixture's own rounding is the whole
    # difference, hence 10 x the reference's float32-against-float64 deviation as the bar.
    d = golden("waveglow_fwd_tiny.npz")
    cfg, sd = load_fixture(d)
    assert cfg == TINY and d["lens"].tolist() == [7, 4]
    assert np.abs(d["audio"]).max() < 1 and np.abs(d["logdet"]).min() > 0.05
    bar_z, bar_l = 10 * float(d["f32_vs_f64_z"]), 10 * float(d["f32_vs_f64_loss"])
    mel, audio = torch.from_numpy(d["mel"]), torch.from_numpy(d["audio"])
    per = HOP // cfg["n_group"]
    for b, n in enumerate(d["lens"].tolist()):
        z, ls, ld = forward_ref(sd, cfg, mel[b:b + 1, :, :n], audio[b:b + 1, :n * HOP])
        ez = np.abs(z[0].numpy() - d["z"][b, :, :n * per]).max()
        els = np.abs(np.array([float(x) for x in ls]) - d["log_s_sums"][b]).max()
        eld = np.abs(np.array([float(x) for x in ld]) - d["logdet"]).max()
        el = abs(float(nll_ref(z, ls, ld)) - float(d["loss_item"][b]))
        print(f"item {b}: z {ez:.3e} (bar {bar_z:.3e}), sums of log_s {els:.3e}, logdet {eld:.3e}, loss {el:.3e} "
              f"(bar {bar_l:.3e})")
        assert ez <= bar_z and el <= bar_l
        assert eld <= 1e-6                       # float32 logdet of a matrix of at most 8 x 8
        assert not d["z"][b, :, n * per:].any() and not d["audio"][b, n * HOP:].any()
    # the equal-length batch of two: the sums of both items over the samples of both
    n = int(d["eq_T"])
    terms = [forward_ref(sd, cfg, mel[b:b + 1, :, :n], audio[b:b + 1, :n * HOP]) for b in range(2)]
    z = torch.cat([t[0] for t in terms], 0)
    loss = nll_ref(z, [x for t in terms for x in t[1]], terms[0][2])
    el = abs(float(loss) - float(d["eq_loss"]))
    print(f"equal-length batch: loss {float(loss):.7f}, {el:.3e} from the reference (bar {bar_l:.3e})")
    assert el <= bar_l


def test_restated_inverse_returns_the_audio(golden):
    d = golden("waveglow_fwd_tiny.npz")
    cfg, sd = load_fixture(d)
    mel, audio = torch.from_numpy(d["mel"]), torch.from_numpy(d["audio"])
    for b, n in enumerate(d["lens"].tolist()):
        z, _, _ = forward_ref(sd, cfg, mel[b:b + 1, :, :n], audio[b:b + 1, :n * HOP])
        back = infer_ref(sd, cfg, mel[b:b + 1, :, :n], 1.0, noise_from_z_ref(cfg, z))
        err = (back - audio[b:b + 1, :n * HOP].double()).abs().max().item()
        print(f"item {b}: infer_ref(noise_from_z(forward_ref(audio))) - audio max-abs {err:.3e}")
        assert err <= 1e-9


def test_noise_from_z_order_and_loss_module():
    from rad_mmm_amd.waveglow import WaveGlow, WaveGlowLoss
    m = WaveGlow(**TINY)
    z = torch.arange(8.0)[None, :, None].expand(2, 8, 3)
    noise = m.noise_from_z(z)
    assert [t.shape[1] for t in noise] == m.noise_shapes == [4, 2, 2]
    assert [t[0, :, 0].tolist() for t in noise] == [[4, 5, 6, 7], [2, 3], [0, 1]]
    assert all(torch.equal(a, b) for a, b in zip(noise, noise_from_z_ref(TINY, z)))
    g = torch.Generator().manual_seed(2)
    z = torch.randn(2, 8, 5, generator=g)
    log_s = [torch.randn(2, 4, 5, generator=g), torch.randn(2, 3, 5, generator=g)]
    ld = [torch.tensor(-3.0, dtype=torch.float64), torch.tensor(0.5, dtype=torch.float64)]
    want = ((z.double() ** 2).sum() / (2 * 0.7 ** 2) - sum(t.double().sum() for t in log_s) + 2.5) / z.numel()
    got = WaveGlowLoss(0.7)((z, log_s, ld))
    assert abs(float(got) - float(want)) < 1e-12
    assert float(ld[0]) == -3.0                 # the list is not added into


def test_forward_entry_points_validate_without_gpu():
    lib = ctypes.CDLL(LIB)
    lib.radmmm_last_error.restype = ctypes.c_char_p
    p, i, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    lib.radmmm_wg_group_audio.argtypes = [p, i64, p, i, i, p, i, i, p]
    lib.radmmm_wg_mix_fwd.argtypes = [p, i, i, i, p, p, i, i, p]
    lib.radmmm_wg_end_coupling_fwd.argtypes = [p, i, p, p, p, i, i, i, i, p, i, p, p, i, i, p]
    lib.radmmm_wg_nll_parts.argtypes = [p, i, i, p, p, i, i, p, p]
    d = 0x1000                                   # 16-byte aligned, never dereferenced

    def refused(rc, what):
        assert rc == -1 and what in lib.radmmm_last_error(), lib.radmmm_last_error()

    refused(lib.radmmm_wg_group_audio(None, 80, d, 8, 8, None, 2, 10, None), b"wg_group_audio: null pointer")
    refused(lib.radmmm_wg_group_audio(d, 80, None, 8, 8, None, 2, 10, None), b"wg_group_audio: null pointer")
    refused(lib.radmmm_wg_group_audio(d, 79, d, 8, 8, None, 2, 10, None), b"wg_group_audio: bad dims")     # lda < Tg*n_group
    refused(lib.radmmm_wg_group_audio(d, 80, d, 6, 8, None, 2, 10, None), b"wg_group_audio: bad dims")     # ldx < n_group
    refused(lib.radmmm_wg_group_audio(d, 80, d, 8, 8, None, 0, 10, None), b"wg_group_audio: bad dims")

    refused(lib.radmmm_wg_mix_fwd(None, 8, 0, 8, d, None, 20, 10, None), b"wg_mix_fwd: null pointer")
    refused(lib.radmmm_wg_mix_fwd(d, 8, 0, 8, None, None, 20, 10, None), b"wg_mix_fwd: null pointer")
    for c in (10, 0, -2, 5):
        refused(lib.radmmm_wg_mix_fwd(d, 16, 0, c, d, None, 20, 10, None), b"wg_mix_fwd: bad dims")
    refused(lib.radmmm_wg_mix_fwd(d, 8, 4, 6, d, None, 20, 10, None), b"wg_mix_fwd: bad dims")              # col0 + c > ldx
    refused(lib.radmmm_wg_mix_fwd(d, 8, 0, 8, d, None, 21, 10, None), b"wg_mix_fwd: bad dims")              # rows % T

    def coupling(S=d, We=d, X=d, ls=d, n_half=4, C=32, lds=None, col0=0, ldx=8):
        return lib.radmmm_wg_end_coupling_fwd(S, C if lds is None else lds, We, None, X, ldx, col0, n_half, C, ls, 1, None,
                                              None, 20, 10, None)

    for kw in (dict(S=None), dict(We=None), dict(X=None), dict(ls=None)):
        refused(coupling(**kw), b"wg_end_coupling_fwd: null pointer")
    for kw in (dict(n_half=5, ldx=16), dict(n_half=0), dict(C=0), dict(C=30), dict(C=1024), dict(C=32, lds=28),
               dict(n_half=4, col0=2)):
        refused(coupling(**kw), b"wg_end_coupling_fwd: bad dims")   # C = 1024: 8 * (1024 + 9) > 8192, as its twin

    refused(lib.radmmm_wg_nll_parts(None, 8, 8, d, None, 2, 10, d, None), b"wg_nll_parts: null pointer")
    refused(lib.radmmm_wg_nll_parts(d, 8, 8, None, None, 2, 10, d, None), b"wg_nll_parts: null pointer")
    refused(lib.radmmm_wg_nll_parts(d, 8, 8, d, None, 2, 10, None, None), b"wg_nll_parts: null pointer")
    refused(lib.radmmm_wg_nll_parts(d, 4, 8, d, None, 2, 10, d, None), b"wg_nll_parts: bad dims")
    refused(lib.radmmm_wg_nll_parts(d, 8, 8, d, None, 2, 0, d, None), b"wg_nll_parts: bad dims")
