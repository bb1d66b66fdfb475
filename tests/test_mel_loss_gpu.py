"""GPU checks of the mel L1 loss and the differentiable log-mel (rad_mmm_amd/mel_loss.py: MelSpectrogramLoss,
mel_spectrogram; csrc/mel_loss.hip): losses and gradients against the reference's own (tests/golden/mel_loss_*.npz) and
against the float64 model tests/_mel_loss_ref.py, the forward against the project's forward-only transforms, the fused loss
against F.l1_loss composed from mel_spectrogram, gradient selection, repeatability, the absence of device -> host
synchronisation, the refusals, and one HiFi-GAN generator step.

Bars.  Fixture losses: max(10 |ref32 - ref64| / ref64, 1e-6) relative; fixture gradients: max(10 x the stored
float32-against-float64 deviation, 1e-6) relative L2 (the rule of tests/test_stft_loss_gpu.py and test_vocoder_bwd_gpu.py).
tests/test_mel_loss_cpu.py shows that these bars reject every planted wrong variant in every figure it moves.  Every
comparison prints measured over bar (pytest -s)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _mel_loss_ref as K

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _module(g, mel_basis=None):
    from rad_mmm_amd.mel_loss import MelSpectrogramLoss
    mod = MelSpectrogramLoss(filter_length=g.n_fft, hop_length=g.hop, win_length=g.win, n_mel_channels=g.n_mel,
                             mel_fmax=8000.0 if g.n_fft == 1024 else None).to(DEV)
    if mel_basis is not None:                                   # the fixture's filterbank, bit for bit
        assert np.abs(mod.stft.mel_basis.cpu().numpy() - mel_basis).max() <= 1e-7
        with torch.no_grad():
            mod.stft.mel_basis.copy_(torch.from_numpy(mel_basis))
    return mod


def _run(mod, x, target, lens, frames, need=(True, False)):
    """-> dict(loss, grad_x / grad_t for those `need` asks for), on the device"""
    xs = x.detach().clone().requires_grad_(need[0])
    ts = target.detach().clone().requires_grad_(need[1])
    loss = mod(xs, ts, lens, frames)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.is_cuda
    out = {"loss": loss.detach()}
    if any(need):
        assert loss.grad_fn is not None and type(loss.grad_fn).__name__ == "_MelLossFnBackward"
        loss.backward()
    assert (xs.grad is not None) == need[0] and (ts.grad is not None) == need[1]
    if need[0]:
        out["grad_x"] = xs.grad
    if need[1]:
        out["grad_t"] = ts.grad
    return out


def _check(what, got, want, bars):
    got = {k: v.detach().cpu().numpy() for k, v in got.items()}
    mob = K.measured_over_bar(got, want, {k: b for k, b in bars.items() if k in got})
    for k, v in mob.items():
        print(f"{what} {k}: {v * bars[k]:.3e} = {v:.3f} of its bar {bars[k]:.3e}")
    print(f"RECORD mel_loss {what}: worst measured / bar {max(mob.values()):.3f}")
    bad = {k: v for k, v in mob.items() if not v <= 1.0}
    assert not bad, bad


@pytest.fixture(scope="module", params=K.FIXTURES)
def fx(request, golden):
    name = request.param
    d = golden(f"mel_loss_{name}.npz")
    g = K.fixture_geometry(d)
    audio = d["target"].ndim == 2
    lens = d.get("lens")
    # device lengths as int64 and frames as int32 (small), host lengths (shipped), None (small_win)
    lens_arg = None if lens is None else (_dev(lens, torch.int64) if name == "small" else [int(v) for v in lens])
    return dict(name=name, d=d, g=g, audio=audio, mod=_module(g, d["mel_basis"]), x=_dev(d["x"]), target=_dev(d["target"]),
                lens=lens_arg, frames=_dev(d.get("frames"), torch.int32))


def test_loss_and_gradients_match_the_reference_fixture(fx):
    """fails without the feature: rad_mmm_amd.mel_loss does not exist there"""
    d = fx["d"]
    got = _run(fx["mod"], fx["x"], fx["target"], fx["lens"], fx["frames"], need=(True, fx["audio"]))
    _check(fx["name"], got, K.fixture_want(d), K.fixture_bars(d))
    for b, n in enumerate(d.get("lens", [])):                   # samples past a length get exactly 0
        assert not got["grad_x"][b, n:].any()
    assert torch.isfinite(got["grad_x"]).all()


def test_channel_input_and_the_target_as_audio(fx):
    """x as [B, 1, S] gives the same bits; an audio target gets its gradient only when it asks"""
    base = _run(fx["mod"], fx["x"], fx["target"], fx["lens"], fx["frames"])
    deep = _run(fx["mod"], fx["x"][:, None, :], fx["target"], fx["lens"], fx["frames"])
    assert torch.equal(base["loss"], deep["loss"]) and torch.equal(base["grad_x"], deep["grad_x"][:, 0])
    if fx["audio"]:
        both = _run(fx["mod"], fx["x"], fx["target"], fx["lens"], fx["frames"], need=(True, True))
        only_t = _run(fx["mod"], fx["x"], fx["target"], fx["lens"], fx["frames"], need=(False, True))
        assert torch.equal(both["grad_x"], base["grad_x"]) and torch.equal(both["grad_t"], only_t["grad_t"])
        assert torch.equal(both["loss"], base["loss"]) and torch.equal(only_t["loss"], base["loss"])
        _check(fx["name"] + " target only", only_t, K.fixture_want(fx["d"]), K.fixture_bars(fx["d"]))
    else:
        with pytest.raises(ValueError, match="detach"):
            fx["mod"](fx["x"], fx["target"].clone().requires_grad_(True), fx["lens"], fx["frames"])


def test_no_grad_gives_the_same_bits_and_two_calls_agree(fx):
    a = _run(fx["mod"], fx["x"], fx["target"], fx["lens"], fx["frames"], need=(True, fx["audio"]))
    b = _run(fx["mod"], fx["x"], fx["target"], fx["lens"], fx["frames"], need=(True, fx["audio"]))
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    with torch.no_grad():
        loss = fx["mod"](fx["x"].clone().requires_grad_(True), fx["target"], fx["lens"], fx["frames"])
    assert loss.grad_fn is None and not loss.requires_grad and torch.equal(loss, a["loss"])
    none = _run(fx["mod"], fx["x"], fx["target"], fx["lens"], fx["frames"], need=(False, False))
    assert torch.equal(none["loss"], a["loss"])


def test_forward_and_backward_never_wait_for_the_device(fx):
    mod, x, target = fx["mod"], fx["x"], fx["target"]
    g = fx["g"]
    lens = _dev(fx["d"].get("lens", np.full(g.B, g.S)), torch.int64)
    frames = _dev(fx["d"].get("frames", np.full(g.B, g.F)), torch.int32)

    def step():
        xs = x.detach().clone().requires_grad_(True)
        mod(xs, target, lens, frames).backward()
        return xs.grad
    first = step()                                              # builds the padded mel basis on the device
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        grad = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(grad).all() and grad.any() and torch.equal(grad, first)


def test_fused_loss_equals_l1_loss_composed_from_mel_spectrogram(fx):
    """F.l1_loss over the valid region of mel_spectrogram(...) under torch autograd: the loss within 2 ulp of fp32, the
    gradient within 1e-6 relative L2"""
    from rad_mmm_amd.mel_loss import mel_spectrogram
    d, g, mod = fx["d"], fx["g"], fx["mod"]
    fused = _run(mod, fx["x"], fx["target"], fx["lens"], fx["frames"])
    xs = fx["x"].detach().clone().requires_grad_(True)
    mel = mel_spectrogram(xs, mod.stft, fx["lens"])
    assert mel.shape == (g.B, g.n_mel, g.F) and type(mel.grad_fn).__name__ == "_MelFnBackward"
    with torch.no_grad():
        tmel = mel_spectrogram(fx["target"], mod.stft, fx["lens"]) if fx["audio"] else fx["target"]
    Ft = tmel.shape[2]
    n = torch.from_numpy(K.loss_frames(d.get("lens"), d.get("frames"), g, Ft)).to(DEV)
    k = min(g.F, Ft)
    mask = (torch.arange(k, device=DEV)[None, :] < n[:, None])[:, None, :].expand(g.B, g.n_mel, k)
    loss = F.l1_loss(mel[:, :, :k][mask], tmel[:, :, :k][mask])
    loss.backward()
    ulps = abs(float(loss.detach()) - float(fused["loss"])) / float(np.spacing(np.float32(float(loss.detach()))))
    err = K.rel_l2(fused["grad_x"].cpu().numpy(), xs.grad.cpu().numpy())
    print(f"RECORD mel_loss {fx['name']} fused against composed: loss {ulps:.1f} ulp (bar 2), gradient {err:.3e} (bar 1e-6)")
    assert ulps <= 2.0 and err <= 1e-6


def test_mel_spectrogram_forward_equals_the_forward_only_transforms(fx):
    """lens=None against stft.mel_spectrogram(y), lens against stft.mel_spectrogram_ragged(y, lens): both sides are fp32
    evaluations of the same expression, each within tests/_mel_loss_ref.py forward_fp32_bar of the float64 model, so they
    lie within twice that bar of each other, element by element; exact zeros past an item's frames"""
    from rad_mmm_amd.mel_loss import mel_spectrogram
    d, g, stft = fx["d"], fx["g"], fx["mod"].stft
    y = fx["x"]
    lens = d.get("lens")
    for ln in ([None] if lens is None else [None, lens]):
        bar, model = K.forward_fp32_bar(d["x"], ln, g, d["mel_basis"])
        with torch.no_grad():
            mine = mel_spectrogram(y, stft, None if ln is None else _dev(ln, torch.int32)).cpu().numpy()
            if ln is None:
                stock = stft.mel_spectrogram(y).cpu().numpy()
            else:
                stock = stft.mel_spectrogram_ragged(y, [int(v) for v in ln]).cpu().numpy()
        T = stock.shape[2]
        assert mine.shape == (g.B, g.n_mel, g.F) and T <= g.F and not mine[:, :, T:].any()
        worst = []
        for what, a, ref, tol in (("model", mine, model, bar), ("forward-only", mine[:, :, :T], stock, 2 * bar[:, :, :T])):
            err = np.abs(a.astype(np.float64) - ref)
            assert (err <= tol).all(), (what, float(err.max()))
            worst.append(float((err / np.where(tol > 0, tol, 1)).max()))
        print(f"RECORD mel_loss {fx['name']} forward (lens {'None' if ln is None else 'given'}): worst measured / bar "
              f"{worst[0]:.3f} against the model, {worst[1]:.3f} against the forward-only transform")
        if ln is not None:
            for b, n in enumerate(ln):
                assert not mine[b, :, 1 + n // g.hop:].any()


def test_silent_stretch_against_the_float64_model():
    """four frames of exact zeros inside a valid item (re = im = 0 in every bin: the gradient of sqrt there is pinned to 0):
    finite loss and gradient, exact zeros on the samples only those frames hold, and the figures within the bars of the
    `small` fixture, which has this geometry and this kind of signal (loss 1e-6, gradient 10 x its f32_vs_f64/grad_x)"""
    g, mb, x, target, lens, frames, _, (s_lo, s_hi) = K.silent_case()
    want = K.mel_loss(x, target, lens, frames, g, mb)
    from conftest import load_golden
    bars = K.fixture_bars(load_golden("mel_loss_small.npz"))
    got = _run(_module(g, mb), _dev(x), _dev(target), _dev(lens, torch.int64), None)
    assert torch.isfinite(got["loss"]) and torch.isfinite(got["grad_x"]).all()
    assert not got["grad_x"][0, s_lo:s_hi].any() and not got["grad_x"][1, lens[1]:].any()
    _check("silent stretch", got, want, bars)
    empty = _run(_module(g, mb), _dev(x), _dev(target), _dev(lens, torch.int64), _dev(np.array([0, -2]), torch.int32))
    assert float(empty["loss"]) == 0.0 and not empty["grad_x"].any()


def test_refusals_come_before_any_launch():
    from rad_mmm_amd.mel_loss import MelSpectrogramLoss, mel_spectrogram
    mod = MelSpectrogramLoss().to(DEV)
    x, mel = torch.zeros(2, 8192, device=DEV), torch.zeros(2, 80, 33, device=DEV)
    for bad in ([8192, 512], [8193, 4000], [8192, 0]):
        with pytest.raises(ValueError, match="filter_length // 2 = 512"):
            mod(x, mel, bad)
        with pytest.raises(ValueError, match="filter_length // 2 = 512"):
            mel_spectrogram(x, mod.stft, bad)
    with pytest.raises(ValueError, match="reflect-padded"):
        mod(torch.zeros(2, 512, device=DEV), torch.zeros(2, 80, 3, device=DEV))
    with pytest.raises(ValueError, match=r"\[2, 80, Ft\]"):
        mod(x, torch.zeros(2, 64, 33, device=DEV))
    with pytest.raises(ValueError, match=r"\[2, 80, Ft\]"):
        mod(x, torch.zeros(3, 80, 33, device=DEV))
    with pytest.raises(ValueError, match="must agree"):
        mod(x, torch.zeros(2, 8000, device=DEV))
    with pytest.raises(ValueError, match="3 entries for 2 items"):
        mod(x, mel, [8192, 8192, 8192])
    with pytest.raises(ValueError, match="int32 or int64"):
        mod(x, mel, torch.tensor([8192.0, 8192.0], device=DEV))
    big = torch.zeros(1, 8192, device=DEV).expand(16384, 8192)    # no memory behind it: refused by shape
    with pytest.raises(ValueError, match="2 GiB"):
        mod(big, torch.zeros(1, 80, 33, device=DEV).expand(16384, 80, 33))
    with pytest.raises(ValueError, match="2 GiB"):
        mel_spectrogram(big, mod.stft)


def test_one_generator_step_with_this_loss(golden):
    """The r1 fixture generator in train mode, one step with the mel loss of its audio against the fixture's input mel
    (lens * hop samples, lens frames per item; a 16 / 16 / 16 transform with 80 mels so that the 16-sample item can be
    reflect-padded): every parameter gradient is finite and equals, within the vocoder backward's own rule
    (max(10 x f32_vs_f64/<name>, 1e-6) relative L2), the gradient of the same step taken through the composed form,
    F.l1_loss over the valid region of mel_spectrogram(audio)."""
    from _vocoder_ref import load_fixture
    from rad_mmm_amd.mel_loss import MelSpectrogramLoss, mel_spectrogram
    from rad_mmm_amd.vocoder import HiFiGANGenerator
    cfg, sd = load_fixture(golden("vocoder_gen_r1.npz"))
    d = golden("vocoder_gen_bwd_r1.npz")
    lens = d["lens"].tolist()
    gen = HiFiGANGenerator(cfg)
    gen.load_state_dict(sd)
    gen = gen.to(DEV).train()
    mel = torch.from_numpy(d["mel"]).to(DEV)
    hop = int(np.prod(cfg["upsample_rates"]))
    assert hop == 16 and min(lens) * hop > 8
    mod = MelSpectrogramLoss(filter_length=16, hop_length=hop, win_length=16, n_mel_channels=mel.shape[1]).to(DEV)
    samples = torch.tensor([n * hop for n in lens], device=DEV, dtype=torch.int64)
    frames = torch.tensor(lens, device=DEV, dtype=torch.int32)

    gen.zero_grad(set_to_none=True)
    audio = gen(mel, lens)
    loss = mod(audio[:, 0], mel, samples, frames)
    loss.backward()
    got = {k: p.grad.clone() for k, p in gen.named_parameters()}

    gen.zero_grad(set_to_none=True)
    audio2 = gen(mel, lens)
    assert torch.equal(audio2, audio)
    own = mel_spectrogram(audio2[:, 0], mod.stft, samples)
    k = mel.shape[2]
    mask = (torch.arange(k, device=DEV)[None, :] < frames[:, None])[:, None, :].expand(-1, mel.shape[1], -1)
    composed = F.l1_loss(own[:, :, :k][mask], mel[mask])
    composed.backward()
    ref = {k: p.grad for k, p in gen.named_parameters()}
    print(f"generator step: mel loss {float(loss):.9f}, composed {float(composed):.9f}")
    worst, bad = 0.0, []
    for k in sorted(got):
        assert torch.isfinite(got[k]).all(), k
        bar = max(10 * float(d["f32_vs_f64/" + k]), 1e-6)
        err = K.rel_l2(got[k].cpu().numpy(), ref[k].cpu().numpy())
        worst = max(worst, err / bar)
        if not err <= bar:
            bad.append((k, err, bar))
    print(f"RECORD mel_loss generator step: worst measured / bar {worst:.3f} over {len(got)} gradients")
    assert len(got) > 10 and not bad, bad
