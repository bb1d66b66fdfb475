"""GPU checks of the multi-resolution STFT loss (rad_mmm_amd/stft_loss.py: MultiResolutionSTFTLoss, STFTLoss;
csrc/stft_loss.hip): losses and gradients against the reference's own (tests/golden/stft_loss_*.npz) and against the
float64 oracle tests/_stft_loss_ref.py, gradient selection, repeatability, the absence of device -> host synchronisation,
[B, C, T] input, the state_dict keys and one HiFi-GAN generator step.

Bars.  Fixture losses: max(10 |ref32 - ref64| / ref64, 1e-6) relative; fixture gradients: max(10 x the stored
float32-against-float64 deviation, 1e-6) relative L2 (the rule of tests/test_vocoder_bwd_gpu.py).  The default-resolution
cases: 1e-6 relative for the losses and 1e-5 relative L2 for the gradients against the oracle; in the log form the two
log-magnitude gradients, which no fp32 arithmetic holds to 1e-5 on noise-like signals, are asserted against the bar that
tests/_stft_loss_ref.py log_gradient_fp32_bars derives per bin from the rounding of a K-tap fp32 sum.
tests/test_stft_loss_cpu.py shows that these bars reject every planted wrong variant, key by key.  Every comparison prints measured over bar (pytest -s)."""
import numpy as np
import pytest
import torch

import _stft_loss_ref as K

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _module(res=K.FIXTURE_RES, a_weighting=False):
    from rad_mmm_amd.stft_loss import MultiResolutionSTFTLoss
    return MultiResolutionSTFTLoss(list(res[0]), list(res[1]), list(res[2]), a_weighting=a_weighting).to(DEV)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(mod, x, y, ratios, need=(True, True)):
    """-> dict(sc, mag, and of sc_x, sc_y, mag_x, mag_y those that `need` asks for), all on the device"""
    out = {}
    for which in K.LOSS_KEYS:
        xs = x.detach().clone().requires_grad_(need[0])
        ys = y.detach().clone().requires_grad_(need[1])
        sc, mag = mod(xs, ys, ratios)
        assert sc.shape == mag.shape == () and sc.dtype == mag.dtype == torch.float32 and sc.is_cuda and mag.is_cuda
        assert sc.grad_fn is not None and mag.grad_fn is not None
        (sc if which == "sc" else mag).backward()
        out[which] = (sc if which == "sc" else mag).detach()
        assert (xs.grad is not None) == need[0] and (ys.grad is not None) == need[1]
        if need[0]:
            out[which + "_x"] = xs.grad
        if need[1]:
            out[which + "_y"] = ys.grad
    return out


def _check(what, got, want, bars):
    got = {k: v.detach().cpu().numpy() for k, v in got.items()}
    mob = K.measured_over_bar(got, want, {k: b for k, b in bars.items() if k in got})
    for k, v in mob.items():
        print(f"{what} {k}: {v * bars[k]:.3e} = {v:.3f} of its bar {bars[k]:.3e}")
    print(f"RECORD stft_loss {what}: worst measured / bar {max(mob.values()):.3f}")
    bad = {k: v for k, v in mob.items() if not v <= 1.0}
    assert not bad, bad


@pytest.fixture(scope="module", params=K.FIXTURES)
def fx(request, golden):
    name = request.param
    d = golden(f"stft_loss_{name}.npz")
    return dict(name=name, d=d, x=_dev(d["x"]), y=_dev(d["y"]), ratios=_dev(d.get("len_ratios")),
                mod=_module(a_weighting=name.endswith("log1p")))


def test_losses_and_gradients_match_the_reference_fixture(fx):
    """fails without the feature: rad_mmm_amd.stft_loss does not exist there"""
    d = fx["d"]
    got = _run(fx["mod"], fx["x"], fx["y"], fx["ratios"])
    want = {k: float(d[k + "64"]) for k in K.LOSS_KEYS}
    want.update({k: d["grad/" + k] for k in K.GRAD_KEYS})
    _check(fx["name"], got, want, K.fixture_bars(d))
    for b, n in enumerate(d["lengths"]):                       # what lies past a length took part in no valid frame
        if "len_ratios" in d and n + 64 < 600:
            assert not got["sc_x"][b, n + 64:].any() and not got["mag_y"][b, n + 64:].any()


def test_gradients_only_for_arguments_that_ask_and_the_same_bits(fx):
    both = _run(fx["mod"], fx["x"], fx["y"], fx["ratios"])
    only_x = _run(fx["mod"], fx["x"], fx["y"], fx["ratios"], need=(True, False))
    only_y = _run(fx["mod"], fx["x"], fx["y"], fx["ratios"], need=(False, True))
    for k in K.LOSS_KEYS:
        assert torch.equal(both[k], only_x[k]) and torch.equal(both[k], only_y[k])
        assert torch.equal(both[k + "_x"], only_x[k + "_x"]) and torch.equal(both[k + "_y"], only_y[k + "_y"])
    with torch.no_grad():
        sc, mag = fx["mod"](fx["x"], fx["y"], fx["ratios"])
    assert sc.grad_fn is None and torch.equal(sc, both["sc"]) and torch.equal(mag, both["mag"])


def test_two_calls_give_identical_bits(fx):
    a = _run(fx["mod"], fx["x"], fx["y"], fx["ratios"])
    b = _run(fx["mod"], fx["x"], fx["y"], fx["ratios"])
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_identical_arguments_give_exact_zeros(fx):
    got = _run(fx["mod"], fx["x"], fx["x"], fx["ratios"])
    assert float(got["sc"]) == 0.0 and float(got["mag"]) == 0.0
    for k in K.GRAD_KEYS:
        assert torch.isfinite(got[k]).all() and not got[k].any(), k


def test_forward_and_backward_never_wait_for_the_device(fx):
    mod, x, y, ratios = fx["mod"], fx["x"], fx["y"], fx["ratios"]

    def step():
        xs = x.detach().clone().requires_grad_(True)
        sc, mag = mod(xs, y, ratios)
        (sc + mag).backward()
        return xs.grad
    step()                                                      # builds the basis on the device
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        g = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(g).all() and g.any()


def test_channel_input_equals_the_flattened_call(golden):
    d = golden("stft_loss_ragged_log.npz")
    mod = _module()
    x, y = _dev(d["x"][:2]), _dev(d["y"][:2])
    x3 = torch.stack([x, x.flip(0) * 0.5], 1).contiguous()      # [2, 2, T]
    y3 = torch.stack([y, y.flip(0) * 0.5], 1).contiguous()
    ratios = torch.tensor([1.0, 0.7, 0.45, 1.0], device=DEV)
    flat = _run(mod, x3.view(4, -1), y3.view(4, -1), ratios)
    deep = _run(mod, x3, y3, ratios)
    for k in K.LOSS_KEYS:
        assert torch.equal(flat[k], deep[k])
    for k in K.GRAD_KEYS:
        assert deep[k].shape == x3.shape and torch.equal(flat[k], deep[k].view(4, -1))


def test_state_dict_keys_are_the_reference_s(fx):
    assert sorted(fx["mod"].state_dict().keys()) == list(fx["d"]["state_dict_keys"])
    from rad_mmm_amd.stft_loss import MultiResolutionSTFTLoss
    assert sorted(MultiResolutionSTFTLoss().state_dict().keys()) == list(fx["d"]["state_dict_keys"])


def test_short_signals_and_oversized_batches_raise_before_any_launch():
    mod = _module(K.DEFAULT_RES)
    with pytest.raises(ValueError, match="reflect-padded"):
        mod(torch.zeros(2, 1024, device=DEV), torch.zeros(2, 1024, device=DEV))
    big = torch.zeros(1, 8192, device=DEV).expand(4096, 8192)                     # no memory behind it: refused by shape
    with pytest.raises(ValueError, match="2 GiB"):
        mod(big, big)


@pytest.fixture(scope="module")
def probe():
    """B = 2, T = 4096, ragged, with a quiet stretch whose bins lie below the clamp in x only; the seed is searched on the
    CPU, in the oracle only, for bins that stay clear of the kinks in fp32 (tests/_stft_loss_ref.py probe_case)"""
    return K.probe_case(2, 4096, [4096, 2500], K.DEFAULT_RES)


def test_default_resolutions_against_the_float64_oracle(probe):
    """log(1 + m) form: every loss within 1e-6 and every gradient within 1e-5 relative L2; every bin takes part"""
    x, y, ratios, _, seed, (cm, dm) = probe
    want = K.multi_resolution(x, y, ratios, *K.DEFAULT_RES, a_weighting=True)
    print(f"default resolutions: seed {seed}, bins at least {cm:.1f} (clamp) and {dm:.1f} (dlog) fp32 deviations from a kink")
    got = _run(_module(K.DEFAULT_RES, a_weighting=True), _dev(x), _dev(y), _dev(ratios))
    _check("default resolutions log1p B=2 T=4096", got, want, K.ORACLE_BARS)


def test_default_resolutions_log_form_against_the_float64_oracle(probe):
    """log form (the module's default) on the same signals, all six figures asserted: the losses within 1e-6, the
    spectral-convergence gradients within 1e-5, and the two log-magnitude gradients within the derived bar of
    tests/_stft_loss_ref.py log_gradient_fp32_bars (never below 1e-5).  d|log m| / dm = 1 / m hands such a gradient to
    the bins of smallest magnitude, which a K-tap fp32 sum knows to 2^-24 sqrt(K) ||a o w|| only; that bound, pushed
    through 1 / m^2 and the adjoint, is the bar: 7.6e-4 (x) and 9.9e-3 (y) for the seed the search takes.  Stock float32
    torch.stft on the CPU is printed next to it as a record."""
    x, y, ratios, want, seed, _ = probe
    bars = dict(K.ORACLE_BARS_LOG, **K.log_gradient_fp32_bars(want))
    dev = K.stock_fp32_deviation(x, y, ratios, K.DEFAULT_RES)
    print(f"default resolutions, log form, seed {seed}: stock float32 against float64 on the CPU {dev}")
    got = _run(_module(K.DEFAULT_RES), _dev(x), _dev(y), _dev(ratios))
    _check("default resolutions log B=2 T=4096", got, want, bars)


@pytest.mark.parametrize("a_w", [True, False], ids=["log1p", "log"])
def test_one_generator_step_with_this_loss(golden, a_w):
    """The r2 fixture generator trained one step with sc + mag of its audio against a target: the parameter gradients equal,
    within the vocoder backward's own rule (max(10 x f32_vs_f64/<name>, 1e-6) relative L2), those of the same HIP
    generator backward fed with the float64 oracle's gradient of the loss at the HIP generator's audio.  log(1 + m): that
    rule as it stands.  log: the gradient that comes in already carries the loss's own float32 deviation, which the
    reference shows for this form at these resolutions (1.5e-5, f32_vs_f64/mag_x of stft_loss_ragged_log.npz); the two
    deviations add: max(10 x (f32_vs_f64/<name> + 1.5e-5), 1e-6)."""
    from _vocoder_ref import load_fixture
    from rad_mmm_amd.vocoder import HiFiGANGenerator
    cfg, sd = load_fixture(golden("vocoder_gen_r2.npz"))
    d = golden("vocoder_gen_bwd_r2.npz")
    lens = d["lens"].tolist()
    gen = HiFiGANGenerator(cfg)
    gen.load_state_dict(sd)
    gen = gen.to(DEV).train()
    mel = torch.from_numpy(d["mel"]).to(DEV)
    hop = int(np.prod(cfg["upsample_rates"]))
    T = mel.shape[2] * hop
    ratios = (np.asarray(lens, dtype=np.float32) * np.float32(hop) / np.float32(T)).astype(np.float32)
    mod = _module(a_weighting=a_w)
    loss_dev = 0.0 if a_w else float(golden("stft_loss_ragged_log.npz")["f32_vs_f64/mag_x"])
    with torch.no_grad():
        audio0 = gen(mel, lens)[:, 0].cpu().numpy()
    for seed in range(20):              # the fixture's own target; noise on it until the oracle's bins are clear of the kinks
        target = d["target"] + (0.1 * np.random.RandomState(seed).randn(*audio0.shape).astype(np.float32) if seed else 0)
        target = target.astype(np.float32)
        for b, n in enumerate(lens):
            target[b, n * hop:] = 0
        want = K.multi_resolution(audio0, target, ratios, *K.FIXTURE_RES, a_weighting=a_w)
        cm, dm = K.fp32_kink_ratios(want["res"])
        if cm > K.KINK_FACTOR and dm > K.KINK_FACTOR:
            break
    else:
        raise AssertionError("no target seed keeps the bins clear of the kinks")
    gen.zero_grad(set_to_none=True)
    audio = gen(mel, lens)
    assert np.array_equal(audio.detach()[:, 0].cpu().numpy(), audio0)
    sc, mag = mod(audio[:, 0], _dev(target), _dev(ratios))
    (sc + mag).backward()
    got = {k: p.grad.clone() for k, p in gen.named_parameters()}
    gen.zero_grad(set_to_none=True)
    audio = gen(mel, lens)
    audio.backward(_dev((want["sc_x"] + want["mag_x"]).astype(np.float32))[:, None, :])
    ref = {k: p.grad.cpu().numpy() for k, p in gen.named_parameters()}
    bars = {k: max(10 * (float(d["f32_vs_f64/" + k]) + loss_dev), 1e-6) for k in got}
    sc, mag = sc.detach(), mag.detach()
    print(f"generator step: sc {float(sc):.9f} (oracle {want['sc']:.9f}), mag {float(mag):.9f} (oracle {want['mag']:.9f})")
    worst = 0.0
    bad = []
    for k in sorted(got):
        err = K.rel_l2(got[k].cpu().numpy(), ref[k])
        worst = max(worst, err / bars[k])
        if not err <= bars[k]:
            bad.append((k, err, bars[k]))
    print(f"RECORD stft_loss generator step {'log1p' if a_w else 'log'} (target seed {seed}): worst measured / bar {worst:.3f} over {len(got)} gradients")
    assert not bad, bad
