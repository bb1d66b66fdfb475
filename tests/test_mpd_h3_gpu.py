"""GPU checks of MultiPeriodDiscriminator.precision = "h3" (rad_mmm_amd/discriminators.py, csrc/mpd_h3.hip): the losses and
every gradient against the float64 restatement tests/_mpd_ref.py under the bar rule of tests/test_mpd_gpu.py, unchanged --
a loss within max(10 * |loss32 - loss64|, 1e-6 * |loss64|), a gradient within max(10 * d, 1e-6) relative L2, d the deviation
of the restatement's own float32 run on the CPU from its float64 run (tests/_mpd_h3_cases.py; never taken from the code
under test).  The same bars as fp32 hold because three split products are fp32-class by construction; the audio of a case
is chosen by the restatement alone (clear of the kinks, well-conditioned conv_post.weight_g numbers: _mpd_h3_cases.audio_seed).
Then: which kernels
a step launches, that "fp32" keeps its bits and launches whichever way the mode is chosen, repeatability without a device ->
host synchronisation, selective gradients, the saturation guard through HiFiGANTrainingStep, the split weights' cache, and
the reference's widths.  Every comparison prints measured over bar (pytest -s).  Every test fails without the feature: the
attribute and the per-call argument do not exist there."""
import json
import os

import numpy as np
import pytest
import torch

import _mpd_h3_cases as K
import _mpd_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(a):
    return None if a is None else torch.as_tensor(a).float().to(DEV)


def _model(sd, channels=K.CHANNELS, plain=False, precision="h3"):
    from rad_mmm_amd.discriminators import MultiPeriodDiscriminator
    m = MultiPeriodDiscriminator(channels=channels)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    if plain:
        m.remove_weight_norm()
    m.precision = precision
    return m.to(DEV).train()


def _step(mpd, y, y_hat, ratios, real_grad=False, **kw):
    """the fixtures' loss L = 2 fm + gen + disc in one backward through the two fused methods -> (losses, gradients)"""
    mpd.zero_grad(set_to_none=True)
    yh = y_hat.detach().clone().requires_grad_(True)
    yr = y.detach().clone().requires_grad_(real_grad)
    fm, gen = mpd.generator_losses(yr, yh, ratios, **kw)
    disc, r_l, g_l = mpd.discriminator_loss(yr, yh, ratios, **kw)
    (2 * fm + gen + disc).backward()
    grads = {k: p.grad.clone() for k, p in mpd.named_parameters()}
    grads["y_hat"] = yh.grad.clone()
    if real_grad:
        grads["y"] = yr.grad.clone()
    return {"fm": fm.detach(), "gen": gen.detach(), "disc": disc.detach(), "r_losses": r_l.detach(), "g_losses": g_l.detach()}, grads


def _check(what, losses, grads, w64, lbars, gbars):
    bad, worst = [], 0.0
    for k in K.LOSSES:
        err = float(np.abs(losses[k].double().cpu().numpy() - np.asarray(w64[k])).max())
        print(f"{what} {k}: {err:.3e} from float64 = {err / lbars[k]:.3f} of its bar {lbars[k]:.3e}")
        if not err <= lbars[k]:
            bad.append((k, err, lbars[k]))
    for k in sorted(grads):
        want = w64["grad_y"] if k == "y" else w64["grad"][k]
        err = R.relative_l2(grads[k].detach().cpu().numpy().reshape(-1), np.asarray(want).reshape(-1))
        worst = max(worst, err / gbars[k])
        print(f"{what} {k}: relative L2 {err:.3e} = {err / gbars[k]:.3f} of its bar {gbars[k]:.3e}")
        if not err <= gbars[k]:
            bad.append((k, err, gbars[k]))
    print(f"{what}: worst gradient measured / bar {worst:.3f}")
    assert not bad, bad


def _inputs(c):
    return _dev(c["y"]), _dev(c["y_hat"]), _dev(c["ratios"])


@pytest.mark.parametrize("T,ragged,plain,real_grad", [(97, True, False, True), (97, False, False, False), (64, True, False, False),
                                                      (64, True, True, False)],
                         ids=["t97_ragged_and_real_audio", "t97_plain_means", "t64_ragged", "t64_ragged_without_weight_norm"])
def test_losses_and_gradients_against_the_restatement(T, ragged, plain, real_grad):
    c = K.case(T, ragged, plain)
    mpd = _model(c["sd"], plain=plain)
    assert plain == (not any(k.endswith("weight_g") for k, _ in mpd.named_parameters()))
    assert all(m["convs.1"][0] == m["convs.4"][0] == "h3" for m in mpd.precision_plan(B=K.B, T=T))
    losses, grads = _step(mpd, *_inputs(c), real_grad=real_grad)
    assert set(grads) - {"y"} == set(c["w64"]["grad"])
    _check(f"h3 T={T}", losses, grads, c["w64"], K.loss_bars(c["w32"], c["w64"]), K.grad_bars(c["w32"], c["w64"]))
    assert not mpd.grad_saturated()
    # the views of forward(): fp32, the reference's shapes, differentiable, and the fused losses' values
    rs, gs, frs, fgs = mpd(*_inputs(c)[:2])
    for i, p in enumerate(R.PERIODS):
        H = -(-T // p)
        for l, C in enumerate(K.CHANNELS + (1,)):
            H = (H - 1) // 3 + 1 if l < 4 else H
            assert tuple(frs[i][l].shape) == tuple(fgs[i][l].shape) == (K.B, C, H, p) and frs[i][l].dtype == torch.float32
            assert frs[i][l].untyped_storage().data_ptr() == fgs[i][l].untyped_storage().data_ptr() and frs[i][l].requires_grad
        assert tuple(rs[i].shape) == tuple(gs[i].shape) == (K.B, H * p)
    disc, _, _ = R.discriminator_loss(rs, gs, _inputs(c)[2])
    assert abs(float(disc.detach()) - float(losses["disc"])) <= 1e-6 * abs(float(losses["disc"]))


@pytest.mark.parametrize("channels,modes", [((32, 48, 64, 32, 32), ["fp32", "fp32", "fp32", "h3", "h3", "fp32"]),
                                            ((32, 32, 64, 48, 32), ["fp32", "h3", "h3", "fp32", "fp32", "fp32"])],
                         ids=["fp32_below_h3", "fp32_above_h3"])
def test_an_h3_conv_beside_an_fp32_conv(channels, modes, monkeypatch):
    """widths at which the split kernels refuse some wide convs (C_out = 48, K = 5 * 48): an fp32 conv feeds an "h3" one
    (mpdh3_repad after an fp32 GEMM, the "h3" data gradient into mpd_unframe) and an "h3" conv feeds an fp32 one (the fp32
    data-gradient GEMM into mpdh3_unframe, conv_post's fp32 dZ kernel above an fp32 conv); the same bars"""
    import rad_mmm_amd.discriminators as D
    c = K.case(64, True, False, channels)
    mpd = _model(c["sd"], channels)
    assert all([m for m, _ in p.values()] == modes for p in mpd.precision_plan(B=K.B, T=64))
    monkeypatch.setattr(D, "LAUNCHES", {})
    losses, grads = _step(mpd, *_inputs(c))
    n_h3 = modes.count("h3")
    assert D.LAUNCHES["conv_h3"] == D.LAUNCHES["dgrad_h3"] == D.LAUNCHES["wgrad_rm"] == 2 * 5 * n_h3
    assert D.LAUNCHES["dgrad"] == 2 * 5 * (4 - n_h3) and D.LAUNCHES["mpdh3_unframe"] + D.LAUNCHES["mpd_unframe"] == 2 * 5 * 4
    assert ("mpdh3_conv_post_dgrad" in D.LAUNCHES) == (modes[4] == "h3") and ("mpd_conv_post_dgrad" in D.LAUNCHES) == (modes[4] != "h3")
    _check(f"mixed {channels}", losses, grads, c["w64"], K.loss_bars(c["w32"], c["w64"]), K.grad_bars(c["w32"], c["w64"]))


def test_a_step_runs_the_kernels_it_claims(monkeypatch):
    import rad_mmm_amd.discriminators as D
    from rad_mmm_amd._lib import rowgemm_h3_last_kernel
    c = K.case(97, True)
    mpd = _model(c["sd"])
    y, y_hat, ratios = _inputs(c)
    monkeypatch.setattr(D, "LAUNCHES", {})
    with torch.no_grad():
        mpd(y, y_hat)
    assert rowgemm_h3_last_kernel() // 100 % 10 == 3              # a three-product kernel
    n = 5                                                         # members
    assert D.LAUNCHES == {"mpd_fold_frame": n, "conv": n, "conv_h3": 4 * n, "mpdh3_repad": 4 * n, "mpd_repad": n, "mpd_conv_post": n,
                          "split_w": 4 * n, "transpose_w": 4 * n}
    D.LAUNCHES.clear()
    _step(mpd, y, y_hat, ratios)                                  # two fused calls, every gradient but the real audio's
    L = D.LAUNCHES
    assert L["conv_h3"] == L["mpdh3_repad"] == L["dgrad_h3"] == L["mpdh3_frame"] == L["wgrad_rm"] == 2 * 4 * n
    assert L["mpdh3_conv_post_dgrad"] == 2 * n and L["mpdh3_unframe"] == 2 * 3 * n
    assert L["conv"] == L["mpd_repad"] == L["mpd_unframe"] == L["wgrad"] == 2 * n       # convs.0 and what surrounds it
    assert not {"dgrad", "mpd_frame", "mpd_conv_post_dgrad", "split_w", "transpose_w"} & set(L)


def test_fp32_keeps_its_bits_and_launches_however_the_mode_is_chosen(monkeypatch):
    import rad_mmm_amd.discriminators as D
    c = K.case(64, True)
    y, y_hat, ratios = _inputs(c)
    monkeypatch.setattr(D, "LAUNCHES", {})
    runs = {}
    for key, attr, arg in (("plain", "fp32", {}), ("h3 attribute, fp32 call", "h3", {"precision": "fp32"}),
                           ("h3 attribute", "h3", {}), ("fp32 attribute, h3 call", "fp32", {"precision": "h3"})):
        mpd = _model(c["sd"], precision=attr)
        D.LAUNCHES.clear()
        runs[key] = _step(mpd, y, y_hat, ratios, **arg) + (dict(D.LAUNCHES),)
        with torch.no_grad():
            runs[key] += (torch.cat([t.reshape(-1) for t in mpd(y, y_hat, **arg)[2][4]]),)
    for a, b in (("plain", "h3 attribute, fp32 call"), ("h3 attribute", "fp32 attribute, h3 call")):
        for x, z in zip(runs[a][:2], runs[b][:2]):
            assert set(x) == set(z) and all(torch.equal(x[k], z[k]) for k in x), (a, b)
        assert runs[a][2] == runs[b][2] and torch.equal(runs[a][3], runs[b][3])
    assert not any("h3" in k or k in ("split_w", "wgrad_rm") for k in runs["plain"][2])
    assert not torch.equal(runs["plain"][1]["y_hat"], runs["h3 attribute"][1]["y_hat"])        # the modes are two arithmetics


def test_repeatable_and_free_of_synchronisation():
    c = K.case(97, True)
    mpd = _model(c["sd"])
    y, y_hat, ratios = _inputs(c)
    first = _step(mpd, y, y_hat, ratios)                          # also warms every lazily initialised piece up
    flag = mpd.saturation_flag()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = _step(mpd, y, y_hat, ratios)
        mpd.zero_grad(set_to_none=True)
        rs, gs, frs, fgs = mpd(y, y_hat)
        (rs[0].sum() + fgs[4][2].sum()).backward()
        with torch.no_grad():
            mpd.eval()
            mpd.discriminator_loss(y, y_hat, ratios)
            mpd.train()
        assert mpd.saturation_flag() is flag
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for a, b in zip(first, second):
        assert set(a) == set(b)
        for k in a:
            assert torch.equal(a[k], b[k]), k


def test_only_the_requested_gradients_are_computed(monkeypatch):
    import rad_mmm_amd.discriminators as D
    c = K.case(64, True)
    mpd = _model(c["sd"])
    y, y_hat, ratios = _inputs(c)
    walks, inner = [], D._walk
    monkeypatch.setattr(D, "_walk", lambda g, tape, W, s0, n, *a: walks.append((g.S, s0, n)) or inner(g, tape, W, s0, n, *a))
    monkeypatch.setattr(D, "LAUNCHES", {})
    # the D step: parameter gradients, no audio gradient formed
    yh = y_hat.clone().requires_grad_(True)
    mpd.discriminator_loss(y, yh.detach(), ratios)[0].backward()
    assert yh.grad is None and all(p.grad is not None and p.grad.abs().max() > 0 for p in mpd.parameters())
    assert "dgrad_audio" not in D.LAUNCHES and "mpd_unfold_audio" not in D.LAUNCHES and "mpd_fm_terms" not in D.LAUNCHES
    assert D.LAUNCHES["wgrad_rm"] == 4 * 5 and D.LAUNCHES["wgrad"] == 5 and all(s0 == 0 and n == S for S, s0, n in walks)
    # the G side: with and without parameter gradients the audio gradient has the same bits; frozen: no weight gradient
    # launch, and the generated half of every buffer is walked alone
    fm, gen = mpd.generator_losses(y, yh, ratios)
    (fm + gen).backward()
    with_params = yh.grad.clone()
    for p in mpd.parameters():
        p.requires_grad_(False)
    yh.grad = None
    D.LAUNCHES.clear()
    walks.clear()
    fm, gen = mpd.generator_losses(y, yh, ratios)
    (fm + gen).backward()
    assert torch.equal(yh.grad, with_params)
    assert not {"wgrad_rm", "mpdh3_frame", "wgrad", "colsum", "mpd_frame", "mpd_conv_post_wgrad", "colsum_final"} & set(D.LAUNCHES)
    assert D.LAUNCHES["dgrad_h3"] == 4 * 5 and D.LAUNCHES["dgrad_audio"] == D.LAUNCHES["mpd_unfold_audio"] == 5
    assert len(walks) == 5 and all(s0 == n == S // 2 for S, s0, n in walks)


def test_the_split_weights_are_made_once_per_parameter_version(monkeypatch):
    import rad_mmm_amd.discriminators as D
    c = K.case(64, True)
    mpd = _model(c["sd"])
    y, y_hat, ratios = _inputs(c)
    opt = torch.optim.SGD(mpd.parameters(), lr=0.05)
    monkeypatch.setattr(D, "LAUNCHES", {})
    loss = mpd.discriminator_loss(y, y_hat, ratios)[0]
    assert D.LAUNCHES["split_w"] == D.LAUNCHES["transpose_w"] == 4 * 5
    loss.backward()
    D.LAUNCHES.clear()
    again = mpd.discriminator_loss(y, y_hat, ratios)[0]           # no step in between: the copies are reused
    with torch.no_grad():
        mpd(y, y_hat)
    assert "split_w" not in D.LAUNCHES and "transpose_w" not in D.LAUNCHES and torch.equal(again, loss)
    opt.step()
    after = mpd.discriminator_loss(y, y_hat, ratios)[0]
    assert D.LAUNCHES["split_w"] == D.LAUNCHES["transpose_w"] == 4 * 5 and not torch.equal(after, loss)
    fresh = _model({k: v.detach().cpu() for k, v in mpd.state_dict().items()})
    assert torch.equal(fresh.discriminator_loss(y, y_hat, ratios)[0], after)   # the new weights, not the cached ones


# ---- the guard, through HiFiGANTrainingStep (the narrow models of tests/test_vocoder_step_gpu.py, the MPD at h3 widths) ----
def _training_step(grad_scale):
    from rad_mmm_amd.discriminators import MultiPeriodDiscriminator, MultiScaleDiscriminator
    from rad_mmm_amd.vocoder import HiFiGANGenerator
    from rad_mmm_amd.vocoder_step import HiFiGANTrainingStep
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "vocoder_gen_r2.npz"))
    gen = HiFiGANGenerator(json.loads(str(d["config"])))
    gen.load_state_dict({k[3:]: torch.from_numpy(d[k].astype(np.float32)) for k in d.files if k.startswith("sd/")})
    torch.manual_seed(21)
    mpd = MultiPeriodDiscriminator(channels=K.CHANNELS)
    msd = MultiScaleDiscriminator((8, 8, 16, 16, 32, 32, 16), (1, 2, 2, 4, 4, 4, 1))
    mpd.grad_scale = grad_scale
    step = HiFiGANTrainingStep(gen.to(DEV), mpd.to(DEV), msd.to(DEV), mpd_precision="h3")
    g = torch.Generator().manual_seed(33)
    mel = (torch.randn(3, 80, 4, generator=g) - 2.0).to(DEV)
    audio = torch.rand(3, 1, 4 * 256, generator=g) - 0.5
    lens = [4, 3, 4]
    for b, n in enumerate(lens):
        audio[b, :, n * 256:] = 0.0
    return step, mel, lens, audio.to(DEV)


def _optimizer_state(step):
    out = {}
    for name, opt in (("g", step.optim_g), ("d", step.optim_d)):
        out[name + ".step"] = opt._step.clone()
        for i, b in enumerate(opt.buckets):
            for k in ("flat", "m", "v"):
                out[f"{name}.{i}.{k}"] = b[k].clone()
    return out


def test_a_clamped_step_changes_nothing_and_the_automatic_scale_does_not_clamp():
    step, mel, lens, audio = _training_step(2.0 ** 40)            # 2^40 times any gradient of this step is beyond 60000
    assert step.mpd.precision == "h3"
    before = _optimizer_state(step)
    out = step.training_step(mel, lens, audio)                    # a clamp is ordinary arithmetic, not a fault
    after = _optimizer_state(step)
    assert all(torch.equal(before[k], after[k]) for k in before) and int(after["g.step"]) == int(after["d.step"]) == 0
    assert all(bool(torch.isfinite(v)) for v in out.values())
    assert step.mpd.grad_saturated() is True and step.mpd.grad_saturated() is False             # read and cleared
    step, mel, lens, audio = _training_step(None)
    before = _optimizer_state(step)
    step.training_step(mel, lens, audio)
    after = _optimizer_state(step)
    assert int(step.mpd.saturation_flag().item()) == 0 and step.mpd.grad_saturated() is False
    assert int(after["g.step"]) == int(after["d.step"]) == 1
    assert not torch.equal(before["g.0.flat"], after["g.0.flat"]) and not torch.equal(before["d.0.flat"], after["d.0.flat"])
    with pytest.raises(ValueError, match="precision"):
        from rad_mmm_amd.vocoder_step import HiFiGANTrainingStep
        HiFiGANTrainingStep(step.generator, step.mpd, step.msd, mpd_precision="f16")


def test_real_widths_against_the_restatement():
    """B = 2, T = 97 at the reference's widths (K up to 5120): the inputs and the bar rule of tests/test_mpd_gpu.py's case of
    the same name -- the first audio seed at which the float64 restatement, alone, shows well-conditioned conv_post.weight_g
    gradients (condition number below 100); every bar max(10 d, 1e-6) with d measured from the restatement's float32 run;
    nothing excluded"""
    sd = R.make_state(K.WIDE)
    ratios = torch.tensor([1.0, 0.7])
    for seed in range(20):
        gen = torch.Generator().manual_seed(seed)
        y, y_hat = torch.rand(2, 1, 97, generator=gen) * 2 - 1, torch.rand(2, 1, 97, generator=gen) * 2 - 1
        w64 = R.run(sd, y, y_hat, ratios, torch.float64)
        cond = max(R.weight_g_condition(sd, w64["grad"], f"discriminators.{i}.conv_post.") for i in range(5))
        print(f"wide: input seed {seed}, largest condition number of a conv_post.weight_g gradient {cond:.1f}")
        if cond < 100:
            break
    else:
        raise AssertionError("no input seed gives well-conditioned conv_post.weight_g gradients")
    w32 = R.run(sd, y, y_hat, ratios, torch.float32)
    mpd = _model(sd, K.WIDE)
    losses, grads = _step(mpd, y.to(DEV), y_hat.to(DEV), ratios.to(DEV))
    assert set(grads) == set(w64["grad"])
    _check("h3 wide", losses, grads, w64, K.loss_bars(w32, w64), K.grad_bars(w32, w64))
    assert not mpd.grad_saturated()
