"""GPU checks of the multi-scale discriminator (rad_mmm_amd/discriminators.py, csrc/msd.hip): the losses and every gradient
against the reference's own (tests/golden/msd_t97.npz / msd_t64.npz) and against the float64 restatement (tests/_msd_ref.py),
spectral norm's power iteration, eval mode, the views of forward(), selective gradients, repeatability, the absence of device
-> host synchronisation and the reference's widths.

Bars (the rule of tests/test_mpd_gpu.py).  A loss is within max(10 * |loss32 - loss64|, 1e-6 * |loss64|) of the reference's
float64 value, a gradient within max(10 * f32_vs_f64/<name>, 1e-6) relative L2, the whole tensor compared: ten times what
the reference's own float32 run deviates from its float64 run.  Where no fixture exists the deviation d is measured in the
test by running the restatement in float32 on the CPU against its float64 run, never taken from the code under test.  Every
comparison prints measured over bar (pytest -s).

The fixtures' loss L = 2 fm + gen + disc comes from ONE forward of the reference, the fused methods are two calls, and a
training-mode call advances the spectral-norm member's weight_u / weight_v: _step() puts those buffers back between its two
calls, so that both see the weights the reference's one forward saw, and they end where the reference's end (sd_after)."""
import numpy as np
import pytest
import torch

import _msd_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KEYS = ("fm", "gen", "disc", "r_losses", "g_losses")
WIDE = ((128, 128, 256, 512, 1024, 1024, 1024), (1, 4, 16, 16, 16, 16, 1))


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(dtype).to(DEV)


def _model(sd, channels, groups, plain=False):
    from rad_mmm_amd.discriminators import MultiScaleDiscriminator
    m = MultiScaleDiscriminator(channels, groups)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    if plain:
        m.remove_weight_norm()
    return m.to(DEV).train()


def _sd(d):
    return {k[3:]: d[k] for k in d if k.startswith("sd/")}


def _vectors(msd):
    return {k: v for k, v in msd.named_buffers() if k.endswith(("weight_u", "weight_v"))}


def _step(msd, y, y_hat, ratios, y_grad=False):
    """L = 2 fm + gen + disc in one backward through the two fused methods -> (losses, gradients)"""
    msd.zero_grad(set_to_none=True)
    yh = y_hat.detach().clone().requires_grad_(True)
    yy = y.detach().clone().requires_grad_(y_grad)
    before = {k: v.clone() for k, v in _vectors(msd).items()}
    fm, gen = msd.generator_losses(yy, yh, ratios)
    with torch.no_grad():
        for k, v in _vectors(msd).items():
            v.copy_(before[k])
    disc, r_l, g_l = msd.discriminator_loss(yy, yh, ratios)
    (2 * fm + gen + disc).backward()
    grads = {k: p.grad.clone() for k, p in msd.named_parameters()}
    grads["y_hat"] = yh.grad.clone()
    if y_grad:
        grads["y"] = yy.grad.clone()
    return {"fm": fm.detach(), "gen": gen.detach(), "disc": disc.detach(), "r_losses": r_l.detach(), "g_losses": g_l.detach()}, grads


def _check_losses(what, got, want64, bars):
    bad = []
    for k in sorted(bars):
        err = float(np.abs(got[k].double().cpu().numpy() - np.asarray(want64[k])).max())
        print(f"{what} {k}: {err:.3e} from float64 = {err / bars[k]:.3f} of its bar {bars[k]:.3e}")
        if not err <= bars[k]:
            bad.append((k, err, bars[k]))
    assert not bad, bad


def _check_grads(what, got, want, bars):
    worst, bad = 0.0, []
    for k in sorted(bars):
        err = R.relative_l2(got[k].detach().cpu().numpy().reshape(-1), np.asarray(want[k]).reshape(-1))
        worst = max(worst, err / bars[k])
        print(f"{what} {k}: relative L2 {err:.3e} = {err / bars[k]:.3f} of its bar {bars[k]:.3e}")
        if not err <= bars[k]:
            bad.append((k, err, bars[k]))
    print(f"{what}: worst measured / bar {worst:.3f}")
    assert not bad, bad


def _loss_bars(l32, l64):
    return {k: max(10 * float(np.abs(np.asarray(l32[k]) - np.asarray(l64[k])).max()), 1e-6 * float(np.abs(l64[k]).max()))
            for k in KEYS}


@pytest.fixture(scope="module", params=["t97", "t64"])
def fx(request, golden):
    d = golden(f"msd_{request.param}.npz")
    sd = _sd(d)
    lr = torch.from_numpy(d["len_ratios"])
    return dict(name=request.param, d=d, sd=sd, y=_dev(d["y"]), y_hat=_dev(d["y_hat"]), ratios=_dev(d["len_ratios"]),
                narrow=(tuple(int(c) for c in d["widths"]), tuple(int(g) for g in d["groups"])),
                w64=R.run(sd, d["y"], d["y_hat"], lr), w32=R.run(sd, d["y"], d["y_hat"], lr, torch.float32))


def test_losses_gradients_and_power_iteration_match_the_reference_fixture(fx):
    d = fx["d"]
    msd = _model(fx["sd"], *fx["narrow"])
    losses, grads = _step(msd, fx["y"], fx["y_hat"], fx["ratios"])
    _check_losses(fx["name"], losses, {k: d[k + "64"] for k in KEYS},
                  _loss_bars({k: d[k + "32"] for k in KEYS}, {k: d[k + "64"] for k in KEYS}))
    names = [k[5:] for k in d if k.startswith("grad/")]
    assert set(names) == set(grads)
    _check_grads(fx["name"], grads, {k: d["grad/" + k] for k in names},
                 {k: max(10 * float(d["f32_vs_f64/" + k]), 1e-6) for k in names})
    vec = _vectors(msd)
    assert len(vec) == 16
    for k, v in vec.items():             # two power iterations in float32 against the reference's float64 vectors
        err = float(np.abs(v.cpu().numpy() - d["sd_after/" + k]).max())
        assert err <= 1e-5, (k, err)
    msd.load_state_dict({k: torch.as_tensor(v) for k, v in fx["sd"].items()})
    with torch.no_grad():
        rs, gs, _, _ = msd(fx["y"], fx["y_hat"])
    for i in range(3):
        for got, key in ((rs[i], f"out_r/{i}"), (gs[i], f"out_g/{i}")):
            assert got.shape == d[key].shape
            assert R.relative_l2(got.cpu().numpy(), d[key]) <= 1e-5, key


def test_eval_mode_is_one_pass_with_the_buffers_untouched(fx, monkeypatch):
    import rad_mmm_amd.discriminators as D
    msd = _model(fx["sd"], *fx["narrow"]).eval()
    before = {k: v.clone() for k, v in _vectors(msd).items()}
    monkeypatch.setattr(D, "LAUNCHES", {})
    with torch.no_grad():
        rs, gs, frs, fgs = msd(fx["y"], fx["y"])
    assert D.LAUNCHES["msd_gconv_fwd"] == 3 * 5 and D.LAUNCHES["msd_frame15"] == 3 and D.LAUNCHES["msd_avgpool"] == 2
    for i in range(3):
        assert torch.equal(rs[i], gs[i])
        for a, b in zip(frs[i], fgs[i]):
            assert torch.equal(a, b)
    for k, v in _vectors(msd).items():
        assert torch.equal(v, before[k]), k
    want = R.run(fx["sd"], fx["d"]["y"], fx["d"]["y"], None, training=False)
    for i in range(3):
        assert R.relative_l2(rs[i].cpu().numpy(), want["out_r"][i]) <= 1e-5
    # training mode: the same audio through two weight sets, twice the member's launches
    msd.train()
    D.LAUNCHES.clear()
    with torch.no_grad():
        rs, gs, _, _ = msd(fx["y"], fx["y"])
    assert D.LAUNCHES["msd_gconv_fwd"] == 4 * 5
    assert not torch.equal(rs[0], gs[0]) and torch.equal(rs[1], gs[1]) and torch.equal(rs[2], gs[2])


def test_plain_weight_gradients_match_the_restatement(fx):
    """after remove_weight_norm(): the weight-normed members hold plain weights; against the float64 restatement's
    gradients of those weights"""
    d = fx["d"]
    msd = _model(fx["sd"], *fx["narrow"], plain=True)
    names = [k for k, _ in msd.named_parameters()]
    assert not any(k.endswith("weight_g") for k in names) and "discriminators.0.convs.0.weight_orig" in names
    folded = R.fold_plain(fx["sd"])
    sd = {k: v for k, v in fx["sd"].items() if k.startswith("discriminators.0.")}
    sd.update({k: v.numpy() for k, v in folded.items() if not k.startswith("discriminators.0.")})
    lr = torch.from_numpy(d["len_ratios"])
    want, want32 = R.run(sd, d["y"], d["y_hat"], lr), R.run(sd, d["y"], d["y_hat"], lr, torch.float32)
    losses, grads = _step(msd, fx["y"], fx["y_hat"], fx["ratios"])
    _check_losses(fx["name"] + " plain", losses, want, _loss_bars(want32, want))
    assert set(grads) == set(want["grad"])
    _check_grads(fx["name"] + " plain", grads, want["grad"],
                 {k: max(10 * R.relative_l2(want32["grad"][k], want["grad"][k]), 1e-6) for k in grads})


def test_gradient_of_the_real_audio(fx):
    """y.requires_grad_(): the full walk with both audio gradients through the pools, against the float64 restatement; bars
    from the restatement's own float32 run"""
    msd = _model(fx["sd"], *fx["narrow"])
    w64, w32 = fx["w64"], fx["w32"]
    _, grads = _step(msd, fx["y"], fx["y_hat"], fx["ratios"], y_grad=True)
    want = {"y": w64["grad_y"], "y_hat": w64["grad"]["y_hat"]}
    bars = {"y": max(10 * R.relative_l2(w32["grad_y"], w64["grad_y"]), 1e-6),
            "y_hat": max(10 * R.relative_l2(w32["grad"]["y_hat"], w64["grad"]["y_hat"]), 1e-6)}
    _check_grads(fx["name"] + " audio", {k: grads[k] for k in want}, want, bars)


def test_views_have_the_reference_shapes_and_carry_gradients(fx):
    """forward()'s views: shapes, no copies, and the reference-form losses computed by plain torch on them match the fixture
    in every gradient"""
    d = fx["d"]
    msd = _model(fx["sd"], *fx["narrow"])
    yh = fx["y_hat"].clone().requires_grad_(True)
    rs, gs, frs, fgs = msd(fx["y"], yh)
    B, T = fx["y"].shape[0], fx["y"].shape[2]
    for i in range(3):
        H = T
        bases = set()
        for l, C in enumerate(fx["narrow"][0] + (1,)):
            H = (H - 1) // R.STRIDES[l] + 1
            for m in (frs[i][l], fgs[i][l]):
                assert tuple(m.shape) == (B, C, H), (i, l, m.shape)
            assert frs[i][l].untyped_storage().data_ptr() == fgs[i][l].untyped_storage().data_ptr()       # one stacked buffer
            bases.add(frs[i][l].untyped_storage().data_ptr())
        assert len(bases) == 8
        assert tuple(rs[i].shape) == tuple(gs[i].shape) == (B, H) == d[f"out_r/{i}"].shape
        assert rs[i].untyped_storage().data_ptr() == frs[i][7].untyped_storage().data_ptr()
        T = T // 2 + 1
    fm = R.feature_loss(frs, fgs, fx["ratios"])
    gen = R.generator_loss(gs, fx["ratios"])
    disc, r_l, g_l = R.discriminator_loss(rs, gs, fx["ratios"])
    got = {"fm": fm.detach(), "gen": gen.detach(), "disc": disc.detach(), "r_losses": r_l.detach(), "g_losses": g_l.detach()}
    _check_losses(fx["name"] + " views", got, {k: d[k + "64"] for k in KEYS},
                  _loss_bars({k: d[k + "32"] for k in KEYS}, {k: d[k + "64"] for k in KEYS}))
    (2 * fm + gen + disc).backward()
    via = {k: p.grad.clone() for k, p in msd.named_parameters()}
    via["y_hat"] = yh.grad.clone()
    _check_grads(fx["name"] + " views", via, {k: d["grad/" + k] for k in via},
                 {k: max(10 * float(d["f32_vs_f64/" + k]), 1e-6) for k in via})


def test_only_the_requested_gradients_are_computed(fx, monkeypatch):
    import rad_mmm_amd.discriminators as D
    msd = _model(fx["sd"], *fx["narrow"])
    monkeypatch.setattr(D, "LAUNCHES", {})
    # the D step: parameter gradients, no audio gradient, no data gradient below the first grouped conv
    yh = fx["y_hat"].clone().requires_grad_(True)
    loss, _, _ = msd.discriminator_loss(fx["y"], yh.detach(), fx["ratios"])
    loss.backward()
    assert yh.grad is None
    assert all(p.grad is not None and p.grad.abs().max() > 0 for p in msd.parameters())
    assert not {"dgrad_audio", "msd_unframe15", "msd_avgpool_bwd", "msd_fm_terms", "msd_fm_grad"} & set(D.LAUNCHES)
    passes = 4                                    # the spectral-norm member walks each half with its own weights
    assert D.LAUNCHES["msd_gconv_wgrad"] == 5 * passes and D.LAUNCHES["msd_gconv_dgrad"] == 5 * passes
    assert D.LAUNCHES["wgrad"] == 2 * passes and D.LAUNCHES["mpd_conv_post_wgrad"] == passes
    # the G side: with and without parameter gradients the audio gradient has the same bits; frozen: no weight gradient and
    # the generated half alone
    state = {k: v.clone() for k, v in _vectors(msd).items()}
    fm, gen = msd.generator_losses(fx["y"], yh, fx["ratios"])
    (fm + gen).backward()
    with_params = yh.grad.clone()
    for p in msd.parameters():
        p.requires_grad_(False)
    with torch.no_grad():
        for k, v in _vectors(msd).items():
            v.copy_(state[k])
    yh.grad = None
    D.LAUNCHES.clear()
    fm, gen = msd.generator_losses(fx["y"], yh, fx["ratios"])
    (fm + gen).backward()
    assert torch.equal(yh.grad, with_params)
    assert not {"wgrad", "colsum", "mpd_frame", "mpd_conv_post_wgrad", "msd_gconv_wgrad"} & set(D.LAUNCHES)
    assert D.LAUNCHES["dgrad_audio"] == 3 and D.LAUNCHES["msd_unframe15"] == 3 and D.LAUNCHES["msd_avgpool_bwd"] == 2
    assert D.LAUNCHES["msd_gconv_dgrad"] == 3 * 5


def test_partially_frozen_d_step_stops_where_nothing_below_is_wanted(golden, monkeypatch):
    """A D step (y_hat detached) in training mode with convs.0 .. convs.2 of every member frozen, on the t64 fixture: the
    unfrozen parameters' gradients have the bits of the fully unfrozen step, the frozen ones get none, and each of the four
    passes (the spectral-norm member walks two) stops descending at convs.3.  The power iteration's buffers are put back
    between the runs, so both see the same weights.  The module against itself: no tolerance."""
    import rad_mmm_amd.discriminators as D
    d = golden("msd_t64.npz")
    y, y_hat, ratios = _dev(d["y"]), _dev(d["y_hat"]), _dev(d["len_ratios"])
    msd = _model(_sd(d), tuple(int(c) for c in d["widths"]), tuple(int(g) for g in d["groups"]))
    state = {k: v.clone() for k, v in _vectors(msd).items()}

    def d_step():
        msd.zero_grad(set_to_none=True)
        with torch.no_grad():
            for k, v in _vectors(msd).items():
                v.copy_(state[k])
        msd.discriminator_loss(y, y_hat.detach(), ratios)[0].backward()
        return {k: None if p.grad is None else p.grad.clone() for k, p in msd.named_parameters()}

    full = d_step()
    assert all(g is not None for g in full.values())
    frozen = (0, 1, 2)
    is_frozen = {k: any(f".convs.{l}." in k for l in frozen) for k in full}
    assert sum(is_frozen.values()) == len(frozen) * (2 + 3 + 3)       # weight_orig, bias; weight_g, weight_v, bias twice
    for k, p in msd.named_parameters():
        p.requires_grad_(not is_frozen[k])
    monkeypatch.setattr(D, "LAUNCHES", {})
    part = d_step()
    for k in full:
        if is_frozen[k]:
            assert part[k] is None, k
        else:
            assert torch.equal(part[k], full[k]), k
    assert not {"dgrad_audio", "msd_unframe15", "msd_avgpool_bwd"} & set(D.LAUNCHES)
    # The walk goes conv_post, convs.6 (dense), convs.5 .. convs.1 (grouped), convs.0.  The data gradient of grouped conv l is
    # launched while some conv below it is unfrozen: with convs.3 the lowest unfrozen one that is l = 4, 5, two levels.
    passes, levels = 4, 5 - (max(frozen) + 1)
    assert levels == 2
    assert D.LAUNCHES["msd_gconv_dgrad"] == levels * passes
    assert D.LAUNCHES["msd_gconv_wgrad"] == 3 * passes                # convs.3 .. convs.5
    assert D.LAUNCHES["dgrad"] == passes and D.LAUNCHES["wgrad"] == passes        # convs.6 alone: convs.0 is frozen
    assert D.LAUNCHES["mpd_conv_post_wgrad"] == passes


def test_repeatable_and_free_of_synchronisation(fx):
    msd = _model(fx["sd"], *fx["narrow"])
    state = {k: v.clone() for k, v in _vectors(msd).items()}
    first = _step(msd, fx["y"], fx["y_hat"], fx["ratios"])          # also warms every lazily initialised piece up
    host_ratios = fx["d"]["len_ratios"].tolist()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            for k, v in _vectors(msd).items():
                v.copy_(state[k])
        second = _step(msd, fx["y"], fx["y_hat"], fx["ratios"])
        msd.generator_losses(fx["y"], fx["y_hat"], host_ratios)     # host ratios travel through pinned memory
        msd.zero_grad(set_to_none=True)
        rs, gs, frs, fgs = msd(fx["y"], fx["y_hat"])
        (rs[0].sum() + fgs[2][3].sum()).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for a, b in zip(first, second):
        assert set(a) == set(b)
        for k in a:
            assert torch.equal(a[k], b[k]), k


def test_len_ratios_none_is_the_plain_means(fx):
    d = fx["d"]
    msd = _model(fx["sd"], *fx["narrow"])
    state = {k: v.clone() for k, v in _vectors(msd).items()}
    want = R.run(fx["sd"], d["y"], d["y_hat"], None)
    want32 = R.run(fx["sd"], d["y"], d["y_hat"], None, torch.float32)
    losses, grads = _step(msd, fx["y"], fx["y_hat"], None)
    _check_losses(fx["name"] + " None", losses, want, _loss_bars(want32, want))
    _check_grads(fx["name"] + " None", grads, want["grad"],
                 {k: max(10 * R.relative_l2(want32["grad"][k], want["grad"][k]), 1e-6) for k in grads})
    with torch.no_grad():
        for k, v in _vectors(msd).items():
            v.copy_(state[k])
    ones = _step(msd, fx["y"], fx["y_hat"], [1.0] * fx["y"].shape[0])[0]          # host ratios of ones
    for k in ("fm", "gen", "disc"):
        assert abs(float(ones[k]) - float(losses[k])) <= 1e-6 * abs(float(losses[k]))


def test_refusals_come_before_any_launch(fx, monkeypatch):
    import rad_mmm_amd.discriminators as D
    from rad_mmm_amd._lib import RadmmmError
    msd = _model(fx["sd"], *fx["narrow"])
    state = {k: v.clone() for k, v in _vectors(msd).items()}
    monkeypatch.setattr(D, "LAUNCHES", {})
    y = torch.zeros(2, 1, 12, device=DEV)
    with pytest.raises(RadmmmError):
        msd(y.cpu(), y.cpu())
    with pytest.raises(ValueError):
        msd(y[:, 0], y[:, 0])
    with pytest.raises(ValueError):
        msd(y, y[:, :, :11])
    with pytest.raises(ValueError, match="len_ratios"):
        msd.generator_losses(y, y, torch.ones(3, device=DEV))
    with pytest.raises(ValueError, match="operand"):
        msd(torch.zeros(8, 1, 1, device=DEV).expand(8, 1, 1 << 22), torch.zeros(8, 1, 1, device=DEV).expand(8, 1, 1 << 22))
    half = _model(fx["sd"], *fx["narrow"])
    half.discriminators[1].half()
    with pytest.raises(RadmmmError, match="fp32 only"):
        half(y, y)
    assert not D.LAUNCHES
    for k, v in _vectors(msd).items():
        assert torch.equal(v, state[k]), k                      # a refused call does not advance the power iteration
    out = msd(torch.rand(1, 1, 1, device=DEV), torch.rand(1, 1, 1, device=DEV))        # the shortest audio: one frame everywhere
    assert tuple(out[0][2].shape) == (1, 1)


def test_reference_widths_against_the_restatement():
    """B = 2, T = 97, len_ratios [1.0, 0.7] at the reference's widths and groups: the bar of every figure is max(10 d, 1e-6)
    with d the deviation of the restatement's own float32 run from its float64 run, measured here.  Nothing is excluded; the
    float32 run carries its sign flips at the kinks and so does the bar.

    The conv_post weight_g of a weight-normed member is ONE number, <dW, v^>, a sum of 3072 terms of both signs whose
    conditioning the inputs decide (tests/test_mpd_gpu.py).  The test takes the first input seed at which the float64
    restatement, alone, shows a condition number below 100 for both; at every passed-over seed those scalars are bounded by
    Cauchy-Schwarz instead (e * ||dW|| / |<dW, v^>| with e the bar of the same conv's weight_v gradient), not dropped.  That
    bound holds at any conditioning, so it is also asserted at the accepted seed: with this weight recipe seed 0 is already
    well conditioned (73 and 24), no seed is passed over, and the bound's code would otherwise never run."""
    sd = R.make_state(*WIDE)
    ratios = torch.tensor([1.0, 0.7])
    msd = _model(sd, *WIDE)
    posts = [f"discriminators.{i}.conv_post." for i in (1, 2)]

    def scalar_terms(w64, pre):
        v = torch.as_tensor(sd[pre + "weight_v"]).double()
        g = torch.as_tensor(sd[pre + "weight_g"]).double().reshape(())
        n = v.norm()
        # dL/dv = g / n (dW - <dW, v^> v^)  ->  dW = n / g dv + <dW, v^> v^, and <dW, v^> is weight_g's gradient
        dg = float(np.asarray(w64["grad"][pre + "weight_g"]).reshape(()))
        dW = torch.as_tensor(w64["grad"][pre + "weight_v"]).double() * (n / g) + dg * v / n
        terms = (dW * v / n).abs().sum()
        return float(terms) / abs(dg), float(dW.norm()) / abs(dg)

    for seed in range(20):
        gen = torch.Generator().manual_seed(seed)
        y, y_hat = torch.rand(2, 1, 97, generator=gen) * 2 - 1, torch.rand(2, 1, 97, generator=gen) * 2 - 1
        w64 = R.run(sd, y, y_hat, ratios, torch.float64)
        w32 = R.run(sd, y, y_hat, ratios, torch.float32)
        conds = [scalar_terms(w64, pre) for pre in posts]
        print(f"wide: input seed {seed}, condition numbers of the conv_post.weight_g gradients {[round(c[0], 1) for c in conds]}")
        msd.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
        losses, grads = _step(msd, y.to(DEV), y_hat.to(DEV), ratios.to(DEV))
        assert set(grads) == set(w64["grad"])
        bars = {k: max(10 * R.relative_l2(w32["grad"][k], w64["grad"][k]), 1e-6) for k in grads}
        well = max(c[0] for c in conds) < 100
        cs = {pre + "weight_g": bars[pre + "weight_v"] * amp for pre, (_, amp) in zip(posts, conds)}
        if not well:
            bars.update(cs)
        _check_losses(f"wide seed {seed}", losses, w64, _loss_bars(w32, w64))
        _check_grads(f"wide seed {seed}", grads, w64["grad"], bars)
        _check_grads(f"wide seed {seed} Cauchy-Schwarz", grads, w64["grad"], cs)      # holds at any conditioning: every seed
        if well:
            break
    else:
        raise AssertionError("no input seed gives well-conditioned conv_post.weight_g gradients")


def test_one_generator_step_with_these_losses(golden):
    """The r1 fixture generator trained one step with fm + gen of this discriminator (narrow widths, the t97 fixture's weights,
    training mode, parameters frozen) on its audio.  The audio gradient leaves through msd_unframe15 and the two
    msd_avgpool_bwd launches and is added across the members before it enters the generator's backward: the generator's
    parameter gradients equal, within max(10 x (f32_vs_f64/<name> + d), 1e-6) relative L2, those of the same HIP generator
    backward fed with the float64 restatement's gradient of the loss at the HIP generator's audio (the scheme of
    tests/test_mpd_gpu.py).

    d is the deviation of the restatement's own float32 audio gradient from its float64 one, measured here on these inputs.
    The kink condition of the fixtures cannot be asked of this audio: the three members hold some 10^5 differences r - g on
    it, the smallest of them a few float32 roundings wide at every one of 40 target seeds tried (ratios 0.0 to 2.4 against the
    factor 8), so as at the reference's widths the float32 runs carry their sign flips and so does the bar.  The target is
    the fixture's own with noise of the seed, of 40, at which the restatement alone (float64 against float32) stays clearest
    of the kinks; the ratios are printed."""
    from _vocoder_ref import load_fixture
    from rad_mmm_amd.vocoder import HiFiGANGenerator
    cfg, gsd = load_fixture(golden("vocoder_gen_r1.npz"))
    d = golden("vocoder_gen_bwd_r1.npz")
    dm = golden("msd_t97.npz")
    narrow = (tuple(int(c) for c in dm["widths"]), tuple(int(g) for g in dm["groups"]))
    lens = d["lens"].tolist()
    gen = HiFiGANGenerator(cfg)
    gen.load_state_dict(gsd)
    gen = gen.to(DEV).train()
    mel = torch.from_numpy(d["mel"]).to(DEV)
    hop = int(np.prod(cfg["upsample_rates"]))
    T = mel.shape[2] * hop
    ratios = (np.asarray(lens, dtype=np.float32) * np.float32(hop) / np.float32(T)).astype(np.float32)
    msd = _model(_sd(dm), *narrow)
    for p in msd.parameters():
        p.requires_grad_(False)
    with torch.no_grad():
        audio0 = gen(mel, lens).cpu().numpy()
    def target_of(seed):
        t = d["target"] + (0.1 * np.random.RandomState(seed).randn(*d["target"].shape).astype(np.float32) if seed else 0)
        t = t.astype(np.float32)
        for b, n in enumerate(lens):
            t[b, n * hop:] = 0
        return t

    best = (-1.0, 0)
    for seed in range(40):
        ki, kd = R.kink_ratios(_sd(dm), target_of(seed)[:, None, :], audio0, torch.from_numpy(ratios))
        best = max(best, (min(ki, kd), -seed))
        if min(ki, kd) > R.KINK_FACTOR:
            break
    target = target_of(-best[1])
    print(f"generator step: target seed {-best[1]}, smaller kink ratio {best[0]:.2f}")
    want = R.run(_sd(dm), target[:, None, :], audio0, torch.from_numpy(ratios), w_fm=1.0, w_gen=1.0, w_disc=0.0)
    want32 = R.run(_sd(dm), target[:, None, :], audio0, torch.from_numpy(ratios), torch.float32, w_fm=1.0, w_gen=1.0, w_disc=0.0)
    gen.zero_grad(set_to_none=True)
    audio = gen(mel, lens)
    assert np.array_equal(audio.detach().cpu().numpy(), audio0)
    fm, g_loss = msd.generator_losses(_dev(target)[:, None, :], audio, _dev(ratios))
    (fm + g_loss).backward()
    got = {k: p.grad.clone() for k, p in gen.named_parameters()}
    gen.zero_grad(set_to_none=True)
    audio = gen(mel, lens)
    audio.backward(_dev(want["grad"]["y_hat"]))
    ref = {k: p.grad.cpu().numpy() for k, p in gen.named_parameters()}
    for k, w in (("fm", fm), ("gen", g_loss)):
        assert abs(float(w.detach()) - want[k]) <= 1e-5 * abs(want[k]), k
    audio_dev = R.relative_l2(want32["grad"]["y_hat"], want["grad"]["y_hat"])
    print(f"generator step: the restatement's float32 audio gradient deviates by {audio_dev:.3e}")
    bars = {k: max(10 * (float(d["f32_vs_f64/" + k]) + audio_dev), 1e-6) for k in got}
    _check_grads("generator step", got, ref, bars)
