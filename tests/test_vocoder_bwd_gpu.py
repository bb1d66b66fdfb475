"""GPU checks of HiFi-GAN generator training (rad_mmm_amd/vocoder.py: HiFiGANGenerator.forward in training mode,
_GeneratorFn; csrc/vocoder_bwd.hip): the gradients against the reference's own (tests/golden/vocoder_gen_bwd_r*.npz)
and against the float64 restatement, the forward's bits, raggedness, repeatability, the absence of device -> host
synchronisation, three Adam steps and a V1-width step.

Bars.  A gradient's bar is max(10 * f32_vs_f64/<name>, 1e-6) relative L2, the rule of tests/test_waveglow_bwd_gpu.py:
ten times what the reference's own float32 run deviates from its float64 run on that gradient.  The loss's bar is
max(10 * |loss32 - loss64|, 1e-6).  After remove_weight_norm() the folded weight of a conv has no stored deviation of
its own: it takes the larger of its weight_g's and weight_v's (the two gradients autograd derives from it).  Every
comparison prints measured over bar (pytest -s)."""
import numpy as np
import pytest
import torch

import _vocoder_bwd_ref as K
from _vocoder_ref import V1, load_fixture, random_state

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _gen(cfg, sd, plain=False):
    from rad_mmm_amd.vocoder import HiFiGANGenerator
    g = HiFiGANGenerator(cfg)
    g.load_state_dict(sd)
    if plain:
        g.remove_weight_norm()
    return g.to(DEV).train()


def _mask(lens, T, hop):
    return (torch.arange(T * hop)[None, :] < torch.tensor(lens)[:, None] * hop).to(DEV)


def _loss(gen, mel, lens, target, mask):
    """the fixtures' loss: the squared error over the valid samples / their number, accumulated in float64"""
    y = gen(mel, lens)[:, 0].double()
    return (((y - target.double()) * mask) ** 2).sum() / mask.sum()


def _grads(gen):
    return {k: p.grad.clone() for k, p in gen.named_parameters()}


def _same_bits(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


def _backward(gen, mel, lens, G):
    """one forward + backward with the incoming gradient G: -> (audio, parameter gradients, mel's gradient or None)"""
    gen.zero_grad(set_to_none=True)
    mel = mel.detach().clone().requires_grad_(mel.requires_grad)
    y = gen(mel, lens)
    y.backward(G)
    return y.detach(), _grads(gen), mel.grad


@pytest.fixture(scope="module", params=["r1", "r2"])
def fx(request, golden):
    name = request.param
    cfg, sd = load_fixture(golden(f"vocoder_gen_{name}.npz"))
    d = golden(f"vocoder_gen_bwd_{name}.npz")
    lens = d["lens"].tolist()
    hop = int(np.prod(cfg["upsample_rates"]))
    mel = torch.from_numpy(d["mel"]).to(DEV)
    target = torch.from_numpy(d["target"]).to(DEV)
    return dict(name=name, cfg=cfg, sd=sd, d=d, lens=lens, hop=hop, mel=mel, target=target,
                mask=_mask(lens, mel.shape[2], hop))


def _check(what, got, want, bars):
    worst, bad = 0.0, []
    for k in sorted(bars):
        err = K.rel_l2(got[k].detach().cpu().numpy(), np.asarray(want[k]))
        worst = max(worst, err / bars[k])
        print(f"{what} {k}: relative L2 {err:.3e} = {err / bars[k]:.3f} of its bar {bars[k]:.3e}")
        if not err <= bars[k]:
            bad.append((k, err, bars[k]))
    print(f"{what}: worst measured / bar {worst:.3f}")
    assert not bad, bad


def _loss_bar(d):
    return max(10 * abs(float(d["loss32"]) - float(d["loss64"])), 1e-6)


def test_gradients_match_the_reference_fixture(fx):
    """weight norm on, as a training checkpoint: the loss and every gradient against the reference's float64 run.
    Fails without the feature: the audio has no grad_fn there."""
    d = fx["d"]
    gen = _gen(fx["cfg"], fx["sd"])
    mel = fx["mel"].clone().requires_grad_(True)
    loss = _loss(gen, mel, fx["lens"], fx["target"], fx["mask"])
    assert loss.grad_fn is not None
    loss.backward()
    loss = loss.detach()
    bar = _loss_bar(d)
    print(f"{fx['name']}: loss {float(loss):.9f}, {abs(float(loss) - float(d['loss64'])):.3e} from the reference's "
          f"float64 (bar {bar:.3e})")
    assert abs(float(loss) - float(d["loss64"])) <= bar
    got = _grads(gen)
    got["mel"] = mel.grad
    names = [k[5:] for k in d if k.startswith("grad/")]
    assert set(names) == set(got)
    bars = {k: max(10 * float(d["f32_vs_f64/" + k]), 1e-6) for k in names}
    _check(fx["name"], got, {k: d["grad/" + k] for k in names}, bars)
    for b, n in enumerate(fx["lens"]):
        assert not mel.grad[b, :, n:].any()


def test_plain_weight_gradients_match_the_restatement(fx):
    """after remove_weight_norm(): against the float64 restatement's gradients of the folded weights"""
    d = fx["d"]
    gen = _gen(fx["cfg"], fx["sd"], plain=True)
    assert not any(k.endswith("weight_g") for k, _ in gen.named_parameters())
    ref_loss, ref = K.restatement_step(fx["cfg"], fx["sd"], fx["mel"].cpu(), fx["lens"], fx["target"].cpu(), plain=True)
    mel = fx["mel"].clone().requires_grad_(True)
    loss = _loss(gen, mel, fx["lens"], fx["target"], fx["mask"])
    loss.backward()
    loss = loss.detach()
    assert abs(float(loss) - float(ref_loss)) <= _loss_bar(d)
    got = _grads(gen)
    got["mel"] = mel.grad
    assert set(got) == set(ref)
    dev = lambda k: float(d["f32_vs_f64/" + k])
    bars = {}
    for k in ref:
        if k.endswith(".weight"):
            bars[k] = max(10 * max(dev(k + "_g"), dev(k + "_v")), 1e-6)
        else:
            bars[k] = max(10 * dev(k), 1e-6)
    _check(fx["name"] + " plain", got, {k: v.numpy() for k, v in ref.items()}, bars)


def test_forward_is_unchanged(fx):
    gen = _gen(fx["cfg"], fx["sd"])
    y_train = gen(fx["mel"], fx["lens"])
    assert y_train.grad_fn is not None and y_train.requires_grad
    with torch.no_grad():
        assert gen(fx["mel"], fx["lens"]).grad_fn is None
    gen.eval()
    y_eval = gen(fx["mel"], fx["lens"])
    assert y_eval.grad_fn is None and not y_eval.requires_grad
    assert torch.equal(y_train.detach(), y_eval)
    gen.train()
    for p in gen.parameters():
        p.requires_grad_(False)
    assert gen(fx["mel"], fx["lens"]).grad_fn is None           # nothing asks for a gradient
    y_mel = gen(fx["mel"].clone().requires_grad_(True), fx["lens"])
    assert y_mel.grad_fn is not None and torch.equal(y_mel.detach(), y_eval)


def test_ragged_batch_repeatability_and_nan_past_the_lengths(fx):
    gen = _gen(fx["cfg"], fx["sd"])
    lens, hop = fx["lens"], fx["hop"]
    B, _, T = fx["mel"].shape
    G = torch.randn(B, 1, T * hop, generator=torch.Generator().manual_seed(3)).to(DEV)
    mel = fx["mel"].clone().requires_grad_(True)
    y, grads, gm = _backward(gen, mel, lens, G)
    # item b of the batch behaves as a call with item b alone at T = lens[b]
    total, gm_items = None, torch.zeros_like(gm)
    for b, n in enumerate(lens):
        yb, gb, gmb = _backward(gen, mel[b:b + 1, :, :n], None, G[b:b + 1, :, :n * hop])
        assert torch.equal(yb[0, 0], y[b, 0, :n * hop])
        total = gb if total is None else {k: total[k] + gb[k] for k in gb}
        gm_items[b, :, :n] = gmb[0]
    worst = 0.0
    for k in sorted(grads):
        err = K.rel_l2(grads[k].cpu().numpy(), total[k].cpu().numpy())
        worst = max(worst, err)
        assert err <= 1e-6, (k, err)
    err = K.rel_l2(gm.cpu().numpy(), gm_items.cpu().numpy())
    print(f"{fx['name']}: batch against the sum of single-item calls: worst relative L2 {max(worst, err):.3e} (bar 1e-6)")
    assert err <= 1e-6
    for b, n in enumerate(lens):                                  # gradient rows at or past a length are exactly 0
        assert not gm[b, :, n:].any()
    y2, again, gm2 = _backward(gen, mel, lens, G)                 # two steps: the same bits
    assert torch.equal(y, y2) and _same_bits(grads, again) and torch.equal(gm, gm2)
    y3, dev, gm3 = _backward(gen, mel, torch.tensor(lens, device=DEV), G)      # device lengths: the same bits
    assert torch.equal(y, y3) and _same_bits(grads, dev) and torch.equal(gm, gm3)
    mel_nan, G_nan = mel.detach().clone(), G.clone()             # what lies past a length reaches nothing
    for b, n in enumerate(lens):
        mel_nan[b, :, n:] = float("nan")
        G_nan[b, :, n * hop:] = float("nan")
    y4, nan, gm4 = _backward(gen, mel_nan.requires_grad_(True), lens, G_nan)
    assert torch.equal(y, y4) and _same_bits(grads, nan) and torch.equal(gm, gm4)


def test_a_step_with_host_lengths_never_waits_for_the_device(fx):
    gen = _gen(fx["cfg"], fx["sd"])

    def step():
        gen.zero_grad(set_to_none=True)
        y = gen(fx["mel"], fx["lens"])
        (y * y).sum().backward()
        with torch.no_grad():                                     # as an optimizer does: the next step folds again
            for p in gen.parameters():
                p.mul_(1.0)
    step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(p.grad is not None for p in gen.parameters())


def test_three_adam_steps_follow_the_restatement(fx):
    d = fx["d"]
    want = K.restatement_adam(fx["cfg"], fx["sd"], fx["mel"].cpu(), fx["lens"], fx["target"].cpu(), 3, 1e-3)

    def run():
        gen = _gen(fx["cfg"], fx["sd"])
        opt = torch.optim.Adam(gen.parameters(), lr=1e-3)
        losses = []
        for _ in range(3):
            opt.zero_grad()
            loss = _loss(gen, fx["mel"], fx["lens"], fx["target"], fx["mask"])
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        return losses, {k: p.detach().clone() for k, p in gen.named_parameters()}
    losses, params = run()
    bar = 10 * _loss_bar(d)
    for i, (a, b) in enumerate(zip(losses, want)):
        print(f"{fx['name']} Adam step {i}: loss {a:.9f}, {abs(a - b):.3e} from the restatement's {b:.9f} (bar {bar:.3e})")
        assert abs(a - b) <= bar
    assert losses[2] < losses[1] < losses[0]
    losses2, params2 = run()
    assert losses == losses2 and _same_bits(params, params2)


def test_v1_widths_step():
    """B = 1, 2 frames, the full V1 widths (512 .. 32 channels, kernels 3 / 7 / 11): every gradient finite and not
    zero, and two steps give the same bits.  No parity gate at this size: about a million leaky-relu inputs make a sign
    disagreement with float64 likely (the kernels are held to their bars at these widths in
    tests/test_hip_vocoder_bwd_direct.py and tests/test_hip_gemm_direct.py); the relative L2 against the float64
    restatement and the number of inputs inside the fixtures' kink margin are printed as a record."""
    import torch.nn.functional as F
    from rad_mmm_amd.vocoder import HiFiGANGenerator
    gen = HiFiGANGenerator(V1)
    sd = random_state(gen, 7)
    gen.load_state_dict(sd)
    gen = gen.to(DEV).train()
    gsrc = torch.Generator().manual_seed(8)
    mel = torch.randn(1, 80, 2, generator=gsrc) - 2.0
    target = torch.rand(1, 2 * gen.hop, generator=gsrc) * 2 - 1
    mask = _mask([2], 2, gen.hop)

    def step():
        gen.zero_grad(set_to_none=True)
        x = mel.to(DEV).requires_grad_(True)
        _loss(gen, x, [2], target.to(DEV), mask).backward()
        g = _grads(gen)
        g["mel"] = x.grad
        return g
    grads = step()
    for k, v in grads.items():
        assert bool(torch.isfinite(v).all()) and bool(v.any()), k
    assert _same_bits(grads, step())
    seen, stock = [], F.leaky_relu

    def recording(x, *a, **k):
        seen.append(x.detach().abs().reshape(-1))
        return stock(x, *a, **k)
    F.leaky_relu = recording
    try:
        _, ref = K.restatement_step(V1, sd, mel, [2], target)
    finally:
        F.leaky_relu = stock
    margin = 8 * 1.5e-6                                           # 8 x the float32 deviation the fixtures recorded
    inside = int(sum(int((s < margin).sum()) for s in seen))
    errs = {k: K.rel_l2(grads[k].cpu().numpy(), ref[k].numpy()) for k in ref}
    worst = max(errs, key=errs.get)
    print(f"V1 widths, 2 frames: {sum(s.numel() for s in seen)} leaky-relu inputs, {inside} inside the kink margin "
          f"{margin:.1e}; relative L2 against the float64 restatement: median {np.median(list(errs.values())):.3e}, worst "
          f"{errs[worst]:.3e} ({worst}) -- a record, not a gate")
