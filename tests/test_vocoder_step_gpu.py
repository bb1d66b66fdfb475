"""rad_mmm_amd.vocoder_step.HiFiGANTrainingStep on the GPU, narrow models: the generator of vocoder_gen_r2.npz (hop 256),
the discriminators at the widths of make_golden_mpd.py / make_golden_msd.py, the STFT resolutions of
make_golden_stft_loss.py; B = 3 items of 4, 3 and 4 frames (every item above filter_length // 2 = 512 samples, 1024
samples against a largest n_fft of 128).

Step 1's losses equal, bit for bit, the README recipe written out by hand on modules of their own with the same values
(same kernels, same order, the optimizers two FlatAdam as the object owns them; _modules() rebuilds them, spectral-norm
buffers included, because torch cannot deep-copy a module under the old weight_norm hook); the parameters follow float64
torch.optim.AdamW fed the recorded gradients within the optimizer's bars (tests/test_hip_adam_direct.py); two runs give
the same bits; no device -> host synchronisation with host lengths; the G side leaves the discriminators' gradients
alone; end_epoch; the checkpoint pair."""
import json
import os

import numpy as np
import pytest
import torch

import _adam_ref as R
from rad_mmm_amd.optim import FlatAdam
from rad_mmm_amd.vocoder_step import HiFiGANTrainingStep

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MPD_WIDTHS = (4, 8, 16, 16, 16)
MSD_WIDTHS, MSD_GROUPS = (8, 8, 16, 16, 32, 32, 16), (1, 2, 2, 4, 4, 4, 1)
FFT, HOPS, WIN = [64, 128, 32], [12, 24, 5], [40, 100, 16]
LENS, T = [4, 3, 4], 4
STEPS = 3


def _config():
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "vocoder_gen_r2.npz"))
    cfg = json.loads(str(d["config"]))
    sd = {k[3:]: torch.from_numpy(d[k].astype(np.float32)) for k in d.files if k.startswith("sd/")}
    return cfg, sd


def _modules():
    """fresh (generator, mpd, msd, stft_loss, mel_loss) on the device, the same values every call"""
    from rad_mmm_amd.discriminators import MultiPeriodDiscriminator, MultiScaleDiscriminator
    from rad_mmm_amd.mel_loss import MelSpectrogramLoss
    from rad_mmm_amd.stft_loss import MultiResolutionSTFTLoss
    from rad_mmm_amd.vocoder import HiFiGANGenerator
    cfg, sd = _config()
    gen = HiFiGANGenerator(cfg)
    gen.load_state_dict(sd)
    torch.manual_seed(21)
    mpd = MultiPeriodDiscriminator(channels=MPD_WIDTHS)
    msd = MultiScaleDiscriminator(MSD_WIDTHS, MSD_GROUPS)
    return (gen.to(DEV), mpd.to(DEV), msd.to(DEV), MultiResolutionSTFTLoss(FFT, HOPS, WIN).to(DEV),
            MelSpectrogramLoss().to(DEV))


def _batches():
    g = torch.Generator().manual_seed(33)
    out = []
    for _ in range(STEPS + 1):
        mel = (torch.randn(3, 80, T, generator=g) - 2.0).to(DEV)
        audio = torch.rand(3, 1, T * 256, generator=g) - 0.5
        for b, n in enumerate(LENS):
            audio[b, :, n * 256:] = 0.0
        out.append((mel, audio.to(DEV)))
    return out


def _step_object(mods=None, **kw):
    gen, mpd, msd, stft_loss, mel_loss = mods if mods is not None else _modules()
    return HiFiGANTrainingStep(gen, mpd, msd, stft_loss=stft_loss, mel_loss=mel_loss, **kw)


def _state(step):
    return {f"{n}.{k}": v.detach().clone() for n, m in (("g", step.generator), ("mpd", step.mpd), ("msd", step.msd))
            for k, v in m.state_dict().items()}


def _same(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


def _record(opt, log):
    """wrap opt.step: log (parameters before, gradients, parameters after) of every call"""
    inner = opt.step

    def step(*a, **k):
        before = [p.detach().clone() for p in opt._order]
        grads = [torch.zeros_like(p) if p.grad is None else p.grad.detach().clone() for p in opt._order]
        inner(*a, **k)
        log.append((before, grads, [p.detach().clone() for p in opt._order]))
    opt.step = step


@pytest.fixture(scope="module")
def run():
    """three recorded steps of one object: (object, batches, per-step losses, the two optimizers' logs, initial modules)"""
    initial = _modules()
    step = _step_object(_modules())
    logs = {"g": [], "d": []}
    _record(step.optim_g, logs["g"])
    _record(step.optim_d, logs["d"])
    batches = _batches()
    losses = [step.training_step(mel, LENS, audio) for mel, audio in batches[:STEPS]]
    return step, batches, losses, logs, initial


def test_step_one_is_the_readme_recipe_bit_for_bit(run):
    _, batches, losses, _, initial = run
    gen, mpd, msd, loss_fn, mel_loss = _modules()
    for mine, theirs in zip((gen, mpd, msd), initial):           # the same start, spectral-norm buffers included
        a, b = mine.state_dict(), theirs.state_dict()
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    gen.train(), mpd.train(), msd.train()
    kw = dict(lr=2e-4, betas=(0.8, 0.99), weight_decay=0.01, decoupled=True)
    opt_g = FlatAdam(gen.named_parameters(), **kw)
    opt_d = FlatAdam([(f"mpd.{n}", p) for n, p in mpd.named_parameters()] + [(f"msd.{n}", p) for n, p in msd.named_parameters()],
                     **kw)
    mel, target = batches[0]
    lens = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    hop = gen.hop
    # the README's lines
    audio = gen(mel, lens)
    ratios = lens / lens.max()
    opt_d.zero_grad()
    loss_p, _, _ = mpd.discriminator_loss(target, audio.detach(), ratios)
    loss_s, _, _ = msd.discriminator_loss(target, audio.detach(), ratios)
    (loss_p + loss_s).backward()
    opt_d.step()
    opt_g.zero_grad()
    for p in list(mpd.parameters()) + list(msd.parameters()):
        p.requires_grad_(False)
    fm_p, gen_p = mpd.generator_losses(target, audio, ratios)
    fm_s, gen_s = msd.generator_losses(target, audio, ratios)
    sc, mag = loss_fn(audio[:, 0], target[:, 0], ratios)
    l_mel = mel_loss(audio[:, 0], mel, lens * hop, lens)
    total = 45.0 * l_mel + fm_p + fm_s + gen_p + gen_s + sc + mag
    total.backward()
    opt_g.step()
    want = {"d_mpd": loss_p, "d_msd": loss_s, "d_total": loss_p + loss_s, "mel": l_mel, "fm_mpd": fm_p, "fm_msd": fm_s,
            "gen_mpd": gen_p, "gen_msd": gen_s, "sc": sc, "mag": mag, "g_total": total}
    got = losses[0]
    assert set(got) == set(want)
    for k, v in want.items():
        assert got[k].is_cuda and got[k].dim() == 0 and not got[k].requires_grad, k
        assert torch.isfinite(got[k]), k
        assert torch.equal(got[k], v.detach()), (k, float(got[k]), float(v))


def test_parameters_follow_float64_adamw_on_the_recorded_gradients(run):
    step, _, _, logs, _ = run
    for name, log in logs.items():
        assert len(log) == STEPS
        ref = [torch.nn.Parameter(p.double().cpu()) for p in log[0][0]]
        topt = torch.optim.AdamW(ref, lr=2e-4, betas=(0.8, 0.99), weight_decay=0.01)
        worst = 0.0
        for k, (before, grads, after) in enumerate(log):
            if k:
                assert all(torch.equal(a, b) for a, b in zip(log[k - 1][2], before)), (name, k)     # nothing else wrote them
            assert all(bool(torch.isfinite(g).all()) for g in grads) and any(bool(g.any()) for g in grads)
            for q, g in zip(ref, grads):
                q.grad = g.double().cpu()
            topt.step()
            for i, (q, a) in enumerate(zip(ref, after)):
                got, want = a.cpu().numpy(), q.detach().numpy()
                worst = max(worst, R.worst_over_bar(got, want, k + 1))
                assert R.within_bar(got, want, k + 1), (name, k, i, R.worst_over_bar(got, want, k + 1))
        print(f"optimizer {name}: worst measured / bar over {STEPS} steps {worst:.3g}")
    assert step.steps == STEPS and step.optim_g.step_count == STEPS and step.optim_d.step_count == STEPS


def test_two_runs_from_the_same_state_end_in_the_same_bits(run):
    step, batches, losses, _, initial = run
    again = _step_object(_modules())
    for k, (mel, audio) in enumerate(batches[:STEPS]):
        out = again.training_step(mel, LENS, audio)
        assert _same(out, losses[k]), k
    assert _same(_state(again), _state(step))


def test_no_device_to_host_synchronisation_with_host_lengths(run):
    _, batches, _, _, initial = run
    step = _step_object(_modules(), clip=1000.0)
    mel, audio = batches[0]
    step.training_step(mel, LENS, audio)                       # warm
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = step.training_step(mel, LENS, audio)
        val = step.validation_step(mel, LENS, audio)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(bool(torch.isfinite(v)) for v in out.values()) and bool(torch.isfinite(val)) and val.dim() == 0
    assert step.generator.training and step.steps == 2


def test_g_side_gives_the_discriminators_no_gradient_and_restores_the_flags(run):
    _, batches, _, _, initial = run
    step = _step_object(_modules())
    d_params = list(step.mpd.parameters()) + list(step.msd.parameters())
    seen = {}
    d_inner, g_inner = step.optim_d.step, step.optim_g.step

    def d_step(*a, **k):
        d_inner(*a, **k)
        seen["d"] = [p.grad.detach().clone() for p in d_params]

    def g_step(*a, **k):
        seen["same"] = all(torch.equal(p.grad, g) for p, g in zip(d_params, seen["d"]))
        g_inner(*a, **k)

    def mel_loss(*a, **k):                                     # called in the middle of the G side
        seen["flags"] = [p.requires_grad for p in d_params]
        return mel_inner(*a, **k)
    mel_inner, step.mel_loss = step.mel_loss, mel_loss
    step.optim_d.step, step.optim_g.step = d_step, g_step
    mel, audio = batches[0]
    step.training_step(mel, LENS, audio)
    assert seen["same"] and not any(seen["flags"])
    assert all(p.requires_grad for p in d_params)
    assert all(p.grad is not None and bool(p.grad.any()) for p in step.generator.parameters())


def test_end_epoch_scales_both_learning_rates(run):
    _, _, _, _, initial = run
    step = _step_object(_modules(), lr=1e-3, lr_decay=0.5)
    step.end_epoch()
    step.end_epoch()
    assert step.optim_g.lr == 2.5e-4 and step.optim_d.lr == 2.5e-4 and step.epoch == 2


def test_checkpoint_round_trip(run, tmp_path):
    from rad_mmm_amd.discriminators import load_mpd, load_msd
    from rad_mmm_amd.vocoder import load_hifigan_vocoder
    _, batches, _, _, initial = run
    step = _step_object(_modules())
    for mel, audio in batches[:STEPS]:
        step.training_step(mel, LENS, audio)
    step.end_epoch()
    g_path, do_path = step.save_checkpoint(str(tmp_path))
    assert os.path.basename(g_path) == f"g_{STEPS:08d}" and os.path.basename(do_path) == f"do_{STEPS:08d}"
    do = torch.load(do_path, map_location="cpu")
    assert set(do) == {"mpd", "msd", "optim_g", "optim_d", "steps", "epoch"} and do["steps"] == STEPS and do["epoch"] == 1
    assert set(torch.load(g_path, map_location="cpu")) == {"generator"}
    cfg_path = tmp_path / "config.json"
    cfg_path.write_text(json.dumps(_config()[0]))
    gen, _ = load_hifigan_vocoder(g_path, str(cfg_path), DEV)
    mpd = load_mpd(do_path, DEV, channels=MPD_WIDTHS)
    msd = load_msd(do_path, DEV, channels=MSD_WIDTHS, groups=MSD_GROUPS)
    for got, want in ((gen, step.generator), (mpd, step.mpd), (msd, step.msd)):
        a, b = got.state_dict(), want.state_dict()
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    resumed = _step_object(_modules())
    assert resumed.load_checkpoint(str(tmp_path)) == STEPS
    assert resumed.steps == STEPS and resumed.epoch == 1 and resumed.optim_g.lr == step.optim_g.lr
    assert _same(_state(resumed), _state(step))
    mel, audio = batches[STEPS]
    want = step.training_step(mel, LENS, audio)
    got = resumed.training_step(mel, LENS, audio)
    assert _same(got, want) and _same(_state(resumed), _state(step))
    assert resumed.steps == STEPS + 1 and resumed.optim_d.step_count == STEPS + 1
