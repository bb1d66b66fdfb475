"""GPU checks of HiFi-GAN's precision "f16" (rad_mmm_amd/vocoder.py): the audio against the float64 emulation of the mode
(tests/_vocoder_f16_ref.generator_f16_ref) by the rule of tests/test_waveglow_half_gpu.py, the properties every mode keeps
(zero tails, repeatable bits, device lengths, NaN past the lengths, no synchronisation), and that the fp32 mode and the
training step are untouched by the switch."""
import numpy as np
import pytest
import torch

from _vocoder_f16_ref import case, rel_l2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = ["r1", "r1_wide", "v1_stage"]          # the r1 fixture (mixed plan), r1's shape at width 64 (all f16), one V1-width stage


def _gen(c):
    from rad_mmm_amd.vocoder import HiFiGANGenerator
    g = HiFiGANGenerator(c["cfg"])
    g.load_state_dict(c["sd"])
    return g.to(DEV).eval()


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(name):
        if name not in cache:
            c = case(name)
            cache[name] = (c, _gen(c), c["mel"].to(DEV))
        return cache[name]
    return get


@pytest.mark.parametrize("name", NAMES)
def test_f16_error_is_the_emulations(models, name):
    """per item the rel-L2 error of the HIP audio against the exact float64 restatement lies within a factor 3 of the
    emulation's, both ways; in batch against alone within 3 x the emulation's error; samples past each length exactly 0"""
    c, gen, mel = models(name)
    assert [m for m, _ in gen.precision_plan("f16")] == c["plan"]
    y = gen(mel, c["lens"], precision="f16")[:, 0].cpu().double()
    hop = gen.hop
    for b, n in enumerate(c["lens"]):
        ref, emu = c["refs"][b]["exact"], c["refs"][b]["f16"]
        e_emu, e_hip = rel_l2(emu, ref), rel_l2(y[b, :n * hop], ref)
        alone = gen(mel[b:b + 1, :, :n], [n], precision="f16")[0, 0].cpu().double()
        e_alone = rel_l2(y[b, :n * hop], alone)
        print(f"f16 {name} item {b} ({n} frames): rel-L2 against exact: HIP {e_hip:.3e}, emulation {e_emu:.3e} (ratio "
              f"{e_hip / e_emu:.2f}); in batch against alone {e_alone:.3e}")
        assert e_emu / 3.0 <= e_hip <= 3.0 * e_emu
        assert e_alone <= 3.0 * e_emu
        assert not y[b, n * hop:].any()


@pytest.mark.parametrize("name", ["r1", "r1_wide"])
def test_bits_are_repeatable_and_lengths_and_nan_do_not_matter(models, name):
    c, gen, mel = models(name)
    lens, hop = c["lens"], gen.hop
    y = gen(mel, lens, precision="f16")
    assert torch.equal(gen(mel, lens, precision="f16"), y)                       # two identical calls
    assert torch.isfinite(y).all()
    for b, n in enumerate(lens):
        assert not y[b, 0, n * hop:].any() and y[b, 0, :n * hop].abs().max() > 0
    dl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    assert torch.equal(gen(mel, dl, precision="f16"), y)                         # device lengths
    poisoned = mel.clone()
    for b, n in enumerate(lens):
        poisoned[b, :, n:] = float("nan")
    assert torch.equal(gen(poisoned, lens, precision="f16"), y)                  # NaN in mel past the lengths
    fp32 = gen(mel, lens)
    assert not torch.equal(fp32, y)                                              # the mode is not the fp32 path
    gen.precision = "f16"                                                        # the attribute is a call's default
    try:
        assert torch.equal(gen(mel, lens), y)
        assert torch.equal(gen(mel, lens, precision="fp32"), fp32)
    finally:
        gen.precision = "fp32"
    assert torch.equal(gen(mel, lens), fp32)                                     # switched back: fp32's bits
    assert torch.equal(_gen(c)(mel, lens), fp32)                                 # ... those of a model that never left it


def test_fp32_and_the_training_step_ignore_the_switch(models):
    """eval-mode fp32 audio, and a training step's audio and gradients with precision = "f16" set, are bit for bit those
    of a model whose attribute was never touched"""
    c, _, mel = models("r1_wide")
    lens = c["lens"]
    plain, switched = _gen(c), _gen(c)
    switched.precision = "f16"
    assert torch.equal(switched(mel, lens, precision="fp32"), plain(mel, lens))
    g_audio = torch.randn(len(lens), 1, mel.shape[2] * plain.hop, generator=torch.Generator().manual_seed(5)).to(DEV)
    out = []
    for m in (plain, switched):
        m.train()
        x = mel.clone().requires_grad_(True)
        y = m(x, lens)
        assert y.grad_fn is not None
        y.backward(g_audio)
        out.append((y.detach(), x.grad, [p.grad for p in m.parameters()]))
        m.eval()
    (y0, gx0, gp0), (y1, gx1, gp1) = out
    assert torch.equal(y0, y1) and torch.equal(gx0, gx1)
    assert torch.equal(y0, plain(mel, lens))                                     # the step's audio is eval fp32's
    assert len(gp0) == len(gp1) and all(torch.equal(a, b) for a, b in zip(gp0, gp1))
    assert not torch.equal(switched(mel, lens), y0)                              # while eval mode follows the attribute


def test_no_sync_and_vocode_mels_returns_the_f16_audio(models):
    from rad_mmm_amd.common import SequenceLength
    from rad_mmm_amd.tts_step import TTSTrainingStep
    from rad_mmm_amd.vocoder import vocode
    c, _, _ = models("r1_wide")
    gen = _gen(c)
    hop = gen.hop
    lens = [40, 25]
    mels = (torch.randn(2, 80, 40, generator=torch.Generator().manual_seed(3)) - 2.0).to(DEV)
    want32, _ = vocode(gen, None, mels, lens, normalize=False)
    want16, _ = vocode(gen, None, mels, lens, normalize=False, precision="f16")       # warm: both weight sets made
    assert not torch.equal(want16, want32)
    assert torch.equal(want16, gen(mels, lens, precision="f16")[:, 0])
    gen.precision = "f16"
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                          # no device -> host synchronisation with host lengths
    try:
        audio, s_lens = vocode(gen, None, mels, lens, normalize=False)
        y = gen(mels, lens)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert s_lens.tolist() == [40 * hop, 25 * hop] and not s_lens.is_cuda
    assert torch.equal(audio, want16) and torch.equal(y[:, 0], want16)
    step = TTSTrainingStep.__new__(TTSTrainingStep)                  # vocode_mels uses nothing of the training modules
    torch.nn.Module.__init__(step)
    step.synth_vocoder = (gen, None)
    ln = torch.tensor(lens)
    got = step.vocode_mels(mels, SequenceLength(ln.to(DEV), ln), normalize=False)
    for b, n in enumerate(lens):
        assert np.array_equal(got[b], want16[b, :n * hop].cpu().numpy())
    gen.precision = "fp32"
    got = step.vocode_mels(mels, SequenceLength(ln.to(DEV), ln), normalize=False)
    assert np.array_equal(got[0], want32[0, :lens[0] * hop].cpu().numpy())
