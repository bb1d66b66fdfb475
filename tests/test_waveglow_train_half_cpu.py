"""CPU checks of WaveGlow's training precision switch (rad_mmm_amd/waveglow.py `train_precision`, `grad_scale`): the
defaults, every argument check (all of them run before the device check and before any launch, on a CPU model), the
independence of `precision` (infer) and `train_precision`, and the automatic gradient scale as a pure function."""
import math

import pytest
import torch

from _waveglow_ref import HOP, TINY


def _model(**over):
    from rad_mmm_amd.waveglow import WaveGlow
    cfg = dict(TINY, **over)
    return WaveGlow(**cfg)                       # training mode, on the CPU


def _batch(m, T=2, B=1):
    return torch.zeros(B, m.n_mel_channels, T), torch.zeros(B, T * HOP)


def test_defaults():
    from rad_mmm_amd.waveglow import TRAIN_PRECISIONS
    m = _model()
    assert TRAIN_PRECISIONS == ("fp32", "h3")
    assert m.train_precision == "fp32" and m.precision == "fp32" and m.grad_scale is None
    assert m.grad_saturated() is False           # no step has run: no flag word, nothing to read


@pytest.mark.parametrize("name", ["f16", "bf16", "H3", ""])
def test_unknown_names_raise_before_the_device_check(name):
    m = _model()
    mel, audio = _batch(m)
    with pytest.raises(ValueError, match="train_precision"):
        m.nll_loss(mel, audio, precision=name)
    m.train_precision = name
    with pytest.raises(ValueError, match="train_precision"):
        m.nll_loss(mel, audio)
    with pytest.raises(ValueError, match="train_precision"):
        m((mel, audio))
    m.eval()                                     # outside a training step the attribute is not looked at,
    with pytest.raises(ValueError, match="train_precision"):
        m.nll_loss(mel, audio, precision=name)   # a name given to the call still is


@pytest.mark.parametrize("over", [dict(WN_config=dict(n_layers=2, n_channels=48, kernel_size=3)),
                                  dict(n_mel_channels=5)])
def test_h3_needs_k_multiples_of_32(over):
    m = _model(**over)
    mel, audio = _batch(m)
    with pytest.raises(ValueError, match="train_precision 'h3' needs n_channels % 32"):
        m.nll_loss(mel, audio, precision="h3")
    m.train_precision = "h3"
    with pytest.raises(ValueError, match="train_precision 'h3' needs n_channels % 32"):
        m((mel, audio))


def test_h3_needs_32_group_steps_per_padded_item():
    # T * 256 / n_group group steps: every n_group this module accepts gives at least 32 per frame, so only an empty
    # batch falls below radmmm_wgrad_rm's K step
    m = _model()
    mel, audio = _batch(m, T=0)
    with pytest.raises(ValueError, match="32 group steps"):
        m.nll_loss(mel, audio, precision="h3")


@pytest.mark.parametrize("bad", [3.0, 0.0, -4.0, float("inf"), float("nan"), 1000])
def test_grad_scale_must_be_a_power_of_two(bad):
    m = _model()
    mel, audio = _batch(m)
    m.grad_scale = bad
    with pytest.raises(ValueError, match="grad_scale"):
        m.nll_loss(mel, audio, precision="h3")
    from rad_mmm_amd._lib import RadmmmError
    m.grad_scale = 2.0 ** -3                     # a power of two passes on to the device check
    with pytest.raises(RadmmmError, match="GPU"):
        m.nll_loss(mel, audio, precision="h3")


def test_valid_modes_reach_the_device_check():
    from rad_mmm_amd._lib import RadmmmError
    m = _model()
    mel, audio = _batch(m)
    for mode in ("fp32", "h3"):
        with pytest.raises(RadmmmError, match="GPU"):
            m.nll_loss(mel, audio, precision=mode)


def test_the_two_switches_do_not_touch_each_other():
    m = _model()
    m.train_precision = "h3"
    assert m.precision == "fp32" and m._precision() == "fp32"
    m.precision = "f16"                          # infer's one-product mode says nothing about training
    assert m.train_precision == "h3" and m._train_precision() == "h3"
    m.train_precision = "fp32"
    assert m.precision == "f16" and m._precision() == "f16" and m._train_precision() == "fp32"


@pytest.mark.parametrize("n", [8192, 190464, 6553600])
def test_automatic_grad_scale_rule(n):
    from rad_mmm_amd.waveglow import auto_grad_scale
    g = auto_grad_scale(n)
    assert math.frexp(g)[0] == 0.5 and 1.0 <= g / n < 2.0
    m = _model()
    assert m._g_scale(n) == g
    m.grad_scale = 64
    assert m._g_scale(n) == 64.0
