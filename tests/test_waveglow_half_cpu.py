"""CPU checks of WaveGlow's 16-bit GEMM modes (rad_mmm_amd/waveglow.py `precision`): the fp64 emulation the GPU tests
rest on (tests/_waveglow_half_ref.py) against the plain fp64 restatement, and the public switch's argument checks, which
run before the device check and before any launch."""
import pytest
import torch

from _waveglow_ref import HOP, TINY, infer_ref, load_fixture, random_state
from _waveglow_half_ref import W_SCALE, infer_half_ref, item_refs, rel_l2, shipped_case


def _tiny_items(golden):
    d = golden("waveglow_tiny.npz")
    cfg, sd = load_fixture(d)
    mel = torch.from_numpy(d["mel"])
    noise = [torch.from_numpy(d[f"noise{i}"]) for i in range(3)]
    per = HOP // cfg["n_group"]
    for b, n in enumerate(d["lens"].tolist()):
        yield cfg, sd, mel[b:b + 1, :, :n], float(d["sigma"]), [z[b:b + 1, :, :n * per] for z in noise]


def test_exact_mode_is_the_plain_restatement(golden):
    for cfg, sd, mel, sigma, noise in _tiny_items(golden):
        ref = infer_ref(sd, cfg, mel, sigma, noise)
        got = infer_half_ref(sd, cfg, mel, sigma, noise, "exact")
        assert torch.equal(got, ref)


def test_emulated_modes_on_the_tiny_fixture_are_ordered(golden):
    # h3 is fp32-class, f16 carries the 2^-11 operand rounding: the emulation must show both, or it emulates nothing
    for cfg, sd, mel, sigma, noise in _tiny_items(golden):
        ref = infer_ref(sd, cfg, mel, sigma, noise)
        e3 = rel_l2(infer_half_ref(sd, cfg, mel, sigma, noise, "h3"), ref)
        e1 = rel_l2(infer_half_ref(sd, cfg, mel, sigma, noise, "f16"), ref)
        print(f"tiny item ({mel.shape[2]} frames): rel-L2 of the emulation: h3 {e3:.3e}, f16 {e1:.3e}")
        assert 0.0 < e3 < 1e-5 < e1 < 1e-2


def test_h3_emulation_meets_the_fp32_bars_at_the_shipped_wn_size():
    cfg, sd, mel, lens, noise, sigma = shipped_case()
    for b, r in enumerate(item_refs(sd, cfg, mel, lens, noise, sigma, ("exact", "h3", "f16"))):
        diff = r["h3"] - r["exact"]
        mx, rel = diff.abs().max().item(), (diff.norm() / r["exact"].norm()).item()
        print(f"shipped WN size item {b}: h3 emulation max-abs {mx:.3e} rel-L2 {rel:.3e}; f16 emulation rel-L2 "
              f"{rel_l2(r['f16'], r['exact']):.3e}")
        assert mx <= 1e-4 and rel <= 1e-5


def test_the_scale_of_the_emulation_is_the_packages():
    from rad_mmm_amd import ops
    assert ops.W_SCALE == W_SCALE and ops.NPROD["h3"] == 3 and ops.NPROD["f16"] == 1


def _model(cfg, seed=3):
    from rad_mmm_amd.waveglow import WaveGlow
    m = WaveGlow(**cfg)
    m.load_state_dict(random_state(cfg, seed))
    return m.eval()


def test_default_precision_is_fp32():
    from rad_mmm_amd._lib import RadmmmError
    from rad_mmm_amd.waveglow import PRECISIONS
    m = _model(dict(TINY, n_flows=2))
    assert m.precision == "fp32" and PRECISIONS == ("fp32", "h3", "f16")
    for mode in (None, "fp32", "h3", "f16"):            # a valid mode on a CPU tensor gets as far as the device check
        with pytest.raises(RadmmmError):
            m.infer(torch.zeros(1, 8, 2), precision=mode)


def test_unknown_precision_raises_before_the_device_check():
    from rad_mmm_amd.waveglow import vocode_waveglow
    m = _model(dict(TINY, n_flows=2))
    mel = torch.zeros(1, 8, 2)                           # a CPU tensor: the device check would raise RadmmmError
    with pytest.raises(ValueError, match="precision"):
        m.infer(mel, precision="bf16")
    with pytest.raises(ValueError, match="precision"):
        vocode_waveglow(m, None, mel, [2], precision="fp16")
    m.precision = "half"
    with pytest.raises(ValueError, match="precision"):
        m.infer(mel)
    with pytest.raises(ValueError, match="precision"):
        vocode_waveglow(m, None, mel, [2])


@pytest.mark.parametrize("mode", ["h3", "f16"])
def test_half_modes_refuse_a_k_that_is_no_multiple_of_32(golden, mode):
    from rad_mmm_amd.waveglow import WaveGlow, vocode_waveglow
    cfg, _ = load_fixture(golden("waveglow_denoiser.npz"))           # n_channels = 16
    assert cfg["WN_config"]["n_channels"] == 16
    m = WaveGlow(**cfg).eval()
    mel = torch.zeros(1, cfg["n_mel_channels"], 2)
    with pytest.raises(ValueError, match=r"n_channels % 32"):
        m.infer(mel, precision=mode)
    with pytest.raises(ValueError, match=r"n_channels % 32"):
        vocode_waveglow(m, None, mel, [2], precision=mode)
    m.precision = mode
    with pytest.raises(ValueError, match=r"n_channels % 32"):
        m.infer(mel)
    m5 = _model(dict(TINY, n_flows=2, n_mel_channels=5))             # n_mel_channels * n_group = 40
    with pytest.raises(ValueError, match=r"\(n_mel_channels \* n_group\) % 32"):
        m5.infer(torch.zeros(1, 5, 2), precision=mode)


def test_loader_sets_the_precision(tmp_path, golden):
    from rad_mmm_amd.waveglow import load_waveglow_vocoder
    cfg = dict(TINY, n_flows=4)
    path = tmp_path / "wg.pt"
    torch.save({"state_dict": random_state(cfg, 3), "waveglow_config": cfg}, str(path))
    assert load_waveglow_vocoder(str(path), None, device="cpu")[0].precision == "fp32"
    for mode in ("fp32", "h3", "f16"):
        model, den = load_waveglow_vocoder(str(path), None, device="cpu", precision=mode)
        assert model.precision == mode and den.generator is model
    with pytest.raises(ValueError, match="precision"):
        load_waveglow_vocoder(str(path), None, device="cpu", precision="int8")
    cfg16, sd16 = load_fixture(golden("waveglow_denoiser.npz"))
    p16 = tmp_path / "wg16.pt"
    torch.save({"state_dict": sd16, "waveglow_config": cfg16}, str(p16))
    with pytest.raises(ValueError, match=r"n_channels % 32"):
        load_waveglow_vocoder(str(p16), None, device="cpu", precision="h3")
