"""CPU checks of the WaveGlow path: the fp64 restatement (tests/_waveglow_ref.py) replays the reference's recorded
outputs (tests/golden/waveglow_*.npz), the state_dict formats load to the same tensors, the plain checkpoint format
loads from a file, and the packed polyphase upsample weight equals F.conv_transpose1d."""
import json

import numpy as np
import torch
import torch.nn.functional as F

from _waveglow_ref import (HOP, TINY, UP_KERNEL, bias_spec_ref, denoise_ref, infer_ref, load_fixture, noise_channels,
                           random_state)


def test_fp64_restatement_replays_the_tiny_fixture(golden):
    d = golden("waveglow_tiny.npz")
    cfg, sd = load_fixture(d)
    assert cfg == TINY and float(d["f32_vs_f64"]) <= 1e-5
    mel, sigma = torch.from_numpy(d["mel"]), float(d["sigma"])
    per = HOP // cfg["n_group"]
    assert [d[f"noise{i}"].shape[1] for i in range(3)] == noise_channels(cfg) == [4, 2, 2]
    for b, n in enumerate(d["lens"].tolist()):
        noise = [torch.from_numpy(d[f"noise{i}"][b:b + 1, :, :n * per]) for i in range(3)]
        y = infer_ref(sd, cfg, mel[b:b + 1, :, :n], sigma, noise)[0].numpy()
        err = np.abs(y - d["audio"][b, :n * HOP]).max()
        print(f"item {b}: fp64 restatement vs reference max-abs {err:.3e}")
        assert err <= 1e-6
        assert not d["audio"][b, n * HOP:].any()


def test_fp64_restatement_replays_the_denoiser_fixture(golden):
    d = golden("waveglow_denoiser.npz")
    cfg, sd = load_fixture(d)
    bias = bias_spec_ref(sd, cfg)
    err = (bias - torch.from_numpy(d["bias_spec"]).double()).abs().max().item()
    print(f"bias_spec max-abs {err:.3e} (max {d['bias_spec'].max():.3f})")
    assert err <= 1e-6 * max(1.0, float(d["bias_spec"].max()))
    audio = torch.from_numpy(d["audio"])
    for tag, strength in (("s0p1", 0.1), ("s0p001", 0.001)):
        for b, n in enumerate(d["lens"].tolist()):
            y = denoise_ref(audio[b:b + 1, :n], torch.from_numpy(d["bias_spec"]), strength).numpy()
            ref = d["out_" + tag][b, :y.shape[0]]
            err = np.abs(y - ref).max()
            print(f"denoiser {tag} item {b}: max-abs {err:.3e}")
            assert y.shape[0] == n // HOP * HOP and err <= 1e-6 * max(1.0, np.abs(ref).max())


def test_weight_normed_and_folded_keys_load_to_the_same_tensors(golden):
    from rad_mmm_amd.vocoder import fold_weight_norm
    from rad_mmm_amd.waveglow import WaveGlow, fold_weight_norm_keys
    cfg, sd = load_fixture(golden("waveglow_tiny.npz"))
    assert any(k.endswith("weight_g") for k in sd)
    a = WaveGlow(**cfg)
    a.load_state_dict(sd)                                   # weight_g / weight_v keys
    folded = fold_weight_norm_keys(sd)
    assert not any(k.endswith(("weight_g", "weight_v")) for k in folded)
    assert sorted(folded) == sorted(a.state_dict())         # the names of a reference model after remove_weightnorm
    b = WaveGlow(**cfg)
    b.load_state_dict(folded)
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
    k = "WN.3.in_layers.2"
    assert torch.equal(a.state_dict()[k + ".weight"], fold_weight_norm(sd[k + ".weight_v"], sd[k + ".weight_g"]))
    # the parametrization spelling of weight norm
    para = {}
    for key, v in sd.items():
        key = key.replace(".weight_g", ".parametrizations.weight.original0")
        para[key.replace(".weight_v", ".parametrizations.weight.original1")] = v
    c = WaveGlow(**cfg)
    c.load_state_dict(para)
    assert all(torch.equal(va, vc) for va, vc in zip(a.state_dict().values(), c.state_dict().values()))
    assert a.noise_shapes == noise_channels(cfg)


def test_plain_checkpoint_format_loads_from_a_file(tmp_path):
    from rad_mmm_amd.waveglow import WaveGlow, WaveGlowDenoiser, load_waveglow_vocoder
    cfg = dict(TINY, n_flows=4)
    sd = random_state(cfg, 3)
    path = tmp_path / "waveglow.pt"
    torch.save({"state_dict": sd, "waveglow_config": cfg}, path)
    model, den = load_waveglow_vocoder(str(path), None, device="cpu")
    assert isinstance(model, WaveGlow) and isinstance(den, WaveGlowDenoiser) and not model.training
    assert all(torch.equal(v, sd[k]) for k, v in model.state_dict().items())
    assert dict(den.named_parameters()) == {} and "generator" not in dict(den.named_children())
    # without the embedded config: the reference's config.json layout
    torch.save({"state_dict": sd}, path)
    cj = tmp_path / "config.json"
    cj.write_text(json.dumps({"train_config": {}, "waveglow_config": cfg}))
    model2, _ = load_waveglow_vocoder(str(path), str(cj), device="cpu")
    assert model2.n_flows == 4 and model2.n_remaining_channels == 6


def test_polyphase_upsample_matches_conv_transpose():
    # ConvTranspose1d(k = 1024, stride 256, padding 0) trimmed by k - stride: output group g takes frames g - 3 .. g
    from rad_mmm_amd.vocoder import pack_polyphase
    g = torch.Generator().manual_seed(5)
    n_mel, T = 6, 9
    w = torch.randn(n_mel, n_mel, UP_KERNEL, generator=g, dtype=torch.float64)
    bias = torch.randn(n_mel, generator=g, dtype=torch.float64)
    x = torch.randn(1, n_mel, T, generator=g, dtype=torch.float64)
    ref = F.conv_transpose1d(x, w, bias, stride=HOP)[:, :, :-(UP_KERNEL - HOP)]
    assert ref.shape[2] == T * HOP
    Wp = pack_polyphase(w, HOP, 0, 0, 8)                    # [taps, HOP*n_mel, ldk = 8]
    taps = Wp.shape[0]
    assert taps == 7 and not Wp[4:].any() and not Wp[:, :, n_mel:].any()
    xr = torch.zeros(T + taps - 1, 8, dtype=torch.float64)  # channels-last rows, zero padded by taps // 2 frames
    xr[taps // 2:taps // 2 + T, :n_mel] = x[0].T
    y = torch.zeros(T, HOP * n_mel, dtype=torch.float64)
    for tap in range(taps):
        y += xr[tap:tap + T] @ Wp[tap].T
    y = (y + bias.repeat(HOP)).reshape(T * HOP, n_mel).T
    assert (y - ref[0]).abs().max().item() < 1e-11


class _PickledWaveGlow(torch.nn.Module):
    """stand-in with the attributes load_waveglow_vocoder reads from an unpickled reference module"""

    def __init__(self, cfg, sd):
        super().__init__()
        from rad_mmm_amd.waveglow import WaveGlow
        inner = WaveGlow(**cfg)
        inner.load_state_dict(sd)
        self.upsample, self.WN, self.convinv = inner.upsample, inner.WN, inner.convinv
        self.n_flows, self.n_group = cfg["n_flows"], cfg["n_group"]
        self.n_early_every, self.n_early_size = cfg["n_early_every"], cfg["n_early_size"]


def test_pickled_module_checkpoint_needs_the_callers_consent(tmp_path):
    import pytest
    from rad_mmm_amd.waveglow import config_of_module, load_waveglow_vocoder
    cfg = dict(TINY, n_flows=4)
    sd = random_state(cfg, 4)
    module = _PickledWaveGlow(cfg, sd)
    assert config_of_module(module) == cfg
    path = tmp_path / "waveglow_module.pt"
    torch.save({"model": module}, path)
    with pytest.raises(ValueError, match="allow_pickled_module"):       # the restricted unpickler refuses the class
        load_waveglow_vocoder(str(path), None, device="cpu")
    model, _ = load_waveglow_vocoder(str(path), None, device="cpu", allow_pickled_module=True)
    assert model.n_flows == 4 and model.WN[0].kernel_size == 3
    assert all(torch.equal(v, sd[k]) for k, v in model.state_dict().items())
    model.load_state_dict({**sd}, strict=True, assign=False)            # the keyword nn.Module.load_state_dict takes
