"""CPU checks of the batched HiFi-GAN vocoder (rad_mmm_amd/vocoder.py): the fp64 restatement that the GPU tests use
as their oracle reproduces the reference's outputs (tests/golden/vocoder_*.npz, made by running the reference), the
polyphase packing of a transposed conv, the per-input-channel weight-norm fold, checkpoint key handling, the C ABI
bindings of the new entry points, and the errors raised before any device work."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _vocoder_ref import V1, denoise_ref, generator_ref, load_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["r1", "r2"])
def test_fp64_generator_restatement_matches_reference(golden, name):
    d = golden(f"vocoder_gen_{name}.npz")
    cfg, sd = load_fixture(d)
    mel = torch.from_numpy(d["mel"])
    hop = int(np.prod(cfg["upsample_rates"]))
    for b, n in enumerate(d["lens"].tolist()):
        y = generator_ref(sd, cfg, mel[b:b + 1, :, :n])[0, 0].numpy()
        ref = d["audio"][b, :n * hop]
        assert y.shape == ref.shape
        assert np.abs(y - ref).max() < 2e-5, (name, b, np.abs(y - ref).max())
        assert np.abs(ref).max() > 0.1           # the fixture carries signal


def test_fp64_denoiser_restatement_matches_reference(golden):
    d = golden("vocoder_denoiser.npz")
    audio = torch.from_numpy(d["audio"])
    bias = torch.from_numpy(d["bias_spec"])
    for tag, strength in (("s0p1", 0.1), ("s0p001", 0.001)):
        for b, n in enumerate(d["lens"].tolist()):
            y = denoise_ref(audio[b:b + 1, :n], bias, strength).numpy()
            ref = d["out_" + tag][b, :y.shape[0]]
            assert y.shape[0] == n // 256 * 256
            assert np.abs(y - ref).max() < 1e-5 * max(1.0, np.abs(ref).max()), (tag, b, np.abs(y - ref).max())
            assert not d["out_" + tag][b, y.shape[0]:].any()


def test_denoiser_bias_spectrum_matches_reference(golden):
    from _vocoder_ref import stft_mag_ref
    dg = golden("vocoder_gen_r2.npz")
    cfg, sd = load_fixture(dg)
    audio = generator_ref(sd, cfg, torch.zeros(1, 80, 88))[0]
    mag, _ = stft_mag_ref(audio)
    ref = golden("vocoder_denoiser.npz")["bias_spec"]
    np.testing.assert_allclose(mag[0, :, 0].numpy(), ref, rtol=1e-4, atol=1e-6)


def _packed_conv_transpose(x, w, u, p, off=0):
    """y via the packed polyphase row GEMM (the arithmetic radmmm_rowgemm_f32 performs), channels-first in/out"""
    from rad_mmm_amd.vocoder import pack_polyphase
    Wp = pack_polyphase(w, u, p, off)
    taps, h = Wp.shape[0], Wp.shape[0] // 2
    Cin, Cout, _ = w.shape
    T = x.shape[-1]
    xr = x[0].t()                                             # [T, Cin] rows
    y = torch.zeros(T, u * Cout, dtype=x.dtype)
    for tap in range(taps):
        sh = tap - h
        xs = torch.zeros_like(xr)
        lo, hi = max(0, -sh), min(T, T - sh)
        if hi > lo:
            xs[lo:hi] = xr[lo + sh:hi + sh]
        y += xs @ Wp[tap].t()
    return y.reshape(T * u, Cout).t()[None]


@pytest.mark.parametrize("k,u", [(16, 8), (4, 2), (8, 4), (11, 5), (6, 2), (3, 3)])
def test_polyphase_packing_reproduces_conv_transpose_exactly(k, u):
    g = torch.Generator().manual_seed(k * 31 + u)
    Cin, Cout, T = 5, 3, 9
    # small integers: every product and sum is exact in fp64, so the two orders of summation agree bit for bit
    w = torch.randint(-4, 5, (Cin, Cout, k), generator=g).double()
    x = torch.randint(-4, 5, (1, Cin, T), generator=g).double()
    p = (k - u) // 2
    ref = F.conv_transpose1d(x, w, stride=u, padding=p)
    n = min(ref.shape[-1], T * u)
    y = _packed_conv_transpose(x, w, u, p)
    assert torch.equal(y[..., :n], ref[..., :n])


def test_polyphase_packing_with_output_offset_is_the_trimmed_istft():
    # the inverse STFT: k = 1024, u = 256, p = 0, the first n_fft/2 samples trimmed = an output offset of 2 groups
    g = torch.Generator().manual_seed(3)
    Cin, k, u, T = 6, 1024, 256, 5
    w = torch.randint(-3, 4, (Cin, 1, k), generator=g).double()
    x = torch.randint(-3, 4, (1, Cin, T), generator=g).double()
    ref = F.conv_transpose1d(x, w, stride=u)[..., 512:-512]
    y = _packed_conv_transpose(x, w, u, 0, off=2)
    assert ref.shape[-1] == (T - 1) * u
    assert torch.equal(y[..., :ref.shape[-1]], ref)


def test_convtranspose_weight_norm_fold_is_per_input_channel():
    from rad_mmm_amd.vocoder import fold_weight_norm
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = torch.nn.utils.weight_norm(torch.nn.ConvTranspose1d(8, 4, 16, 8, padding=4))
    with torch.no_grad():
        m.weight_g.uniform_(0.5, 1.5)
        m.weight_v.normal_()
    assert m.weight_g.shape == (8, 1, 1)                      # dim 0 of [Cin, Cout, k]: the INPUT channel
    m(torch.zeros(1, 8, 3))                                   # the pre-forward hook recomputes .weight
    w = fold_weight_norm(m.weight_v.detach(), m.weight_g.detach())
    torch.testing.assert_close(w, m.weight.detach(), rtol=1e-6, atol=1e-7)
    norms = w.reshape(8, -1).norm(dim=1)
    torch.testing.assert_close(norms, m.weight_g.detach().reshape(-1), rtol=1e-5, atol=0)


def test_state_dict_round_trip_and_old_key_remap(golden):
    from rad_mmm_amd.vocoder import HiFiGANGenerator
    d = golden("vocoder_gen_r1.npz")
    assert bool(d["old_keys"])
    cfg, sd = load_fixture(d)
    assert any(re.match(r"resblocks\.\d+\.convs1\.", k) for k in sd)      # the old 5-part format
    gen = HiFiGANGenerator(cfg)
    gen.load_state_dict(sd)
    out = gen.state_dict()
    assert len(out) == len(sd)
    for k, v in sd.items():
        p = k.split(".")
        nk = f"resblocks.{int(p[1]) // 3}.{int(p[1]) % 3}.{'.'.join(p[2:])}" if p[0] == "resblocks" else k
        assert torch.equal(out[nk], v), k
    gen2 = HiFiGANGenerator(cfg)
    gen2.load_state_dict(out)                                  # new-format keys load unchanged
    assert all(torch.equal(a, b) for a, b in zip(gen2.state_dict().values(), out.values()))
    names = set(out)
    for must in ("conv_pre.weight_g", "conv_pre.weight_v", "conv_pre.bias", "ups.0.weight_g", "ups.1.weight_v",
                 "resblocks.1.2.convs1.2.weight_v", "resblocks.0.0.convs2.0.bias", "conv_post.weight_g"):
        assert must in names
    gen2.remove_weight_norm()
    assert "conv_pre.weight" in gen2.state_dict() and "conv_pre.weight_g" not in gen2.state_dict()
    torch.testing.assert_close(gen2.conv_pre.weight.detach(),
                               gen.conv_pre.weight_g.detach() * gen.conv_pre.weight_v.detach()
                               / gen.conv_pre.weight_v.detach().reshape(gen.conv_pre.weight_v.shape[0], -1)
                               .norm(dim=1).reshape(-1, 1, 1))


def test_resblock2_state_dict_names(golden):
    from rad_mmm_amd.vocoder import HiFiGANGenerator
    cfg, sd = load_fixture(golden("vocoder_gen_r2.npz"))
    gen = HiFiGANGenerator(cfg)
    gen.load_state_dict(sd)
    assert set(gen.state_dict()) == set(sd)
    assert "resblocks.2.1.convs.1.weight_v" in sd


def test_v1_work_size_matches_the_issue_arithmetic():
    from rad_mmm_amd.vocoder import HiFiGANGenerator
    gen = HiFiGANGenerator(V1)
    flop = 0.0
    rows = 1
    for i, u in enumerate(V1["upsample_rates"]):
        rows *= u
        for m in gen.resblocks[i].modules():
            if isinstance(m, torch.nn.Conv1d):
                flop += 2 * rows * m.in_channels * m.out_channels * m.kernel_size[0]
    assert 0.58e9 < flop < 0.62e9                              # ~0.59 GFLOP of resblock convs per mel frame


def test_blur_and_cpu_tensors_raise():
    from rad_mmm_amd._lib import RadmmmError
    from rad_mmm_amd.vocoder import Denoiser, HiFiGANGenerator
    cfg = dict(V1, upsample_initial_channel=32, gaussian_blur={"p_blurring": 0.5, "kernel_size": 3, "sigmas": [1.0]})
    with pytest.raises(ValueError, match="p_blurring"):
        HiFiGANGenerator(cfg)
    gen = HiFiGANGenerator(dict(V1, upsample_initial_channel=64))
    with pytest.raises(RadmmmError, match="GPU"):
        gen(torch.zeros(1, 80, 4))
    den = Denoiser(gen)
    with pytest.raises(RadmmmError, match="GPU"):
        den(torch.zeros(1, 2048))
    with pytest.raises(ValueError):
        Denoiser(gen, mode="normal")


def test_new_entry_points_bound_with_the_header_arity():
    import rad_mmm_amd._lib as L
    hdr = open(os.path.join(ROOT, "include", "radmmm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decls = dict(re.findall(r"\bint\s+(radmmm_voc_[a-z_]+)\s*\(([^)]*)\)", hdr))
    assert set(decls) == {"radmmm_voc_lrelu", "radmmm_voc_conv_post", "radmmm_voc_reflect_pad", "radmmm_voc_spec_bins",
                          "radmmm_voc_istft_finish", "radmmm_voc_normalize"}
    for name, args in decls.items():
        fn = getattr(L.lib, name)
        assert len(fn.argtypes) == len(args.split(",")), name
    assert L.lib.radmmm_abi_version() == 4
