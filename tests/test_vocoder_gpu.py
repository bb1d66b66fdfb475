"""GPU checks of the batched HiFi-GAN vocoder (rad_mmm_amd/vocoder.py, csrc/vocoder.hip): the generator and the
denoiser against the reference's outputs (tests/golden/vocoder_*.npz) and against the fp64 restatement at full V1
size, batch invariance, vocode_mels, and the absence of device -> host synchronisation with host lengths."""
import numpy as np
import pytest
import torch

from _vocoder_ref import V1, denoise_ref, generator_ref, load_fixture, random_state, stft_mag_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _gen(cfg, sd):
    from rad_mmm_amd.vocoder import HiFiGANGenerator
    g = HiFiGANGenerator(cfg)
    g.load_state_dict(sd)
    return g.to(DEV).eval()


@pytest.mark.parametrize("name", ["r1", "r2"])
def test_generator_matches_reference_fixture(golden, name):
    d = golden(f"vocoder_gen_{name}.npz")
    cfg, sd = load_fixture(d)
    gen = _gen(cfg, sd)
    lens = d["lens"].tolist()
    y = gen(torch.from_numpy(d["mel"]).to(DEV), lens)[:, 0].cpu().numpy()
    hop = gen.hop
    for b, n in enumerate(lens):
        err = np.abs(y[b, :n * hop] - d["audio"][b, :n * hop]).max()
        print(f"{name} item {b} ({n} frames): max-abs {err:.3e}")
        assert err < 1e-4
        assert not y[b, n * hop:].any()


def test_denoiser_matches_reference_fixture(golden):
    from rad_mmm_amd.vocoder import Denoiser
    cfg, sd = load_fixture(golden("vocoder_gen_r2.npz"))
    d = golden("vocoder_denoiser.npz")
    den = Denoiser(_gen(cfg, sd)).to(DEV)
    lens = d["lens"].tolist()
    audio = torch.from_numpy(d["audio"]).to(DEV)
    for tag, strength in (("s0p1", 0.1), ("s0p001", 0.001)):
        y = den(audio, strength, lens)[:, 0].cpu().numpy()
        if tag == "s0p1":
            bias = den.bias_spec.cpu().numpy()
            berr = np.abs(bias - d["bias_spec"]).max() / np.abs(d["bias_spec"]).max()
            print(f"bias_spec rel max {berr:.3e}")
            assert berr < 1e-5
        for b, n in enumerate(lens):
            m = n // 256 * 256
            ref = d["out_" + tag][b, :m]
            err = np.abs(y[b, :m] - ref).max()
            print(f"denoiser {tag} item {b}: max-abs {err:.3e} (|ref| max {np.abs(ref).max():.3f})")
            assert err < 1e-4 * max(1.0, np.abs(ref).max())
            assert not y[b, m:].any()


def test_v1_full_size_against_fp64_restatement():
    from rad_mmm_amd.vocoder import Denoiser, HiFiGANGenerator
    gen = HiFiGANGenerator(V1)
    sd = random_state(gen, 5)
    gen.load_state_dict(sd)
    gen = gen.to(DEV).eval()
    g = torch.Generator().manual_seed(6)
    B, T = 2, 200
    lens = [200, 137]
    mel = torch.randn(B, 80, T, generator=g) - 2.0
    y = gen(mel.to(DEV), lens)[:, 0]
    den = Denoiser(gen).to(DEV)
    yd = den(y, 0.1, [n * 256 for n in lens])[:, 0]
    y, yd = y.cpu().double(), yd.cpu().double()
    bias_ref = stft_mag_ref(generator_ref(sd, V1, torch.zeros(1, 80, 88))[0])[0][0, :, 0]
    for b, n in enumerate(lens):
        ref = generator_ref(sd, V1, mel[b:b + 1, :, :n])[0, 0]
        diff = y[b, :n * 256] - ref
        mx, rel = diff.abs().max().item(), (diff.norm() / ref.norm()).item()
        print(f"V1 generator item {b}: max-abs {mx:.3e} rel-L2 {rel:.3e} (|ref| max {ref.abs().max():.3f})")
        assert mx <= 1e-4 and rel <= 1e-5
        dref = denoise_ref(y[b:b + 1, :n * 256], bias_ref, 0.1)
        dd = yd[b, :n * 256] - dref
        dmx, drel = dd.abs().max().item(), (dd.norm() / dref.norm()).item()
        print(f"V1 denoiser item {b}: max-abs {dmx:.3e} rel-L2 {drel:.3e}")
        assert dmx <= 1e-4 and drel <= 1e-5


def test_batch_invariance_and_zero_tails(golden):
    # radmmm_rowgemm_f32 picks its tile height from the row count, but every output element sums its K range in the same
    # order whatever the tiling: a batched item is bit-identical to the item alone
    from rad_mmm_amd.vocoder import Denoiser
    cfg, sd = load_fixture(golden("vocoder_gen_r2.npz"))
    gen = _gen(cfg, sd)
    den = Denoiser(gen).to(DEV)
    g = torch.Generator().manual_seed(9)
    T = 12
    lens = [T, 1, 5, 3, T, 2, 7, 4]
    mel = (torch.randn(8, 80, T, generator=g) - 2.0).to(DEV)
    y = gen(mel, lens)[:, 0]
    worst = 0.0
    for b, n in enumerate(lens):
        alone = gen(mel[b:b + 1, :, :n], [n])[0, 0]
        worst = max(worst, (y[b, :n * 256] - alone).abs().max().item())
        assert not y[b, n * 256:].any()
    print(f"generator: batched vs alone max-abs {worst:.3e}")
    assert worst == 0.0
    dl = [max(n, 3) * 256 for n in lens]
    yd = den(y, 0.1, dl)[:, 0]
    worst = 0.0
    for b, n in enumerate(dl):
        alone = den(y[b:b + 1, :n], 0.1)[0, 0]
        worst = max(worst, (yd[b, :n] - alone).abs().max().item())
        assert not yd[b, n:].any()
    print(f"denoiser: batched vs alone max-abs {worst:.3e}")
    assert worst == 0.0


def test_vocode_mels_per_utterance_normalised(golden):
    from rad_mmm_amd.common import SequenceLength
    from rad_mmm_amd.tts_step import TTSTrainingStep
    from rad_mmm_amd.vocoder import Denoiser
    cfg, sd = load_fixture(golden("vocoder_gen_r2.npz"))
    gen = _gen(cfg, sd)
    den = Denoiser(gen).to(DEV)
    step = TTSTrainingStep.__new__(TTSTrainingStep)          # vocode_mels uses nothing of the training modules
    torch.nn.Module.__init__(step)
    step.synth_vocoder = (gen, den)
    assert "synth_vocoder" not in dict(step.named_children())
    lens = torch.tensor([6, 3, 9])
    mels = (torch.randn(3, 80, 9) - 2.0).to(DEV)
    out = step.vocode_mels(mels, SequenceLength(lens.to(DEV), lens))
    assert len(out) == 3
    for a, n in zip(out, lens.tolist()):
        assert a.shape == (n * 256,) and a.dtype == np.float32
        assert abs(np.abs(a).max() - 1.0) < 1e-6


def test_no_device_to_host_sync_with_host_lengths(golden):
    from rad_mmm_amd.vocoder import Denoiser, vocode
    cfg, sd = load_fixture(golden("vocoder_gen_r2.npz"))
    gen = _gen(cfg, sd)
    den = Denoiser(gen).to(DEV)
    mels = (torch.randn(2, 80, 40) - 2.0).to(DEV)
    vocode(gen, den, mels, [40, 30])                         # warm: weights folded, bias spectrum computed
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        audio, s_lens = vocode(gen, den, mels, [40, 25])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert s_lens.tolist() == [40 * 256, 25 * 256] and not s_lens.is_cuda
    a = audio.cpu()
    assert not a[1, 25 * 256:].any()
    assert abs(a[1, :25 * 256].abs().max().item() - 1.0) < 1e-6


def test_cpu_tensors_and_short_denoiser_items_raise(golden):
    from rad_mmm_amd._lib import RadmmmError
    from rad_mmm_amd.vocoder import Denoiser
    cfg, sd = load_fixture(golden("vocoder_gen_r2.npz"))
    gen = _gen(cfg, sd)
    den = Denoiser(gen).to(DEV)
    with pytest.raises(RadmmmError):
        gen(torch.zeros(1, 80, 4))
    audio = torch.zeros(2, 4 * 256, device=DEV)
    with pytest.raises(ValueError, match="reflect"):
        den(audio, 0.1, [4 * 256, 2 * 256])                  # 2 mel frames: 512 samples, not > 512
    with pytest.raises(ValueError):
        den(audio, 0.1, torch.tensor([4 * 256, 512], device=DEV))
