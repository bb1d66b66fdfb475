"""rad_mmm_amd.data.DeviceCollate / TacotronSTFT.mel_spectrogram_ragged (csrc/collate.hip) on the GPU.

- against the batch the reference's AudioDataset methods + DataCollate made from the same raw items
  (tests/golden/collate_small.npz, tests/golden/make_golden_collate.py);
- row by row against the already-pinned single-length path (mel_spectrogram + get_energy_average), bit for bit, also at
  the benchmark's batch size;
- the tracks against the numpy restatement (tests/_collate_ref.py, itself pinned to the fixture on the CPU);
- no synchronisation, and the batch feeds training_step / reconstruct_from_batch_attributes."""
import os

import numpy as np
import pytest
import torch

import _collate_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HOP, N_FFT, F0_MIN = 256, 1024, 80.0
HERE = os.path.dirname(__file__)


def _stft():
    from rad_mmm_amd.audio_processing import TacotronSTFT
    return TacotronSTFT(N_FFT, HOP, N_FFT, 80, 22050, 0.0, 8000.0).to(DEV)


def _ulps(a, b):
    """distance in units of the last place between two float32 arrays (0 where both are +-0)"""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def _cpu(batch):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in batch.items()}


@pytest.fixture(scope="module")
def fx(golden):
    g = golden("collate_small.npz")
    return g, R.fixture_items(g)


def test_device_collate_matches_the_reference_batch(fx):
    """mel / energy_avg: 2e-4 max-abs, the bar tests/test_hip_aux.py::test_stft_mel holds mel_spectrogram to at this
    geometry.  Measured on an MI355X: mel 4.5e-6, energy_avg 1.2e-7.  f0 is exact: the kernel's log is correctly rounded
    and the fixture's voiced values are ones on which every float32 log routine below 0.97 ulp of error agrees
    (tests/golden/make_golden_collate.py robust_hz; on arbitrary values torch's CPU log, which the reference calls, is
    up to 1 ulp off the correctly rounded one and differs between hosts)."""
    from rad_mmm_amd.data import DeviceCollate
    g, items = fx
    out = DeviceCollate(_stft(), f0_min=F0_MIN, use_log_f0=True, distance_tx_unvoiced=True, return_audio=True)(items)
    assert all(out[k].is_cuda for k in ("mel", "text", "f0", "input_lengths", "speaker_f0_mean", "idx", "audio"))
    assert not out["input_lengths_host"].is_cuda and not out["output_lengths_host"].is_cuda
    o = _cpu(out)
    for k in ("text", "input_lengths", "output_lengths", "speaker_ids", "accent_ids", "idx", "audio_lengths", "p_voiced",
              "voiced_mask", "speaker_f0_mean", "speaker_f0_std", "speaker_energy_mean", "speaker_energy_std"):
        assert o[k].dtype == g[f"batch.{k}"].dtype and o[k].shape == g[f"batch.{k}"].shape, k
        assert np.array_equal(o[k], g[f"batch.{k}"]), k
    assert np.array_equal(o["input_lengths_host"], g["batch.input_lengths"])
    assert np.array_equal(o["output_lengths_host"], g["batch.output_lengths"])
    assert o["audiopaths"] == g["lists.audiopaths"].tolist() and o["text_raw"] == g["lists.text_raw"].tolist()
    assert o["language"] == g["lists.language"].tolist()
    u = _ulps(o["f0"], g["batch.f0"])
    print(f"collate f0: {int((u > 0).sum())} of {u.size} elements differ from the reference, max {int(u.max())} ulp")
    assert u.max() == 0
    assert o["mel"].shape == g["batch.mel"].shape and o["energy_avg"].shape == g["batch.energy_avg"].shape
    e_mel = float(np.abs(o["mel"] - g["batch.mel"]).max())
    e_en = float(np.abs(o["energy_avg"] - g["batch.energy_avg"]).max())
    print(f"collate mel max-abs {e_mel:.3e}  energy_avg max-abs {e_en:.3e}")
    assert e_mel < 2e-4 and e_en < 2e-4
    for b, (t, l) in enumerate(zip(g["batch.output_lengths"], g["batch.input_lengths"])):
        assert not o["mel"][b, :, t:].any() and not o["energy_avg"][b, t:].any() and not o["f0"][b, t:].any()
        assert not o["attn_prior"][b, t:].any() and not o["attn_prior"][b, :, l:].any()
        got, ref = o["attn_prior"][b, :t, :l], g["batch.attn_prior"][b, :t, :l]
        assert np.all(np.abs(got - ref) <= 6e-8 * np.abs(ref) + 1e-9 * ref.max())      # tests/test_data_path.py's bar
    # the audio of the batch: the int16 samples over max_wav_value, zero padded (exact: a power of two)
    order = [int(i) - 100 for i in g["batch.idx"]]
    assert o["audio"].shape == (len(items), 1, int(g["batch.audio_lengths"].max()))
    for b, i in enumerate(order):
        s = len(items[i]["audio"])
        assert np.array_equal(o["audio"][b, 0, :s], items[i]["audio"].astype(np.float32) / 32768.0)
        assert not o["audio"][b, 0, s:].any()


@pytest.mark.parametrize("use_log_f0", [True, False])
@pytest.mark.parametrize("distance_tx", [True, False])
def test_track_settings_against_the_reference(fx, use_log_f0, distance_tx):
    from rad_mmm_amd.data import DeviceCollate
    g, items = fx
    out = DeviceCollate(_stft(), f0_min=F0_MIN, use_log_f0=use_log_f0, distance_tx_unvoiced=distance_tx,
                        use_attn_prior_masking=False)(items)
    assert out["attn_prior"] is None
    u = _ulps(out["f0"].cpu().numpy(), g[f"f0.log{int(use_log_f0)}.dtx{int(distance_tx)}"])
    print(f"f0 log={use_log_f0} dtx={distance_tx}: {int((u > 0).sum())} of {u.size} differ, max {int(u.max())} ulp")
    assert u.max() == 0


def _per_item_identity(stft, audios, scaled=True):
    """ragged mel / energy rows == mel_spectrogram / get_energy_average of each utterance alone, bit for bit"""
    from rad_mmm_amd.data import get_energy_average
    B = len(audios)
    lens = [len(a) for a in audios]
    Smax = max(lens)
    y = torch.zeros(B, Smax)
    for b, a in enumerate(audios):
        y[b, :len(a)] = torch.from_numpy(a)
    y = y.to(DEV)
    Tmax = 1 + Smax // HOP
    energy = torch.empty(B, Tmax, device=DEV)
    mel = stft.mel_spectrogram_ragged(y, lens, energy=energy, scaled_energy=scaled)
    assert mel.shape == (B, 80, Tmax)
    for b, a in enumerate(audios):
        one = stft.mel_spectrogram(torch.from_numpy(a)[None].to(DEV))
        t = 1 + len(a) // HOP
        assert one.shape == (1, 80, t)
        assert torch.equal(mel[b, :, :t], one[0]), f"row {b}: max diff {float((mel[b, :, :t] - one[0]).abs().max()):.3e}"
        assert torch.equal(energy[b, :t], get_energy_average(one[0], scaled))
        assert not mel[b, :, t:].any() and not energy[b, t:].any()
    return mel


def test_ragged_mel_rows_equal_the_single_length_path_bit_for_bit(fx):
    _, items = fx
    stft = _stft()
    _per_item_identity(stft, [it["audio"].astype(np.float32) / 32768.0 for it in items])
    _per_item_identity(stft, [it["audio"].astype(np.float32) / 32768.0 for it in items[:2]], scaled=False)


def test_ragged_mel_rows_at_the_benchmark_batch_size():
    """B = 32, lengths from 0.6 to 1.0 of 800 frames as radmmm_synth.synthetic_batch(ragged=True) draws them"""
    r = np.random.Generator(np.random.PCG64(1234))
    T = 800
    frames = np.sort(r.integers(int(0.6 * T), T + 1, size=32))[::-1].copy()
    frames[0] = T
    audios = []
    for f in frames:
        n = (int(f) - 1) * HOP + int(r.integers(0, HOP))
        audios.append(np.clip(0.3 * r.standard_normal(n), -1, 1).astype(np.float32))
    mel = _per_item_identity(_stft(), audios)
    assert mel.shape == (32, 80, T)


def _random_track(r, T, kind):
    if kind == "all_voiced":
        v = np.ones(T, bool)
    elif kind == "first":
        v = np.zeros(T, bool); v[0] = True
    elif kind == "last":
        v = np.zeros(T, bool); v[-1] = True
    elif kind == "none":
        v = np.zeros(T, bool)
    else:
        v = r.random(T) < r.choice([0.03, 0.3, 0.8])
        run = r.integers(0, max(1, T // 2))
        v[run:run + T // 3] = False                           # one long unvoiced stretch
    return np.where(v, r.uniform(50.0, 400.0, T), 0.0).astype(np.float32)


@pytest.mark.parametrize("use_log_f0", [True, False])
def test_padded_tensor_functions_against_the_restatement(use_log_f0):
    """f0_normalize + distance_tx_unvoiced on padded batches: T of 1, 2, 255, 256, 257, 5000, the voicing patterns at the
    edges, and the all-unvoiced utterance (d = t + 1, as scipy)."""
    from rad_mmm_amd.data import distance_tx_unvoiced, f0_denormalize, f0_normalize
    r = np.random.Generator(np.random.PCG64(11))
    for Tmax in (1, 2, 255, 256, 257, 5000):
        kinds = ["random", "all_voiced", "first", "last", "none", "random", "random"]
        lens = [Tmax] + [int(r.integers(1, Tmax + 1)) for _ in kinds[1:]]
        raw = [_random_track(r, t, k) for t, k in zip(lens, kinds)]
        f0 = torch.from_numpy(R.pad_rows(raw, Tmax, np.float32)).to(DEV)
        norm = f0_normalize(f0, F0_MIN, use_log_f0)
        want_n = R.pad_rows([R.f0_transform(x, F0_MIN, use_log_f0, False) for x in raw], Tmax, np.float32)
        assert _ulps(norm.cpu().numpy(), want_n).max() <= (1 if use_log_f0 else 0)
        got = distance_tx_unvoiced(torch.from_numpy(want_n).to(DEV), torch.tensor(lens, device=DEV)).cpu().numpy()
        want = R.pad_rows([R.f0_transform(x, F0_MIN, use_log_f0, True) for x in raw], Tmax, np.float32)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (Tmax, int(_ulps(got, want).max()))
        if use_log_f0:
            back = f0_denormalize(torch.from_numpy(want_n).to(DEV), F0_MIN, True).cpu().numpy()
            hz = R.pad_rows(raw, Tmax, np.float32)
            assert np.allclose(back, np.where(hz >= F0_MIN, hz, 0.0), rtol=1e-5)


def test_all_unvoiced_utterance_matches_scipy(fx):
    from rad_mmm_amd.data import distance_tx_unvoiced, f0_normalize
    g, _ = fx
    f0 = torch.from_numpy(g["unvoiced.f0_in"])[None].to(DEV)
    out = distance_tx_unvoiced(f0_normalize(f0, F0_MIN, True), torch.tensor([f0.shape[1]], device=DEV))
    assert np.array_equal(out[0].cpu().numpy().view(np.int32), g["unvoiced.f0_out"].view(np.int32))


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_device_collate_on_random_ragged_items(dtype):
    """frame counts 3, 255, 256, 257 and 5000 in one batch, both sample types: tracks, ids and audio against the
    restatement, mel rows against the single-length path"""
    from rad_mmm_amd.data import DeviceCollate, plan_batch
    r = np.random.Generator(np.random.PCG64(5))
    items = []
    kinds = ["random", "none", "first", "last", "all_voiced"]
    for i, (T, kind) in enumerate(zip((3, 255, 256, 257, 5000), kinds)):
        n = (T - 1) * HOP + int(r.integers(1, HOP)) if T != 256 else 255 * HOP
        a = np.clip(np.round(0.2 * 32768 * r.standard_normal(n)), -32768, 32767).astype(dtype)
        f0 = _random_track(r, T, kind)
        items.append({"audio": a, "text_encoded": r.integers(1, 90, 3 + 2 * i), "f0": f0,
                      "p_voiced": r.random(T).astype(np.float32), "voiced_mask": (f0 > 0).astype(np.float32),
                      "speaker_id": i, "accent_id": i % 2, "idx": 7 * i, "speaker_f0_mean": 0.5 * i, "speaker_f0_std": 1.0 + i,
                      "speaker_energy_mean": 0.25 * i, "speaker_energy_std": 2.0 + i})
    items.insert(2, None)                                       # dropped, as the reference does
    stft = _stft()
    collate = DeviceCollate(stft, f0_min=F0_MIN, use_log_f0=True, distance_tx_unvoiced=True, return_audio=True)
    kept = [it for it in items if it is not None]
    order = plan_batch(kept, HOP).order
    want = R.collate(kept, order, F0_MIN, True, True, HOP)
    for _ in range(2):                                          # the second call reuses staging and scratch buffers
        o = _cpu(collate(items))
        for k in ("text", "input_lengths", "output_lengths", "audio_lengths", "speaker_ids", "accent_ids", "idx", "p_voiced",
                  "voiced_mask", "speaker_f0_mean", "speaker_f0_std", "speaker_energy_mean", "speaker_energy_std", "audio"):
            assert o[k].dtype == want[k].dtype and np.array_equal(o[k], want[k]), k
        assert _ulps(o["f0"], want["f0"]).max() <= 1
        unv = want["f0"] <= 0
        assert np.array_equal(o["f0"][unv], want["f0"][unv])     # the distance term is exact
    for b, i in enumerate(order):
        a = kept[i]["audio"].astype(np.float32) / 32768.0
        one = stft.mel_spectrogram(torch.from_numpy(a)[None].to(DEV))[0].cpu().numpy()
        t = one.shape[1]
        assert np.array_equal(o["mel"][b, :, :t], one) and not o["mel"][b, :, t:].any()
    assert collate([None, None]) is None


def _step_model(g, binarization_start_iter=10):
    import radmmm_synth as S
    from rad_mmm_amd.decoders import RADMMMFlow
    from rad_mmm_amd.encoder import Encoder
    from rad_mmm_amd.loss import RADMMMLoss
    from rad_mmm_amd.tts_step import TTSTrainingStep
    kw = {k[4:]: g[k].item() for k in g.files if k.startswith("cfg.")}
    model = TTSTrainingStep(Encoder(3, 32, 5), RADMMMFlow(use_accent=True, **kw), RADMMMLoss(sigma=1.0, kl_loss_start_iter=5),
                            n_speakers=3, n_accents=2, n_text_tokens=40, n_text_dim=32, n_speaker_dim=16, n_accent_dim=8,
                            use_accent=True, binarization_start_iter=binarization_start_iter)
    names = [n for n in model.state_dict() if not n.startswith("decoder_criterion")]
    proc = S.procedural_decoder_state({n: tuple(model.state_dict()[n].shape) for n in names})
    model.load_state_dict({n: torch.from_numpy(np.asarray(v)) for n, v in proc.items()}, strict=False)
    return model.to(DEV).train()


def _reference_batch(g):
    batch = {k[6:]: torch.from_numpy(np.asarray(g[k])).to(DEV) for k in g if k.startswith("batch.")}
    batch["input_lengths_host"] = torch.from_numpy(g["batch.input_lengths"])
    batch["output_lengths_host"] = torch.from_numpy(g["batch.output_lengths"])
    return batch


@pytest.mark.parametrize("tag,step", [("soft", 0), ("hard", 10)])
def test_training_step_on_the_device_batch_equals_the_reference_batch(fx, tag, step, monkeypatch):
    """same loss terms within the bars of tests/test_tts_step.py; identical alignments once MAS binarises them"""
    import torch.nn.functional as F
    from rad_mmm_amd.data import DeviceCollate
    g, items = fx
    monkeypatch.setattr(F, "dropout", lambda x, p=0.5, training=True, inplace=False: x)
    model = _step_model(np.load(os.path.join(HERE, "golden", "tts_step.npz")))
    ours = DeviceCollate(_stft(), f0_min=F0_MIN, use_log_f0=True, distance_tx_unvoiced=True)(items)
    loss_a, losses_a, out_a = model.training_step(ours, global_step=step)
    loss_b, losses_b, out_b = model.training_step(_reference_batch(g), global_step=step)
    assert set(losses_a) == set(losses_b)
    for k in losses_b:
        a, ref = float(losses_a[k][0]), float(losses_b[k][0])
        assert abs(a - ref) <= 1e-4 * max(abs(ref), 1e-3), (k, a, ref)
    assert abs(float(loss_a) - float(loss_b)) < 1e-4 * abs(float(loss_b))
    if tag == "hard":
        assert torch.equal(out_a["attn"], out_b["attn"])
    else:
        assert rel_err(out_a["attn"].detach().cpu(), out_b["attn"].detach().cpu()) < 1e-4
    loss_a.backward()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)


def test_collate_then_training_step_never_synchronises(fx):
    from rad_mmm_amd.data import DeviceCollate
    _, items = fx
    model = _step_model(np.load(os.path.join(HERE, "golden", "tts_step.npz")), binarization_start_iter=0)
    collate = DeviceCollate(_stft(), f0_min=F0_MIN, use_log_f0=True, distance_tx_unvoiced=True, return_audio=True)

    def step():
        loss, _, _ = model.training_step(collate(items), global_step=10)
        loss.backward()
        return loss
    for _ in range(3):                                          # both staging buffers used, priors banked, kernels loaded
        step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = step()
        loss = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert np.isfinite(float(loss.detach()))


def test_reconstruct_from_batch_attributes_reads_the_device_batch(fx):
    from rad_mmm_amd.data import DeviceCollate
    from rad_mmm_amd.synthesis import reconstruct_from_batch_attributes
    g, items = fx
    model = _step_model(np.load(os.path.join(HERE, "golden", "tts_step.npz"))).eval()
    batch = DeviceCollate(_stft(), f0_min=F0_MIN, use_log_f0=True, distance_tx_unvoiced=True)(items)
    with torch.no_grad():
        out = reconstruct_from_batch_attributes(model, batch, vocode=False)
    assert out["out_lens"].tolist() == g["batch.output_lengths"].tolist() == batch["output_lengths_host"].tolist()
    assert out["output_mel"].shape[0] == len(items) and torch.isfinite(out["output_mel"]).all()


def test_errors(fx):
    from rad_mmm_amd.audio_processing import TacotronSTFT
    from rad_mmm_amd.data import DeviceCollate, distance_tx_unvoiced, f0_normalize
    from rad_mmm_amd._lib import RadmmmError
    _, items = fx
    with pytest.raises(RuntimeError, match="GPU"):
        DeviceCollate(TacotronSTFT(N_FFT, HOP, N_FFT, 80, 22050, 0.0, 8000.0))       # model tensors on the CPU
    collate = DeviceCollate(_stft(), f0_min=F0_MIN)
    bad = [dict(it) for it in items]
    bad[1]["f0"] = bad[1]["f0"][:-2]
    with pytest.raises(ValueError, match="frames"):
        collate(bad)
    bad = [dict(it) for it in items]
    bad[0]["audio"] = bad[0]["audio"][:N_FFT // 2]
    bad[0]["f0"] = bad[0]["p_voiced"] = bad[0]["voiced_mask"] = np.zeros(3, np.float32)
    with pytest.raises(ValueError, match="filter_length"):
        collate(bad)
    bad = [dict(it) for it in items]
    bad[2]["audio"] = bad[2]["audio"].astype(np.float32)
    with pytest.raises(ValueError, match="mixed"):
        collate(bad)
    with pytest.raises(RadmmmError):
        f0_normalize(torch.zeros(2, 5), F0_MIN)
    with pytest.raises(RadmmmError):
        distance_tx_unvoiced(torch.zeros(2, 5), torch.tensor([5, 5]))
    with pytest.raises(ValueError, match="filter_length"):
        _stft().mel_spectrogram_ragged(torch.zeros(2, 4000, device=DEV), [4000, 500])
    with pytest.raises(RuntimeError, match="MI355X"):
        _stft().mel_spectrogram_ragged(torch.zeros(2, 4000), [4000, 3000])
    assert collate(items)["mel"].shape[0] == len(items)         # the object is still usable after the refusals
