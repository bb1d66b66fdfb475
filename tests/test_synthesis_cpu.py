"""CPU checks of the synthesis glue: the new C entry points reject null pointers and bad sizes before any HIP call; the CPU
restatement (tests/_synth_ref.py) against tests/golden/synth_small.npz, which the reference's own components produced
(tests/golden/make_golden_synth.py); its quantisation and f0 rules; mel_descale."""
import os

import numpy as np
import torch

from _synth_ref import synth_ref

HERE = os.path.dirname(os.path.abspath(__file__))
SPECS = {"f0": dict(n_layers=2, target_offset=-5.0), "energy": dict(n_layers=2, target_offset=-0.75),
         "voiced": dict(n_layers=2), "duration": dict(n_layers=2, log_target=True)}


def load_synth_fixture():
    """synth_small.npz -> (fixture arrays as tensors, decoder kwargs, step state_dict with the procedural decoder)"""
    from oracle import radmmm_oracle as O
    with np.load(os.path.join(HERE, "golden", "synth_small.npz")) as f:
        d = {k: f[k] for k in f.files}
    cfg_kwargs = {k[4:]: d[k].item() for k in d if k.startswith("cfg.")}
    cfg = O.DecoderConfig(**cfg_kwargs)
    sd = {k[3:]: torch.from_numpy(np.asarray(v)) for k, v in d.items() if k.startswith("sd.")}
    for k, v in O.procedural_decoder_state(O.decoder_state_shapes(cfg), end_scale=float(d["end_scale"])).items():
        sd["decoder." + k] = torch.from_numpy(np.asarray(v))
    t = {k: torch.from_numpy(np.asarray(v)) for k, v in d.items() if not k.startswith(("sd.", "cfg."))}
    return t, cfg_kwargs, sd


def valid_rel(a, ref, lens):
    """max-norm relative error over the frames t < lens[b] of [B, ..., T] tensors"""
    err = 0.0
    for b, n in enumerate(lens.tolist()):
        r = ref[b, ..., :n]
        err = max(err, float((a[b, ..., :n].float() - r).abs().max() / r.abs().max()))
    return err


def test_restatement_matches_reference_fixture():
    from oracle import radmmm_oracle as O
    t, cfg_kwargs, sd = load_synth_fixture()
    with torch.no_grad():
        ref = synth_ref(sd, O.DecoderConfig(**cfg_kwargs), SPECS, t["text"], t["text_lens"], t["speaker_ids"],
                        t["accent_ids"], t["residual"], t["f0_mean"], t["f0_std"])
    n = t["out_lens"]
    assert torch.equal(ref["durations"], t["durations"].long()) and torch.equal(ref["out_lens"], n.long())
    assert float((ref["d_pred"] - t["d_pred"]).abs().max() / t["d_pred"].abs().max()) < 1e-5
    valid = torch.arange(int(n.max()))[None] < n[:, None]
    assert torch.equal(ref["voiced"], t["voiced"] & valid)
    assert valid_rel(ref["f0"], t["f0"], n) < 1e-5 and valid_rel(ref["energy"], t["energy"], n) < 1e-5
    e = valid_rel(ref["mel"], t["mel"], n // 2 * 2)
    print(f"mel {e:.2e}")
    assert e < 1e-4


def test_synth_entry_points_validate_arguments():
    import rad_mmm_amd._lib as L
    lib = L.lib
    fake = 1 << 20                                   # never dereferenced: validation fails first
    err = lambda: lib.radmmm_last_error().decode()   # noqa: E731
    assert lib.radmmm_synth_durations(None, 4, None, 1, 4, 0, fake, fake, fake, None) == -1 and "null" in err()
    assert lib.radmmm_synth_durations(fake, 4, None, 0, 4, 0, fake, fake, fake, None) == -1 and "bad dims" in err()
    assert lib.radmmm_synth_durations(fake, 40000, None, 1, 40000, 0, fake, fake, fake, None) == -1
    assert lib.radmmm_synth_durations(fake, 2, None, 2, 4, 0, fake, fake, fake, None) == -1      # item stride < Tt
    assert lib.radmmm_synth_regulate(fake, 2048, 512, 4, 512, None, fake, 1, 8, fake, 512, None) == -1 and "null" in err()
    assert lib.radmmm_synth_regulate(fake, 2080, 520, 4, 520, fake, fake, 1, 8, fake, 516, None) == -1   # ldc < C
    assert lib.radmmm_synth_regulate(fake, 2060, 515, 4, 515, fake, fake, 1, 8, fake, 544, None) == -1   # C % 4
    assert lib.radmmm_synth_regulate(fake + 4, 2048, 512, 4, 512, fake, fake, 1, 8, fake, 512, None) == -1
    assert "aligned" in err()
    assert lib.radmmm_synth_regulate(fake, 20000 * 512, 512, 20000, 512, fake, fake, 1, 8, fake, 512, None) == -1
    assert lib.radmmm_synth_f0_stats(fake, 8, fake, 8, None, 1, 8, fake, 4, None) == -1 and "null" in err()
    assert lib.radmmm_synth_f0_stats(fake, 8, fake, 8, fake, 1, 8, fake, 0, None) == -1 and "bad dims" in err()
    assert lib.radmmm_synth_f0_stats(fake, 4, fake, 8, fake, 1, 8, fake, 4, None) == -1           # stride < T
    assert lib.radmmm_synth_f0_apply(fake, 8, fake, 8, fake, 8, fake, 1, 8, fake, 4, None, None, fake, fake, fake,
                                     None) == -1 and "f0_mean" in err()
    assert lib.radmmm_synth_f0_apply(fake, 8, fake, 8, fake, 8, fake, 1, 8, None, 0, None, None, None, fake, fake,
                                     None) == -1 and "null" in err()
    assert lib.radmmm_synth_f0_apply(fake, 8, fake, 8, fake, 8, fake, 1, 8, fake, 2000, fake, fake, fake, fake, fake,
                                     None) == -1 and "bad dims" in err()


def test_restatement_quantisation_and_f0_rules():
    from _synth_ref import durations_ref, f0_ref
    d = torch.tensor([[0.5, 1.5, 2.5, -3.0, 7.2], [2.6, 0.1, 9.0, 9.0, 9.0]])
    assert durations_ref(d, torch.tensor([5, 2])).tolist() == [[1, 2, 2, 1, 7], [3, 1, 0, 0, 0]]
    f0 = torch.tensor([[100.0, 200.0, 300.0, 400.0]])
    v = torch.tensor([[True, True, False, True]])
    f, vo = f0_ref(f0, v, torch.tensor([3]), torch.tensor([10.0]), torch.tensor([2.0]))
    assert vo.tolist() == [[True, True, False, False]]
    s = float(torch.tensor([100.0, 200.0]).std())
    assert torch.allclose(f, torch.tensor([[(100 - 150) / s * 2 + 10, (200 - 150) / s * 2 + 10, 0.0, 0.0]]))
    f, _ = f0_ref(f0, v, torch.tensor([1]), torch.tensor([10.0]), torch.tensor([2.0]))         # one voiced frame: unshifted
    assert f.tolist() == [[100.0, 0.0, 0.0, 0.0]]


def test_mel_descale():
    from rad_mmm_amd.synthesis import mel_descale
    from rad_mmm_amd.tts_step import TTSTrainingStep
    m = torch.randn(2, 80, 7)
    assert torch.equal(mel_descale(m), m * 2 - 5) and torch.equal(TTSTrainingStep.mel_descale(m), m * 2 - 5)
    assert (mel_descale(TTSTrainingStep.mel_scale(m)) - m).abs().max() < 1e-6
