"""Host side of the on-device batch builder (rad_mmm_amd.data.plan_batch / DeviceCollate, csrc/collate.hip), without a
GPU: the layout plan against the batch the reference's DataCollate made (tests/golden/collate_small.npz,
tests/golden/make_golden_collate.py), the numpy restatement the GPU tests lean on against the same fixture, and the C ABI
of the new entry points."""
import ctypes
import os
import re

import numpy as np
import pytest

import _collate_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP, F0_MIN = 256, 80.0


@pytest.fixture(scope="module")
def fx(golden):
    g = golden("collate_small.npz")
    assert [int(v) for v in g["cfg"][:4]] == [22050, 1024, HOP, 80] and float(g["cfg"][4]) == F0_MIN
    return g, R.fixture_items(g)


def test_plan_batch_reproduces_the_reference_order_and_lengths(fx):
    from rad_mmm_amd.data import plan_batch
    g, items = fx
    plan = plan_batch(items, HOP, 1024)
    assert [items[i]["idx"] for i in plan.order] == g["batch.idx"].tolist()          # the tie (two texts of 9 ids) included
    lens = sorted(len(it["text_encoded"]) for it in items)
    assert any(a == b for a, b in zip(lens, lens[1:])), "the fixture must hold a tie"
    assert plan.input_lengths.tolist() == g["batch.input_lengths"].tolist()
    assert plan.output_lengths.tolist() == g["batch.output_lengths"].tolist()
    assert plan.audio_lengths.tolist() == g["batch.audio_lengths"].tolist()
    assert (plan.Smax, plan.Tmax, plan.Lmax) == (int(g["batch.audio_lengths"].max()), g["batch.mel"].shape[2],
                                                 g["batch.text"].shape[1])
    assert plan.output_lengths.tolist() == [1 + s // HOP for s in plan.audio_lengths.tolist()]
    assert any(s % HOP == 0 for s in plan.audio_lengths.tolist()) and any(s % HOP for s in plan.audio_lengths.tolist())
    # the packed sections: items back to back in sorted order, sample starts on 16-byte boundaries, nothing overlaps
    assert plan.sample_offsets[0] == plan.frame_offsets[0] == plan.token_offsets[0] == 0
    assert all(o % 8 == 0 for o in plan.sample_offsets.tolist())
    assert np.all(np.diff(plan.sample_offsets) >= plan.audio_lengths[:-1])
    assert np.diff(plan.frame_offsets).tolist() == plan.output_lengths[:-1].tolist()
    assert np.diff(plan.token_offsets).tolist() == plan.input_lengths[:-1].tolist()
    assert plan.n_frames == plan.output_lengths.sum() and plan.n_tokens == plan.input_lengths.sum()
    assert plan.n_samples >= plan.sample_offsets[-1] + plan.audio_lengths[-1]
    assert plan.audio_dtype == np.int16 and plan.tracks == ("f0", "p_voiced", "voiced_mask")


def test_plan_batch_accepts_cpu_tensors_and_float_audio(fx):
    import torch
    from rad_mmm_amd.data import plan_batch
    _, items = fx
    conv = [dict(it, audio=torch.from_numpy(it["audio"].astype(np.float32)), text_encoded=torch.from_numpy(it["text_encoded"]),
                 f0=torch.from_numpy(it["f0"])) for it in items]
    a, b = plan_batch(items, HOP), plan_batch(conv, HOP)
    assert a.order == b.order and b.audio_dtype == np.float32 and a.output_lengths.tolist() == b.output_lengths.tolist()


def test_plan_batch_errors(fx):
    from rad_mmm_amd.data import plan_batch
    _, items = fx
    with pytest.raises(ValueError, match="empty"):
        plan_batch([], HOP)
    bad = [dict(it) for it in items]
    bad[2]["f0"] = bad[2]["f0"][:-1]
    with pytest.raises(ValueError, match="frames"):
        plan_batch(bad, HOP)
    bad = [dict(it) for it in items]
    bad[1]["audio"] = bad[1]["audio"][:512]
    bad[1]["f0"] = bad[1]["p_voiced"] = bad[1]["voiced_mask"] = np.zeros(3, np.float32)
    with pytest.raises(ValueError, match="filter_length"):
        plan_batch(bad, HOP, 1024)
    bad = [dict(it) for it in items]
    bad[0]["audio"] = bad[0]["audio"].astype(np.float32)
    with pytest.raises(ValueError, match="mixed"):
        plan_batch(bad, HOP)
    bad = [dict(it) for it in items]
    bad[3]["p_voiced"] = None
    with pytest.raises(ValueError, match="every item"):
        plan_batch(bad, HOP)


@pytest.mark.parametrize("use_log_f0", [True, False])
@pytest.mark.parametrize("distance_tx", [True, False])
def test_numpy_restatement_equals_the_reference_batch(fx, use_log_f0, distance_tx):
    from rad_mmm_amd.data import plan_batch
    g, items = fx
    order = plan_batch(items, HOP).order
    out = R.collate(items, order, F0_MIN, use_log_f0, distance_tx, HOP)
    ref_f0 = g[f"f0.log{int(use_log_f0)}.dtx{int(distance_tx)}"]
    assert out["f0"].dtype == ref_f0.dtype == np.float32
    assert np.array_equal(out["f0"].view(np.int32), ref_f0.view(np.int32))           # to the last bit
    if use_log_f0 and distance_tx:
        assert np.array_equal(ref_f0, g["batch.f0"])
        for k in ("text", "input_lengths", "output_lengths", "audio_lengths", "speaker_ids", "accent_ids", "idx", "p_voiced",
                  "voiced_mask", "speaker_f0_mean", "speaker_f0_std", "speaker_energy_mean", "speaker_energy_std"):
            assert out[k].dtype == g[f"batch.{k}"].dtype and np.array_equal(out[k], g[f"batch.{k}"]), k
        assert [items[i]["audiopath"] for i in order] == g["lists.audiopaths"].tolist()


def test_fixture_f0_tracks_hold_the_cases_the_issue_names(fx):
    g, items = fx
    gaps, starts, ends = set(), 0, 0
    for it in items:
        v = it["f0"] > 0
        assert v.any()                                     # every utterance of the main fixture has a voiced frame
        starts += int(not v[0])
        ends += int(not v[-1])
        idx = np.flatnonzero(v)
        gaps |= set((np.diff(idx) - 1).tolist())
        assert (it["f0"][v] < F0_MIN).any() or (it["f0"][v] >= F0_MIN).all()
    assert {1, 2} <= gaps and max(gaps) >= 30 and starts and ends
    allv = np.concatenate([it["f0"][it["f0"] > 0] for it in items])
    assert (allv < F0_MIN).any() and (allv >= F0_MIN).any()


def test_all_unvoiced_utterance_follows_scipy(fx):
    """Without any voiced frame scipy's distance transform has no background; scipy 1.15.3 then returns [1 .. T] (stored in
    the fixture), as if a voiced frame sat just before the utterance.  The restatement (and the kernel) do the same."""
    g, _ = fx
    T = g["unvoiced.edt"].size
    assert np.array_equal(g["unvoiced.edt"], np.arange(1, T + 1))
    assert np.array_equal(R.distance_to_voiced(np.zeros(T, bool)), g["unvoiced.edt"])
    out = R.f0_transform(g["unvoiced.f0_in"], F0_MIN, True, True)
    assert np.array_equal(out.view(np.int32), g["unvoiced.f0_out"].view(np.int32))


def test_distance_restatement_against_brute_force():
    r = np.random.Generator(np.random.PCG64(3))
    for T in (1, 2, 5, 64, 300):
        for p in (0.02, 0.5, 0.98):
            v = r.random(T) < p
            if not v.any():
                v[r.integers(T)] = True
            idx = np.flatnonzero(v)
            want = np.abs(np.arange(T)[:, None] - idx[None, :]).min(1)
            assert np.array_equal(R.distance_to_voiced(v), want.astype(np.float64))


def test_new_entry_points_are_declared_exported_and_bound():
    import rad_mmm_amd._lib as L
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "radmmm_hip.h")).read(), flags=re.S)
    protos = dict(re.findall(r"\b(radmmm_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S))
    raw = ctypes.CDLL(L.LIB_PATH)
    for name, n_args in (("radmmm_collate_scratch_floats", 5), ("radmmm_collate_unpack_pad", 11), ("radmmm_collate_mel", 14),
                         ("radmmm_collate_tracks", 23)):
        assert name in protos and protos[name].count(",") + 1 == n_args, name
        assert hasattr(raw, name), name
        assert len(getattr(L.lib, name).argtypes) == n_args, name
    assert getattr(L.lib, "radmmm_collate_scratch_floats").restype is ctypes.c_int64
    assert "#define RADMMM_ABI_VERSION 4" in open(os.path.join(ROOT, "include", "radmmm_hip.h")).read()
    # argument validation happens before any HIP call
    L.lib.radmmm_last_error.restype = ctypes.c_char_p
    assert L.lib.radmmm_collate_mel(None, None, None, None, None, None, 1, 2048, 1024, 256, 80, 1e-5, 1, None) == -1
    assert b"collate_mel" in L.lib.radmmm_last_error()
    assert L.lib.radmmm_collate_scratch_floats(32, 204800, 1024, 256, 80) == L.lib.radmmm_stft_mel_scratch_floats(32, 204800, 1024, 256, 80)
