"""Numpy restatement of the parts of the collate path that are not the STFT: unpack / scale / reflect-pad of the samples,
the f0 transform (data.py:321-327, 527-532, with the 1-D distance transform written out instead of scipy's), and the
zero padding of DataCollate (data.py:616-790).  tests/test_collate_cpu.py pins it to the reference-made fixture
(tests/golden/collate_small.npz) bit for bit; the GPU tests lean on it for shapes the fixture does not hold."""
import numpy as np


def reflect_pad(audio, n_fft, max_wav_value=32768.0):
    """one utterance (int16 or float32 at wav scale) -> float32 [S + n_fft]: scaled, reflected at both ends (no edge repeat)"""
    x = np.asarray(audio).astype(np.float32) * np.float32(1.0 / max_wav_value)
    return np.pad(x, (n_fft // 2, n_fft // 2), mode="reflect")


def distance_to_voiced(voiced):
    """distance in frames to the nearest True of a 1-D bool array: scipy.ndimage.distance_transform_edt(~voiced) in one
    dimension.  Without any True scipy 1.15.3 returns [1, 2, ..., T]; so does this."""
    voiced = np.asarray(voiced, dtype=bool)
    T = voiced.size
    t = np.arange(T)
    if not voiced.any():
        return (t + 1).astype(np.float64)
    last = np.maximum.accumulate(np.where(voiced, t, -1))
    nxt = np.minimum.accumulate(np.where(voiced, t, 2 * T + 2)[::-1])[::-1]
    big = np.float64(4 * T + 4)
    d = np.minimum(np.where(last >= 0, t - last, big), np.where(nxt <= T, nxt - t, big))
    return d.astype(np.float64)


def f0_transform(f0, f0_min, use_log_f0, distance_tx):
    """raw pyin track (Hz, 0 unvoiced) -> what __getitem__ hands DataCollate, as the float32 DataCollate stores"""
    x = np.asarray(f0, dtype=np.float32).copy()
    if use_log_f0:
        m = x >= np.float32(f0_min)
        # the correctly rounded float32 log (float64 log, rounded once): the same on every host, unlike a float32 log
        # routine (torch's, which the reference calls, and numpy's both change with the vector unit; up to 1 ulp).  The
        # fixture's voiced values are chosen so that every such routine agrees on them (make_golden_collate.robust_hz)
        x[m] = np.log(x[m].astype(np.float64)).astype(np.float32)
        x[~m] = 0.0
    if not distance_tx:
        return x
    d = distance_to_voiced(x > 0.0)
    with np.errstate(divide="ignore"):
        dm = np.log(d)
    dm[dm <= 0] = 0.0
    return (x.astype(np.float64) - dm).astype(np.float32)


def pad_rows(rows, width, dtype):
    out = np.zeros((len(rows), width), dtype=dtype)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def collate(items, order, f0_min, use_log_f0, distance_tx, hop):
    """the non-STFT tensors of the batch for items in `order` (a list of indices)"""
    its = [items[i] for i in order]
    frames = [1 + len(it["audio"]) // hop for it in its]
    Tmax = max(frames)
    out = {"text": pad_rows([np.asarray(it["text_encoded"]) for it in its], max(len(it["text_encoded"]) for it in its), np.int64),
           "input_lengths": np.array([len(it["text_encoded"]) for it in its], dtype=np.int64),
           "output_lengths": np.array(frames, dtype=np.int64),
           "audio_lengths": np.array([len(it["audio"]) for it in its], dtype=np.int64),
           "speaker_ids": np.array([int(it["speaker_id"]) for it in its], dtype=np.int64),
           "accent_ids": np.array([int(it["accent_id"]) for it in its], dtype=np.int64),
           "idx": np.array([int(it["idx"]) for it in its], dtype=np.int64)}
    for k in ("speaker_f0_mean", "speaker_f0_std", "speaker_energy_mean", "speaker_energy_std"):
        out[k] = np.array([it[k] for it in its], dtype=np.float32)
    if its[0].get("f0") is not None:
        out["f0"] = pad_rows([f0_transform(it["f0"], f0_min, use_log_f0, distance_tx) for it in its], Tmax, np.float32)
        out["p_voiced"] = pad_rows([it["p_voiced"] for it in its], Tmax, np.float32)
        out["voiced_mask"] = pad_rows([it["voiced_mask"] for it in its], Tmax, np.float32)
    out["audio"] = pad_rows([np.asarray(it["audio"]).astype(np.float32) * np.float32(1.0 / 32768.0) for it in its],
                            max(len(it["audio"]) for it in its), np.float32)[:, None]
    return out


def fixture_items(g):
    """the raw items of tests/golden/collate_small.npz, in the order the reference's DataLoader handed them over"""
    n = len([k for k in g if k.startswith("in.") and k.endswith(".audio")])
    items = []
    for i in range(n):
        ids, st = g[f"in.{i}.ids"], g[f"in.{i}.stats"]
        items.append({"audio": g[f"in.{i}.audio"], "text_encoded": g[f"in.{i}.text"], "f0": g[f"in.{i}.f0"],
                      "p_voiced": g[f"in.{i}.p_voiced"], "voiced_mask": g[f"in.{i}.voiced_mask"],
                      "speaker_id": int(ids[0]), "accent_id": int(ids[1]), "idx": int(ids[2]),
                      "speaker_f0_mean": float(st[0]), "speaker_f0_std": float(st[1]), "speaker_energy_mean": float(st[2]),
                      "speaker_energy_std": float(st[3]), "audiopath": f"wavs/{i}.wav", "text_raw": f"utterance {i}",
                      "language": "en_US"})
    return items
