#!/usr/bin/env python3
"""Generate tests/golden/collate_small.npz by RUNNING THE REFERENCE's data path on procedural utterances.

Run in the build container only (needs the reference checkout):

    python tests/golden/make_golden_collate.py [--ref /root/reference]

Per utterance, in the order of AudioDataset.__getitem__ (data.py:419-610): get_mel on a
TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000), f0_normalize, the distance-transform lines (:527-532, the real
scipy.ndimage.distance_transform_edt), get_energy_average, BetaBinomialInterpolator; then DataCollate()(items)
(:616-790).  The methods run unbound on a SimpleNamespace that carries the few attributes they read: constructing the
dataset itself would need wav files, lmdb and the text processor.  Same stand-ins as make_golden.py (numba, librosa
helpers, the packages data.py imports without using them here); librosa.filters.mel, which TacotronSTFT calls, returns
`mel_22k` of tests/golden/mel_basis_hf.npz, the filterbank the project is pinned to.  Nothing of the reference's source
is written into this repo: the fixture holds the procedural inputs and the dictionary the reference collated.

Utterances: int16 sums of three gliding sines plus white noise at 0.06 of full scale (the noise floor keeps mel bins off
the 1e-5 clamp, where fp32 rounding of the reference itself would dominate), 0.35-0.7 s, two of the lengths multiples of
the hop; text lengths distinct but for one tie.  f0 tracks: voiced runs with unvoiced gaps of 1, 2 and 32 frames, an
unvoiced start and an unvoiced end, values on both sides of f0_min; every utterance has a voiced frame.  The voiced values
are float32 numbers whose log lies within 0.03 ulp of a float32 (robust_hz), and the distances' float64 logs are checked
to lie away from float32 rounding ties, so that the stored f0 does not depend on the log routine of the host that ran
this script.  The tracks are saved for both use_log_f0 and both distance_tx_unvoiced settings; the batch itself is
collated with both on.  A separate block ("unvoiced.*") holds what scipy gives an utterance WITHOUT any voiced frame
(DESIGN.md 4.18).
"""
import argparse
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

SR, N_FFT, HOP, N_MEL, F0_MIN, MAX_WAV = 22050, 1024, 256, 80, 80.0, 32768.0
SAMPLES = [256 * 30, 9001, 256 * 45, 13333, 15000, 15615]          # 31, 36, 46, 53, 59, 61 frames
TOKENS = [12, 9, 15, 9, 7, 11]                                     # items 1 and 3 tie
SPEAKERS, ACCENTS = [0, 2, 1, 1, 0, 2], [1, 0, 0, 1, 1, 0]
# (voiced?, frames) runs per utterance; the last run is stretched or cut to the utterance's frame count
RUNS = [
    [(0, 2), (1, 9), (0, 1), (1, 8), (0, 2), (1, 6), (0, 3)],
    [(1, 4), (0, 32)],                                             # voiced start, one long unvoiced tail
    [(0, 33), (1, 6), (0, 1), (1, 6)],                             # long unvoiced start, voiced end
    [(0, 3), (1, 5), (0, 1), (1, 4), (0, 2), (1, 6), (0, 30), (1, 2)],
    [(1, 20), (0, 2), (1, 1), (0, 1), (1, 30), (0, 5)],
    [(0, 3), (1, 5), (0, 1), (1, 4), (0, 2), (1, 6), (0, 32), (1, 5), (0, 3)],
]


def make_audio(rng, n):
    t = np.arange(n) / SR
    x = np.zeros(n)
    for _ in range(3):
        f_a, f_b = rng.uniform(90, 3500, 2)
        phase = 2 * np.pi * np.cumsum(np.linspace(f_a, f_b, n)) / SR + rng.uniform(0, 2 * np.pi)
        x += rng.uniform(0.08, 0.22) * np.sin(phase) * (0.6 + 0.4 * np.sin(2 * np.pi * rng.uniform(1, 4) * t))
    x += 0.06 * rng.standard_normal(n)
    return np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16)


def log_ulp_offset(x):
    """how far log(x) lies from the nearest float32, in units of float32's last place there (0 .. 0.5), for float32 x;
    measured in long double"""
    true = np.log(np.asarray(x, dtype=np.float32).astype(np.longdouble))
    near = true.astype(np.float32)
    return np.abs(true - near.astype(np.longdouble)) / np.spacing(np.abs(near)).astype(np.longdouble)


def robust_hz(rng, lo, hi):
    """a float32 in [lo, hi) whose log is within 0.03 ulp of a float32: every float32 log routine with an error below
    0.97 ulp returns that float.  The reference takes torch.log, whose result otherwise depends on the host's vector
    unit and on the element's position in the tensor (vector body or scalar tail); with such values the fixture is the
    same on every host, and the kernel's correctly rounded log must reproduce it exactly."""
    while True:
        c = rng.uniform(lo, hi, 64).astype(np.float32)
        ok = np.flatnonzero(log_ulp_offset(c) < 0.03)
        if ok.size:
            return c[ok[0]]


def make_tracks(rng, runs, frames):
    voiced = np.concatenate([np.full(n, v, dtype=bool) for v, n in runs])
    voiced = np.concatenate([voiced, np.full(max(0, frames - voiced.size), voiced[-1])])[:frames]
    f0 = np.zeros(frames, dtype=np.float32)
    for t in np.flatnonzero(voiced):
        f0[t] = robust_hz(rng, 60.0, 300.0)                                            # some voiced frames below f0_min
    f0[np.flatnonzero(voiced)[0]] = robust_hz(rng, 140.0, 160.0)                       # at least one frame above it
    p_voiced = rng.uniform(0.0, 1.0, frames).astype(np.float32)
    return f0, p_voiced, voiced.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    from make_golden import install_stubs, save, t2n
    install_stubs()
    basis = np.load(os.path.join(HERE, "mel_basis_hf.npz"))["mel_22k"]
    sys.modules["librosa.filters"].mel = lambda *a, **k: basis
    for name in ("lmdb", "parselmouth", "parselmouth.praat", "wave_transforms", "tts_text_processing",
                 "tts_text_processing.text_processing"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["librosa"].pyin = None
    sys.modules["parselmouth.praat"].call = None
    sys.modules["wave_transforms"].WaveAugmentations = None
    sys.modules["tts_text_processing.text_processing"].TextProcessing = None
    sys.path[:0] = [args.ref]
    cwd = os.getcwd()
    os.chdir("/tmp")
    import torch
    torch.set_num_threads(8)
    import data as ref_data
    from audio_processing import TacotronSTFT
    os.chdir(cwd)
    DS = ref_data.AudioDataset

    rng = np.random.Generator(np.random.PCG64(2024))
    stft = TacotronSTFT(N_FFT, HOP, N_FFT, N_MEL, SR, 0.0, 8000.0)
    interp = ref_data.BetaBinomialInterpolator()
    arrs = {"cfg": np.array([SR, N_FFT, HOP, N_MEL, F0_MIN, MAX_WAV])}
    raw = []
    for i, (n, L) in enumerate(zip(SAMPLES, TOKENS)):
        audio = make_audio(rng, n)
        f0, p_voiced, voiced_mask = make_tracks(rng, RUNS[i], 1 + n // HOP)
        text = rng.integers(1, 40, L).astype(np.int64)
        stats = rng.uniform(0.1, 6.0, 4).astype(np.float32)
        raw.append(dict(audio=audio, f0=f0, p_voiced=p_voiced, voiced_mask=voiced_mask, text=text, stats=stats))
        for k in ("audio", "f0", "p_voiced", "voiced_mask", "text", "stats"):
            arrs[f"in.{i}.{k}"] = raw[-1][k]
        arrs[f"in.{i}.ids"] = np.array([SPEAKERS[i], ACCENTS[i], 100 + i])

    def build_items(use_log_f0, dist_tx):
        ns = types.SimpleNamespace(max_wav_value=MAX_WAV, stft=stft, mel_noise_scale=0.0, use_log_f0=use_log_f0, f0_min=F0_MIN,
                                   use_scaled_energy=True)
        ns.energy_avg_normalize = lambda x: DS.energy_avg_normalize(ns, x)
        items = []
        for i, r in enumerate(raw):
            audio = torch.FloatTensor(r["audio"].astype(np.float32))          # load_wav_to_torch (data.py:107-109)
            mel = DS.get_mel(ns, audio)
            assert mel.shape == (N_MEL, 1 + len(r["audio"]) // HOP), mel.shape
            f0 = DS.f0_normalize(ns, torch.FloatTensor(r["f0"].copy()))
            if dist_tx:                                                       # data.py:527-532
                mask = f0 <= 0.0
                distance_map = np.log(ref_data.distance_transform(mask))
                distance_map[distance_map <= 0] = 0.0
                f0 = f0 - distance_map
            energy_avg = DS.get_energy_average(ns, mel)
            text = torch.LongTensor(r["text"])
            attn_prior = torch.tensor(interp(text.shape[0], mel.shape[1]))    # get_attention_prior (data.py:397-399)
            items.append({"mel": mel, "speaker_id": torch.LongTensor([SPEAKERS[i]]), "accent_id": torch.LongTensor([ACCENTS[i]]),
                          "text_raw": f"utterance {i}", "language": "en_US", "text_encoded": text, "audiopath": f"wavs/{i}.wav",
                          "attn_prior": attn_prior, "f0": f0, "p_voiced": torch.FloatTensor(r["p_voiced"]),
                          "voiced_mask": torch.FloatTensor(r["voiced_mask"]), "energy_avg": energy_avg, "idx": 100 + i,
                          "speaker_f0_mean": float(r["stats"][0]), "speaker_f0_std": float(r["stats"][1]),
                          "speaker_energy_mean": float(r["stats"][2]), "speaker_energy_std": float(r["stats"][3]),
                          "audio": audio[None] / MAX_WAV})
        return items

    with torch.no_grad():
        for use_log_f0 in (True, False):
            for dist_tx in (True, False):
                out = ref_data.DataCollate()(build_items(use_log_f0, dist_tx))
                arrs[f"f0.log{int(use_log_f0)}.dtx{int(dist_tx)}"] = out["f0"]
                if use_log_f0 and dist_tx:
                    for k, v in out.items():
                        if k == "audio":
                            continue                                          # = in.*.audio / MAX_WAV, zero padded: not stored
                        if torch.is_tensor(v):
                            arrs[f"batch.{k}"] = v
                    arrs["lists.audiopaths"] = np.array(out["audiopaths"])
                    arrs["lists.text_raw"] = np.array(out["text_raw"])
                    arrs["lists.language"] = np.array(out["language"])
        # an utterance without any voiced frame: scipy's transform has no background to measure from
        T0 = 7
        arrs["unvoiced.edt"] = ref_data.distance_transform(np.ones(T0, dtype=bool))
        ns = types.SimpleNamespace(use_log_f0=True, f0_min=F0_MIN)
        f0 = DS.f0_normalize(ns, torch.FloatTensor(np.array([0, 0, 40.0, 0, 0, 79.0, 0], dtype=np.float32)))
        arrs["unvoiced.f0_in"] = np.array([0, 0, 40.0, 0, 0, 79.0, 0], dtype=np.float32)
        distance_map = np.log(ref_data.distance_transform(f0 <= 0.0))
        distance_map[distance_map <= 0] = 0.0
        arrs["unvoiced.f0_out"] = torch.FloatTensor(T0).copy_(f0 - distance_map)
    # the distance term: -log(d) rounded to float32 must not hinge on the last bits of the host's float64 log
    d = np.arange(2, 64, dtype=np.float64).astype(np.longdouble)
    true = np.log(d)
    near = true.astype(np.float64).astype(np.float32)
    off = np.abs(true - near.astype(np.longdouble)) / np.spacing(near).astype(np.longdouble)
    assert np.all(off < 0.499), "a distance whose log is a float32 rounding tie"
    for i in range(len(raw)):
        v = raw[i]["f0"]
        assert np.all(log_ulp_offset(v[v >= F0_MIN]) < 0.03)
    import scipy
    arrs["scipy_version"] = np.array(scipy.__version__)
    save("collate_small.npz", **t2n(arrs))


if __name__ == "__main__":
    main()
