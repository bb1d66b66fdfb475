#!/usr/bin/env python3
"""On-device batch builder benchmark (rad_mmm_amd.data.DeviceCollate, csrc/collate.hip): one JSON line.

    python tools/collate_bench.py [--iters 20] [--warmup 5] [--only new]

B = 32 utterances of 0.6-1.0 x 800 frames (hop 256, n_fft 1024, int16 samples, 90-150 tokens, pyin-like f0 tracks, drawn
from a seed).  Timed after warm-up, medians over the timed calls:
  new     DeviceCollate()(items): host_ms (the call returns: staging fill + enqueue), wall_ms (call + synchronise),
          device_ms (timing events around the copy and the kernels alone)
  loop    the loop a user of the package had to write before: per utterance mel_spectrogram + get_energy_average, torch
          padding, BetaBinomialInterpolator.batch, and the f0 transform in numpy on the host (tests/_collate_ref.py);
          host_ms / wall_ms the same way (it has no separable device clock: mel_spectrogram synchronises twice per
          utterance, so its device work is spread over the whole wall time)
--only new runs the new path alone (for a kernel trace: rocprofv3 --kernel-trace --stats -d out -- python
tools/collate_bench.py --only new)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

HOP, N_FFT, F0_MIN = 256, 1024, 80.0


def make_items(B=32, T=800, seed=1234):
    r = np.random.Generator(np.random.PCG64(seed))
    frames = np.sort(r.integers(int(0.6 * T), T + 1, size=B))[::-1].copy()
    frames[0] = T
    items = []
    for i, f in enumerate(frames):
        n = (int(f) - 1) * HOP + int(r.integers(0, HOP))
        audio = np.clip(np.round(0.2 * 32768 * r.standard_normal(n)), -32768, 32767).astype(np.int16)
        voiced = np.repeat(r.random(int(f) // 8 + 1) < 0.6, 8)[:int(f)]
        f0 = np.where(voiced, r.uniform(70.0, 300.0, int(f)), 0.0).astype(np.float32)
        items.append({"audio": audio, "text_encoded": r.integers(1, 185, int(r.integers(90, 151))), "f0": f0,
                      "p_voiced": r.random(int(f)).astype(np.float32), "voiced_mask": voiced.astype(np.float32),
                      "speaker_id": i % 8, "accent_id": i % 4, "idx": i, "speaker_f0_mean": 5.0, "speaker_f0_std": 0.3,
                      "speaker_energy_mean": 0.5, "speaker_energy_std": 0.1})
    r.shuffle(items)
    return items, int(frames.sum()), int(frames.max()) * B


def clocks(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    host, wall = [], []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        host.append(1e3 * (t1 - t0))
        wall.append(1e3 * (t2 - t0))
    return float(np.median(host)), float(np.median(wall)), float(np.min(wall)), float(np.max(wall))


def parent_loop(stft, prior, items, dev):
    """what the package offered before DeviceCollate, glued the obvious way"""
    import _collate_ref as R
    from rad_mmm_amd.data import get_energy_average
    order = torch.sort(torch.LongTensor([len(it["text_encoded"]) for it in items]), descending=True)[1].tolist()
    its = [items[i] for i in order]
    mels, ens = [], []
    for it in its:
        y = torch.from_numpy(it["audio"].astype(np.float32) / 32768.0)[None].to(dev)
        m = stft.mel_spectrogram(y)[0]
        mels.append(m)
        ens.append(get_energy_average(m))
    in_lens, out_lens = [len(it["text_encoded"]) for it in its], [m.shape[1] for m in mels]
    Tmax, Lmax, B = max(out_lens), max(in_lens), len(its)
    mel = torch.zeros(B, mels[0].shape[0], Tmax, device=dev)
    energy = torch.zeros(B, Tmax, device=dev)
    for b in range(B):
        mel[b, :, :out_lens[b]] = mels[b]
        energy[b, :out_lens[b]] = ens[b]
    f0 = torch.from_numpy(R.pad_rows([R.f0_transform(it["f0"], F0_MIN, True, True) for it in its], Tmax, np.float32)).to(dev)
    pv = torch.from_numpy(R.pad_rows([it["p_voiced"] for it in its], Tmax, np.float32)).to(dev)
    vm = torch.from_numpy(R.pad_rows([it["voiced_mask"] for it in its], Tmax, np.float32)).to(dev)
    text = torch.from_numpy(R.pad_rows([it["text_encoded"] for it in its], Lmax, np.int64)).to(dev)
    return {"mel": mel, "energy_avg": energy, "f0": f0, "p_voiced": pv, "voiced_mask": vm, "text": text,
            "attn_prior": prior.batch(in_lens, out_lens)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="", choices=["", "new"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("collate_bench needs an MI355X")
    from rad_mmm_amd.audio_processing import TacotronSTFT
    from rad_mmm_amd.data import BetaBinomialInterpolator, DeviceCollate
    dev = torch.device("cuda:0")
    stft = TacotronSTFT(N_FFT, HOP, N_FFT, 80, 22050, 0.0, 8000.0).to(dev)
    items, frames, padded = make_items()
    collate = DeviceCollate(stft, f0_min=F0_MIN, use_log_f0=True, distance_tx_unvoiced=True)
    out = {"metric": "collate_ms", "B": len(items), "frames": frames, "padded_frames": padded,
           "padding_row_share": 1.0 - frames / padded, "stft_gemm_gflop": 2e-9 * padded * N_FFT * (N_FFT + 2)}
    new = lambda: collate(items)
    h, w, wmin, wmax = clocks(new, args.iters, args.warmup)
    collate.timing_events = []
    for _ in range(args.iters):
        new()
    torch.cuda.synchronize()
    dev_ms = float(np.median([a.elapsed_time(b) for a, b in collate.timing_events]))
    collate.timing_events = None
    out["new"] = {"host_ms": h, "wall_ms": w, "wall_min_ms": wmin, "wall_max_ms": wmax, "device_ms": dev_ms}
    if not args.only:
        prior = BetaBinomialInterpolator(device=dev)
        loop = lambda: parent_loop(stft, prior, items, dev)
        # alternate the two paths once more, so that neither is favoured by the order
        h2, w2, w2min, w2max = clocks(loop, args.iters, args.warmup)
        h3, w3, _, _ = clocks(new, args.iters, 2)
        out["loop"] = {"host_ms": h2, "wall_ms": w2, "wall_min_ms": w2min, "wall_max_ms": w2max}
        out["new_again"] = {"host_ms": h3, "wall_ms": w3}
        out["loop_over_new_wall"] = w2 / max(w, w3)
        out["loop_over_new_host"] = h2 / max(h, h3)
        a, b = new(), loop()
        out["mel_identical_to_loop"] = bool(torch.equal(a["mel"], b["mel"])) and bool(torch.equal(a["energy_avg"], b["energy_avg"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
