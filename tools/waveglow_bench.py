#!/usr/bin/env python3
"""Batched WaveGlow benchmark (rad_mmm_amd/waveglow.py, csrc/waveglow.hip): one JSON line.

    python tools/waveglow_bench.py [--batch 32] [--frames 800] [--iters 3] [--warmup 1] [--analyze]
                                   [--precision {fp32,h3,f16}]
    python tools/waveglow_bench.py --train [--train-precision {fp32,h3}] [--batch 32] [--frames 800] [--iters 3]
                                   [--warmup 1]

The shipped config (12 flows, 8 layers, 256 channels, n_group 8, 80 mels), random weights from a seed, every item at
full length: device milliseconds of WaveGlow.infer (device events around the whole call, median after warm-up), audio
seconds per second at 22050 Hz, the time of each launch family (events around every launch of one extra call; the last
chunk of items only), and the in_layers row GEMMs' fraction of the fp32-MFMA peak (157.3 TFLOPS on
paper, MI355X).  --analyze adds the other direction in the same run and at the same shape: WaveGlow.analyze on seeded
audio, timed the same way, under "analyze" in the same JSON line with the ratio analyze / infer and the time of the
launch families only that direction has (group_audio, mix_fwd, end_coupling_fwd, nll_parts).  --precision h3 / f16 times
infer in that mode (WaveGlow.precision: the three WN GEMM families on the f16 matrix cores; split_cond is the one split
pass over the conditioning rows) and adds the relative L2 distance of its output to the fp32 mode's on the same noise;
the in_layers fraction stays relative to the fp32-MFMA peak in every mode, so that the modes compare on one scale.

--train times one training step instead, WaveGlow.nll_loss + backward in training mode with weight norm applied, at the
reference's training shape (batch 12, segments of 16000 samples = 62 frames) and at --batch / --frames: device
milliseconds per step, the ratio to analyze at the same shape in the same run, and the step's launch families (the
forward's, and bwd_* for the backward: bwd_recompute is the WN run again per flow; the last chunk of items only).
--train-precision h3 runs the step under WaveGlow.train_precision "h3" (the three WN GEMM families of every pass on the
f16 matrix cores, three products; the same families are timed, plus split_cond) and reports grad_saturated() after the
timed steps; compare it with an fp32 run of the same session."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

FP32_MFMA_PEAK = 157.3e12
SHIPPED = dict(n_mel_channels=80, n_flows=12, n_group=8, n_early_every=4, n_early_size=2,
               WN_config=dict(n_layers=8, n_channels=256, kernel_size=3))


def seeded_state(model, seed):
    """weights ~ N(0, 1 / fan_in) so that activations stay O(1) through 12 flows, biases ~ N(0, 0.1), end ~ N(0, 0.02)
    (the reference's zero end layers would skip the coupling's arithmetic), convinv orthogonal"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in model.state_dict().items():
        if k.startswith("convinv"):
            sd[k] = torch.linalg.qr(torch.randn(v.shape[0], v.shape[0], generator=g))[0].reshape(v.shape).contiguous()
        elif k.endswith("bias"):
            sd[k] = 0.1 * torch.randn(v.shape, generator=g)
        elif ".end." in k:
            sd[k] = 0.02 * torch.randn(v.shape, generator=g)
        elif k == "upsample.weight":
            sd[k] = torch.randn(v.shape, generator=g) / (4 * v.shape[0]) ** 0.5
        else:
            sd[k] = torch.randn(v.shape, generator=g) / (v.shape[1] * v.shape[2]) ** 0.5
    return sd


def timed_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), ts


def train_bench(model, args, dev):
    from rad_mmm_amd.waveglow import HOP
    model.apply_weight_norm()
    model.train_precision = args.train_precision
    shapes = []
    for B, T in ((12, 62), (args.batch, args.frames)):
        mel = (torch.randn(B, 80, T, generator=torch.Generator().manual_seed(6)) - 2.0).to(dev)
        audio = (0.3 * torch.randn(B, T * HOP, generator=torch.Generator().manual_seed(7))).to(dev)
        lens = [T] * B

        def step():
            model.zero_grad(set_to_none=True)
            with torch.enable_grad():
                model.nll_loss(mel, audio, lens).backward()
        model.eval()
        ms_a, ta = timed_ms(lambda: model.analyze(mel, audio, lens), args.iters, args.warmup)
        model.train()
        ms, ts = timed_ms(step, args.iters, args.warmup)
        model._train_events = events = {}
        step()
        torch.cuda.synchronize()
        model._train_events = None
        rows_chunk = events.pop("rows")
        fam = {k: sum(a.elapsed_time(b) for a, b in v) for k, v in events.items()}
        shapes.append({"batch": B, "frames": T, "rows": B * T * HOP // 8, "step_ms": ms, "all_ms": ts,
                       "analyze_ms": ms_a, "analyze_all_ms": ta, "ratio_to_analyze": ms / ms_a,
                       "last_chunk_rows": rows_chunk, "last_chunk_family_ms": fam,
                       "peak_memory_gib": torch.cuda.max_memory_allocated() / 2 ** 30})
        torch.cuda.reset_peak_memory_stats()
    print(json.dumps({"metric": "waveglow_train_step_ms", "train_precision": args.train_precision,
                      "grad_saturated": model.grad_saturated(), "shapes": shapes}))


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=800)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--once", action="store_true", help="one untimed call only (for a kernel trace)")
    ap.add_argument("--analyze", action="store_true", help="also time WaveGlow.analyze (audio -> latent) at the same shape")
    ap.add_argument("--train", action="store_true", help="time one training step (nll_loss + backward) instead")
    ap.add_argument("--precision", choices=("fp32", "h3", "f16"), default="fp32", help="WaveGlow.precision of infer")
    ap.add_argument("--train-precision", choices=("fp32", "h3"), default="fp32",
                    help="WaveGlow.train_precision of the --train step")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("waveglow_bench needs an MI355X")
    from rad_mmm_amd.waveglow import HOP, WaveGlow
    dev = torch.device("cuda:0")
    model = WaveGlow(**SHIPPED)
    model.load_state_dict(seeded_state(model, 5))
    model = model.to(dev).eval()
    model.precision = args.precision
    if args.train:
        return train_bench(model, args, dev)
    B, T = args.batch, args.frames
    mel = (torch.randn(B, 80, T, generator=torch.Generator().manual_seed(6)) - 2.0).to(dev)
    lens = [T] * B
    if args.once:
        model.infer(mel, lens, sigma=0.667)
        torch.cuda.synchronize()
        return
    for _ in range(args.warmup):
        model.infer(mel, lens, sigma=0.667)
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        model.infer(mel, lens, sigma=0.667)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ms = float(np.median(ts))
    events = {}
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    model._run(mel, lens_d, 0.667, None, events)
    torch.cuda.synchronize()
    rows_chunk = events.pop("rows")
    fam = {k: sum(a.elapsed_time(b) for a, b in v) for k, v in events.items()}
    n_in = len(events["in_layers"])
    wn = SHIPPED["WN_config"]
    C = wn["n_channels"]
    flop_in = 2.0 * 3 * C * 2 * C                       # per row and launch
    in_tflops = flop_in * n_in * rows_chunk / (fam["in_layers"] * 1e-3) / 1e12 if fam["in_layers"] else 0.0
    audio_s = B * T * HOP / 22050.0
    out = {"metric": "waveglow_infer_ms", "precision": args.precision, "batch": B, "frames": T, "device_ms": ms,
           "all_ms": ts,
           "audio_seconds": audio_s, "audio_seconds_per_second": audio_s / (ms * 1e-3),
           "last_chunk_family_ms": fam, "last_chunk_rows": rows_chunk, "rows": B * T * HOP // 8,
           "in_layers_tflops": in_tflops, "in_layers_frac_of_fp32_mfma_peak": in_tflops * 1e12 / FP32_MFMA_PEAK}
    if args.precision != "fp32":
        gen = torch.Generator(device=dev).manual_seed(11)
        noise = [torch.randn(B, ch, T * HOP // 8, device=dev, generator=gen) for ch in model.noise_shapes]
        ref = model.infer(mel, lens, sigma=0.667, noise=noise, precision="fp32").double()
        got = model.infer(mel, lens, sigma=0.667, noise=noise).double()
        out["rel_l2_vs_fp32"] = float((got - ref).norm() / ref.norm())
        del ref, got, noise
    if args.analyze:
        audio = (0.3 * torch.randn(B, T * HOP, generator=torch.Generator().manual_seed(7))).to(dev)
        for _ in range(args.warmup):
            model.analyze(mel, audio, lens)
        torch.cuda.synchronize()
        ta = []
        for _ in range(args.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            model.analyze(mel, audio, lens)
            e1.record()
            e1.synchronize()
            ta.append(e0.elapsed_time(e1))
        ms_a = float(np.median(ta))
        events = {}
        model._analyze_run(mel, audio, lens_d, False, events)
        torch.cuda.synchronize()
        events.pop("rows")
        fam_a = {k: sum(a.elapsed_time(b) for a, b in v) for k, v in events.items()}
        new = ("group_audio", "mix_fwd", "end_coupling_fwd", "nll_parts")
        out["analyze"] = {"device_ms": ms_a, "all_ms": ta, "ratio_to_infer": ms_a / ms, "last_chunk_family_ms": fam_a,
                          "new_families_ms": sum(fam_a[k] for k in new)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
