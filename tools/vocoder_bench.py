#!/usr/bin/env python3
"""Batched HiFi-GAN vocoder benchmark (rad_mmm_amd/vocoder.py): one JSON line.

    python tools/vocoder_bench.py [--iters 5] [--warmup 2] [--no-torch]
    python tools/vocoder_bench.py --train [--iters 5] [--warmup 2]

Generator and denoiser ms per call at (B, T) = (32, 800) and (1, 800) for the V1 and V3 configs (random weights
from a seed), the real-time factor (seconds of 22.05 kHz audio per second of compute), per-stage ms of the generator
with its FLOP, bytes and the fraction of the binding roof, and a side leg: the same generator written with stock
torch.nn.functional fp32 convs on the same GPU.  Device events around each call, after warm-up.

--train: one training step of V1 (forward, a fixed quadratic loss on the audio, backward; weight norm on, as a
training checkpoint) at upstream HiFi-GAN's training shape, batch 16 x 32 frames (8192 samples), and at batch 32 x 32
frames, through the HIP backward and, in the same process, through the stock path: the same generator written with
torch.nn.functional in fp32 and trained by torch autograd.  One JSON line with both times, their ratio and the peak
allocated bytes of each."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from _vocoder_ref import V1, V3, random_state  # noqa: E402
from rad_mmm_amd.vocoder import Denoiser, HiFiGANGenerator, fold_weight_norm  # noqa: E402

SR = 22050
FP32_MFMA_TF = 157.3     # v_mfma_f32_32x32x2_f32, MI355X
HBM_TBS = 8.0


def timed(fn, iters, warmup):
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
    return float(np.median(ts))


def stage_costs(gen, cfg, B, T):
    """FLOP and HBM bytes (fp32 tensors read/written by each launch) per stage: conv_pre, stages, conv_post"""
    c0 = cfg["upsample_initial_channel"]
    rows = B * T
    out = [("conv_pre", 2.0 * rows * 80 * c0 * 7, 4.0 * rows * (80 + c0))]
    C = c0
    for i, u in enumerate(cfg["upsample_rates"]):
        k = cfg["upsample_kernel_sizes"][i]
        flop = 2.0 * rows * C * (C // 2) * k
        byt = 4.0 * rows * C * 3 + 4.0 * rows * u * (C // 2)
        rows *= u
        C //= 2
        for blk in gen.resblocks[i]:
            for m in blk.modules():
                if isinstance(m, torch.nn.Conv1d):
                    flop += 2.0 * rows * C * C * m.kernel_size[0]
                    byt += 4.0 * rows * C * 5          # lrelu copy (r+w), conv operand read, residual read, output write
        out.append((f"stage{i + 1}", flop, byt))
    out.append(("conv_post", 2.0 * rows * C * 7, 4.0 * rows * (C + 1)))
    return out


def torch_generator(cfg, sd, dev, g=None):
    """the same generator with stock torch.nn.functional fp32 convs (weight norm folded once); g: a weight-normed
    module to train instead (every weight is then folded from weight_g / weight_v with torch ops in each call, under
    autograd)"""
    if g is None:
        g = HiFiGANGenerator(cfg)
        g.load_state_dict(sd)
        g.remove_weight_norm()
        g = g.to(dev)

    def wt(m):
        return fold_weight_norm(m.weight_v, m.weight_g) if hasattr(m, "weight_g") else m.weight

    def run(mel):
        x = F.conv1d(mel, wt(g.conv_pre), g.conv_pre.bias, padding=3)
        for i, up in enumerate(g.ups):
            x = F.leaky_relu(x, 0.1)
            x = F.conv_transpose1d(x, wt(up), up.bias, stride=up.stride, padding=up.padding)
            xs = None
            for blk in g.resblocks[i]:
                y = x
                if hasattr(blk, "convs1"):
                    for c1, c2 in zip(blk.convs1, blk.convs2):
                        t = F.leaky_relu(y, 0.1)
                        t = F.conv1d(t, wt(c1), c1.bias, dilation=c1.dilation, padding=c1.padding)
                        t = F.leaky_relu(t, 0.1)
                        t = F.conv1d(t, wt(c2), c2.bias, dilation=c2.dilation, padding=c2.padding)
                        y = t + y
                else:
                    for c in blk.convs:
                        t = F.conv1d(F.leaky_relu(y, 0.1), wt(c), c.bias, dilation=c.dilation, padding=c.padding)
                        y = t + y
                xs = y if xs is None else xs + y
            x = xs / len(g.resblocks[i])
        x = F.leaky_relu(x)
        return torch.tanh(F.conv1d(x, wt(g.conv_post), g.conv_post.bias, padding=3))
    return run


def train_bench(args, dev):
    res = {"metric": "hifigan_train_step_ms", "config": "V1", "frames": 32, "iters": args.iters, "warmup": args.warmup,
           "note": "one GPU, one process, one session: both paths timed in turn at each shape", "shapes": {}}
    gen = HiFiGANGenerator(V1)
    sd = random_state(gen, 5, 0.2, 0.6)
    gen.load_state_dict(sd)
    gen = gen.to(dev).train()
    stock = HiFiGANGenerator(V1)
    stock.load_state_dict(sd)
    stock = stock.to(dev).train()
    run_stock = torch_generator(V1, sd, dev, stock)
    g = torch.Generator().manual_seed(6)
    for B in (16, 32):
        T = 32
        mel = (torch.randn(B, 80, T, generator=g) - 2.0).to(dev)
        target = (torch.rand(B, 1, T * gen.hop, generator=g) * 2 - 1).to(dev)
        lens = [T] * B

        def step(model, fwd):
            model.zero_grad(set_to_none=True)
            ((fwd(mel) - target) ** 2).mean().backward()
        row = {}
        for key, model, fwd in (("hip", gen, lambda m: gen(m, lens)), ("torch_fp32", stock, run_stock)):
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            row[key + "_step_ms"] = round(timed(lambda: step(model, fwd), args.iters, args.warmup), 3)
            row[key + "_peak_bytes"] = int(torch.cuda.max_memory_allocated() - base)
        row["torch_over_hip"] = round(row["torch_fp32_step_ms"] / row["hip_step_ms"], 3)
        gw, sw = gen.conv_pre.weight_v.grad, stock.conv_pre.weight_v.grad
        row["conv_pre_weight_v_grad_rel_l2"] = float((gw - sw).norm() / sw.norm())
        res["shapes"][f"B{B}_T{T}"] = row
        print(json.dumps({f"B{B}_T{T}": row}), file=sys.stderr, flush=True)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--train", action="store_true", help="time one V1 training step against stock torch autograd")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    if args.train:
        return train_bench(args, dev)
    res = {"metric": "vocoder_ms", "configs": {}}
    for name, cfg in (("V1", V1), ("V3", V3)):
        gen = HiFiGANGenerator(cfg)
        sd = random_state(gen, 5, 0.2, 0.6)
        gen.load_state_dict(sd)
        gen = gen.to(dev).eval()
        den = Denoiser(gen).to(dev)
        g = torch.Generator().manual_seed(6)
        for B, T in ((32, 800), (1, 800)):
            mel = (torch.randn(B, 80, T, generator=g) - 2.0).to(dev)
            lens = [T] * B
            audio = gen(mel, lens)[:, 0].contiguous()
            s_lens = [T * gen.hop] * B
            gms = timed(lambda: gen(mel, lens), args.iters, args.warmup)
            dms = timed(lambda: den(audio, 0.001, s_lens), args.iters, args.warmup)
            secs = B * T * gen.hop / SR
            row = {"generator_ms": round(gms, 3), "denoiser_ms": round(dms, 3),
                   "rtf": round(secs / ((gms + dms) / 1e3), 1), "audio_s": round(secs, 2),
                   "generator_tflop": round(sum(c[1] for c in stage_costs(gen, cfg, B, T)) / 1e12, 3)}
            # per-stage: device events between the stages of one call
            ev = []
            lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
            for _ in range(2):
                ev = []
                gen._run(mel, lens_d, ev)
            torch.cuda.synchronize()
            stages = []
            for (sname, flop, byt), e0, e1 in zip(stage_costs(gen, cfg, B, T), ev[:-1], ev[1:]):
                ms = e0.elapsed_time(e1)
                t_c, t_m = flop / (FP32_MFMA_TF * 1e12), byt / (HBM_TBS * 1e12)
                roof = "fp32_mfma" if t_c >= t_m else "hbm"
                stages.append({"stage": sname, "ms": round(ms, 3), "gflop": round(flop / 1e9, 1),
                               "mbytes": round(byt / 1e6, 1), "roof": roof,
                               "roof_fraction": round(max(t_c, t_m) * 1e3 / ms, 3) if ms > 0 else None})
            row["stages"] = stages
            if not args.no_torch:
                run = torch_generator(cfg, sd, dev)
                with torch.no_grad():
                    try:
                        tms = timed(lambda: run(mel), max(2, args.iters // 2), 1)
                        y_t = run(mel)[:, 0]
                        row["torch_fp32_generator_ms"] = round(tms, 3)
                        row["speedup_vs_torch"] = round(tms / gms, 2)
                        row["torch_max_abs_diff"] = float((y_t - gen(mel, lens)[:, 0]).abs().max())
                    except Exception as e:           # e.g. out of memory of the stock path at the full batch
                        row["torch_fp32_generator_ms"] = None
                        row["torch_error"] = str(e)[:200]
                torch.cuda.empty_cache()
            res["configs"][f"{name}_B{B}_T{T}"] = row
            print(json.dumps({f"{name}_B{B}_T{T}": row}), file=sys.stderr, flush=True)
            del audio
            torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
