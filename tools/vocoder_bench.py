#!/usr/bin/env python3
"""Batched HiFi-GAN vocoder benchmark (rad_mmm_amd/vocoder.py): one JSON line.

    python tools/vocoder_bench.py [--iters 5] [--warmup 2] [--no-torch]

Generator and denoiser ms per call at (B, T) = (32, 800) and (1, 800) for the V1 and V3 configs (random weights
from a seed), the real-time factor (seconds of 22.05 kHz audio per second of compute), per-stage ms of the generator
with its FLOP, bytes and the fraction of the binding roof, and a side leg: the same generator written with stock
torch.nn.functional fp32 convs on the same GPU.  Device events around each call, after warm-up."""
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
from rad_mmm_amd.vocoder import Denoiser, HiFiGANGenerator  # noqa: E402

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


def torch_generator(cfg, sd, dev):
    """the same generator with stock torch.nn.functional fp32 convs (weight norm folded once)"""
    g = HiFiGANGenerator(cfg)
    g.load_state_dict(sd)
    g.remove_weight_norm()
    g = g.to(dev)

    def run(mel):
        x = F.conv1d(mel, g.conv_pre.weight, g.conv_pre.bias, padding=3)
        for i, up in enumerate(g.ups):
            x = F.leaky_relu(x, 0.1)
            x = F.conv_transpose1d(x, up.weight, up.bias, stride=up.stride, padding=up.padding)
            xs = None
            for blk in g.resblocks[i]:
                y = x
                if hasattr(blk, "convs1"):
                    for c1, c2 in zip(blk.convs1, blk.convs2):
                        t = F.leaky_relu(y, 0.1)
                        t = F.conv1d(t, c1.weight, c1.bias, dilation=c1.dilation, padding=c1.padding)
                        t = F.leaky_relu(t, 0.1)
                        t = F.conv1d(t, c2.weight, c2.bias, dilation=c2.dilation, padding=c2.padding)
                        y = t + y
                else:
                    for c in blk.convs:
                        t = F.conv1d(F.leaky_relu(y, 0.1), c.weight, c.bias, dilation=c.dilation, padding=c.padding)
                        y = t + y
                xs = y if xs is None else xs + y
            x = xs / len(g.resblocks[i])
        x = F.leaky_relu(x)
        return torch.tanh(F.conv1d(x, g.conv_post.weight, g.conv_post.bias, padding=3))
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
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
