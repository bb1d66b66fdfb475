#!/usr/bin/env python3
"""Batched HiFi-GAN vocoder benchmark (rad_mmm_amd/vocoder.py): one JSON line.

    python tools/vocoder_bench.py [--iters 5] [--warmup 2] [--no-torch] [--precision {fp32,f16}] [--config V1|V3]
                                  [--shape BxT]
    python tools/vocoder_bench.py --train [--iters 5] [--warmup 2]
    python tools/vocoder_bench.py --stft-loss [--iters 5] [--warmup 2] [--out profiles/stft_loss.json]
    python tools/vocoder_bench.py --mel-loss [--iters 5] [--warmup 2] [--out profiles/mel_loss.json]
    python tools/vocoder_bench.py --mpd [--iters 5] [--warmup 2] [--out profiles/mpd.json]
    python tools/vocoder_bench.py --mpd --precision h3 [--out profiles/mpd_h3.json]
    python tools/vocoder_bench.py --gan-step --mpd-precision h3 [--out profiles/mpd_h3.json]
    python tools/vocoder_bench.py --msd [--iters 5] [--warmup 2] [--out profiles/msd.json]
    python tools/vocoder_bench.py --gan-step [--iters 5] [--warmup 2] [--out profiles/hifigan_gan_step.json]

Generator and denoiser ms per call at (B, T) = (32, 800) and (1, 800) for the V1 and V3 configs (random weights
from a seed), the real-time factor (seconds of 22.05 kHz audio per second of compute), per-stage ms of the generator
with its FLOP, bytes and the fraction of the binding roof, and a side leg: the same generator written with stock
torch.nn.functional fp32 convs on the same GPU.  Device events around each call, after warm-up.  --precision f16 runs
the generator in its f16 mode (HiFiGANGenerator.precision): a stage on radmmm_voc_conv_f16 is held against the f16 MFMA
roof and its bytes count no leaky-relu copies; the row also carries the audio's rel-L2 distance from the fp32 mode.
--config / --shape restrict the run to one config or one (B, T) (the workload of a kernel trace).

--train: one training step of V1 (forward, a fixed quadratic loss on the audio, backward; weight norm on, as a
training checkpoint) at upstream HiFi-GAN's training shape, batch 16 x 32 frames (8192 samples), and at batch 32 x 32
frames, through the HIP backward and, in the same process, through the stock path: the same generator written with
torch.nn.functional in fp32 and trained by torch autograd.  One JSON line with both times, their ratio and the peak
allocated bytes of each.

--stft-loss: the multi-resolution STFT loss (rad_mmm_amd/stft_loss.py, the default three resolutions, ragged
len_ratios on the device), forward plus backward with respect to the prediction, at 16 x 8192 and 32 x 8192 samples, in
one process: the HIP module, a stock-torch implementation with torch.stft and vectorised masking (no per-item loop, no
host read: the strongest stock alternative) and the per-item loop as the reference writes it.  Median of --iters runs
after --warmup; per form the device launches of one step (torch.profiler) and the host synchronisations
(torch.cuda.set_sync_debug_mode("warn")).  Then the V1 training step of --train with this loss in place of the quadratic
one (HIP generator; HIP loss, stock vectorised loss, and the quadratic loss for scale).  The JSON also goes to --out.

--mel-loss: the mel L1 loss (rad_mmm_amd/mel_loss.py, TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000), ragged sample
counts on the device), forward plus backward with respect to the prediction, at 16 x 8192 and 32 x 8192 samples, in one
process, against the same loss written with torch.stft and vectorised masking in fp32.  Per-item reflection is impossible
for that stock form without a loop over the items, so it reflects every item at the padded length S (torch.stft
center=True) and masks the frames past 1 + lens[b] // hop: an item's last n_fft / (2 hop) = 2 frames see the zeros behind
it instead of its mirror image; and it takes sqrt(re^2 + im^2 + 1e-9), as upstream HiFi-GAN's mel does, because torch's
gradient of sqrt at the all-zero frames behind an item is NaN, which masking cannot remove.  Median of --iters runs after
--warmup, device launches and host synchronisations of one step as for --stft-loss.  Then the V1 training step of --train
with 45 * mel + sc + mag (HIP STFT loss in both) through the HIP mel loss and through the stock one.  The JSON also goes
to --out.

--mpd: the multi-period discriminator and its GAN losses (rad_mmm_amd/discriminators.py, the reference's widths, ragged
len_ratios on the device) at 16 x 8192 and 32 x 8192 samples, in one process: the D step (discriminator loss forward plus
parameter gradients, y_hat detached) and the G side (feature + generator loss forward plus the gradient of y_hat, parameters
frozen), through the HIP module, through the same discriminator written with torch.nn.functional.conv2d in fp32 under torch
autograd (real and generated audio stacked in one pass, vectorised masks, no host read), and through the reference's form
(one pass per signal, its mask builder's and gan_discriminator_loss's .item() calls).  Each stock step computes only the
losses of that step: the D step the discriminator loss, the G side the feature and generator losses.  Per form and
step: median ms of --iters runs after --warmup, device launches, host synchronisations, peak allocated memory.  The JSON
also goes to --out (profiles/mpd.json).

--mpd --precision h3: MultiPeriodDiscriminator.precision "h3" (leg b) against "fp32" (leg a: the code path, launches and
bits the module had before the mode existed) on the same batches, order a b b a, one fresh process per leg, median of
--iters after --warmup: per leg and step both runs' ms, their spread, launches, host synchronisations, peak allocated
memory, and for "h3" the relative L2 of its gradients against the fp32 mode's, to profiles/mpd_h3.json.  With
--d-step-only: the "h3" D step at 32 x 8192 alone, the workload of profiles/mpd_h3_d_step_kernel_stats.csv.
--gan-step --mpd-precision h3: HiFiGANTrainingStep(mpd_precision="h3") against "fp32" in the same way, added to that file
under "gan_step".

--msd: the same for the multi-scale discriminator (the reference's widths and groups, training mode) against stock torch
with conv1d(groups=), to profiles/msd.json; --msd --d-step-only runs the module's D step at 32 x 8192 alone, the workload
of the kernel trace kept as profiles/msd_d_step_kernel_stats.csv.

--gan-step: the whole HiFi-GAN fine-tuning step (V1, the default discriminators, the default three STFT resolutions, mel
weight 45) at 16 x 32 and 32 x 32 frames (8192 samples) with ragged lens.  Leg a: rad_mmm_amd.vocoder_step.
HiFiGANTrainingStep (two fused FlatAdam, the discriminators frozen during the G side).  Leg b: the README recipe as it is
written, on the same modules, with two torch.optim.AdamW; its process then also times the recipe with the discriminators'
parameters frozen during the G side (b_frozen), which isolates the optimizers.  Order a b b a, one fresh process per leg
(the parent never opens the GPU), median of --iters steps after --warmup; per leg ms per step, device launches, host
synchronisations and peak allocated memory.  The JSON also goes to --out."""
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
F16_MFMA_TF = 2500.0     # v_mfma_f32_32x32x16_f16, dense peak
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


def stage_costs(gen, cfg, B, T, plan=None):
    """FLOP and HBM bytes (fp32 tensors read/written by each launch) per stage: conv_pre, stages, conv_post.  plan: the
    modes per stage (HiFiGANGenerator.precision_plan); an "f16" stage has no leaky-relu copies"""
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
                    # lrelu copy (r+w), conv operand read, residual read, output write; f16: the copy is fused into the load
                    byt += 4.0 * rows * C * (3 if plan and plan[i][0] == "f16" else 5)
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


def stock_stft_losses(fft_sizes, hop_sizes, win_lengths, dev):
    """(vectorised, per-item loop): the reference's loss written with stock torch ops.  vectorised masks the frames
    past ceil(len_ratios * F) instead of slicing them, so nothing is read back; loop slices every item at lens[i] as
    stft_loss.py:136-143 does."""
    windows = [torch.hann_window(w, device=dev) for w in win_lengths]

    def mags(sig, n_fft, hop, win, window):
        z = torch.stft(sig, n_fft, hop, win, window, return_complex=True)
        return torch.sqrt(torch.clamp(z.real ** 2 + z.imag ** 2, min=1e-7)).transpose(2, 1)

    def vectorised(x, y, ratios):
        sc = mag = 0.0
        for n_fft, hop, win, window in zip(fft_sizes, hop_sizes, win_lengths, windows):
            xm, ym = mags(x, n_fft, hop, win, window), mags(y, n_fft, hop, win, window)
            frames = (ratios * ym.shape[1]).ceil()
            mask = (torch.arange(ym.shape[1], device=dev)[None, :] < frames[:, None]).to(ym.dtype)
            total = frames.sum()
            sc = sc + (torch.linalg.vector_norm(ym - xm, dim=2) / torch.linalg.vector_norm(ym, dim=2) * mask).sum() / total
            mag = mag + ((torch.log(ym) - torch.log(xm)).abs() * mask[..., None]).sum() / (total * ym.shape[2])
        return sc / len(fft_sizes), mag / len(fft_sizes)

    def loop(x, y, ratios):
        sc = mag = 0.0
        for n_fft, hop, win, window in zip(fft_sizes, hop_sizes, win_lengths, windows):
            xm, ym = mags(x, n_fft, hop, win, window), mags(y, n_fft, hop, win, window)
            lens = (ratios * ym.shape[1]).ceil().long()
            loss = 0.0
            for i in range(len(ym)):
                y_i, x_i = ym[i, :lens[i]], xm[i, :lens[i]]
                loss = loss + (torch.norm(y_i - x_i, dim=1, p="fro") / torch.norm(y_i, dim=1, p="fro")).sum()
            sc = sc + loss / lens.sum()
            mask = (torch.arange(ym.shape[1], device=dev)[None, :] < lens[:, None])[..., None]
            mag = mag + ((torch.log(ym) - torch.log(xm)).abs() * mask).sum() / (mask.sum() * ym.shape[2])
        return sc / len(fft_sizes), mag / len(fft_sizes)
    return vectorised, loop


def count_launches_and_syncs(fn):
    """(device launches of one call, host synchronisations of one call); None where the count could not be taken"""
    import warnings
    launches = syncs = None
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        launches = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as e:
        print(f"launch count failed: {e}", file=sys.stderr)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            fn()
        syncs = sum(1 for w in seen if "synchroniz" in str(w.message).lower())
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return launches, syncs


def stft_loss_bench(args, dev):
    from rad_mmm_amd.stft_loss import MultiResolutionSTFTLoss
    fft, hop, win = [1024, 2048, 512], [120, 240, 50], [600, 1200, 240]
    hip = MultiResolutionSTFTLoss(fft, hop, win).to(dev)
    vectorised, loop = stock_stft_losses(fft, hop, win, dev)
    res = {"metric": "stft_loss_fwd_bwd_ms", "resolutions": {"fft": fft, "hop": hop, "win": win}, "iters": args.iters,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "note": "one GPU, one process, one session; forward + backward with respect to the prediction; ragged "
                   "len_ratios on the device; median of iters after warmup", "shapes": {}}
    g = torch.Generator().manual_seed(11)
    for B in (16, 32):
        T = 8192
        lengths = torch.linspace(T // 3, T, B).round()
        ratios = (lengths / T).to(dev)
        keep = (torch.arange(T)[None, :] < lengths[:, None]).float()
        target = (torch.randn(B, T, generator=g) * keep).to(dev)
        pred = ((target.cpu() + 0.3 * torch.randn(B, T, generator=g)) * keep).to(dev)
        row = {}
        grads = {}
        for key, fn in (("hip", hip), ("torch_vectorised", vectorised), ("torch_item_loop", loop)):
            def step():
                p = pred.detach().requires_grad_(True)
                sc, mag = fn(p, target, ratios)
                (sc + mag).backward()
                return sc.detach(), mag.detach(), p.grad
            ms = timed(step, args.iters, args.warmup)
            launches, syncs = count_launches_and_syncs(step)
            sc, mag, grads[key] = step()
            row[key] = {"fwd_bwd_ms": round(ms, 3), "launches": launches, "host_syncs": syncs, "sc": float(sc),
                        "mag": float(mag)}
        for key in ("torch_vectorised", "torch_item_loop"):
            row[key]["over_hip"] = round(row[key]["fwd_bwd_ms"] / row["hip"]["fwd_bwd_ms"], 3)
            row[key]["grad_rel_l2_vs_hip"] = float((grads[key] - grads["hip"]).norm() / grads["hip"].norm())
        res["shapes"][f"B{B}_T{T}"] = row
        print(json.dumps({f"B{B}_T{T}": row}), file=sys.stderr, flush=True)
    # the V1 training step of --train with this loss in place of the quadratic one
    gen = HiFiGANGenerator(V1)
    gen.load_state_dict(random_state(gen, 5, 0.2, 0.6))
    gen = gen.to(dev).train()
    res["train_step"] = {}
    for B in (16, 32):
        Tm = 32
        S = Tm * gen.hop
        mel = (torch.randn(B, 80, Tm, generator=g) - 2.0).to(dev)
        target = (torch.rand(B, S, generator=g) * 2 - 1).to(dev)
        ratios = (torch.linspace(S // 3, S, B).round() / S).to(dev)
        lens = [Tm] * B
        row = {}
        for key, loss in (("hip_stft_loss", lambda a: sum(hip(a, target, ratios))),
                          ("torch_vectorised_stft_loss", lambda a: sum(vectorised(a, target, ratios))),
                          ("quadratic_loss", lambda a: ((a - target) ** 2).mean())):
            def step():
                gen.zero_grad(set_to_none=True)
                loss(gen(mel, lens)[:, 0]).backward()
            row[key + "_step_ms"] = round(timed(step, args.iters, args.warmup), 3)
        res["train_step"][f"B{B}_T{Tm}"] = row
        print(json.dumps({f"train_B{B}_T{Tm}": row}), file=sys.stderr, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    print(json.dumps(res))


def stock_mel_loss(stft, dev):
    """the mel L1 loss with torch.stft and vectorised masking in fp32 (see the module docstring for its two approximations)"""
    s = stft.stft_fn
    n_fft, hop, win = s.filter_length, s.hop_length, s.win_length
    window = torch.hann_window(win, device=dev)
    mel_basis = stft.mel_basis

    def fn(x, target, lens, frames=None):
        z = torch.stft(x, n_fft, hop, win, window, center=True, pad_mode="reflect", return_complex=True)
        mag = torch.sqrt(z.real ** 2 + z.imag ** 2 + 1e-9)
        mel = torch.log(torch.clamp(torch.matmul(mel_basis, mag), min=1e-5))
        k = min(mel.shape[2], target.shape[2])
        n = torch.clamp(1 + torch.div(lens, hop, rounding_mode="floor"), max=k)
        if frames is not None:
            n = torch.minimum(n, torch.clamp(frames, min=0, max=k))
        mask = (torch.arange(k, device=dev)[None, :] < n[:, None]).to(mel.dtype)[:, None, :]
        return ((mel[:, :, :k] - target[:, :, :k]).abs() * mask).sum() / (mel.shape[1] * n.sum())
    return fn


def mel_loss_bench(args, dev):
    from rad_mmm_amd.mel_loss import MelSpectrogramLoss, mel_spectrogram
    from rad_mmm_amd.stft_loss import MultiResolutionSTFTLoss
    hip = MelSpectrogramLoss().to(dev)
    stock = stock_mel_loss(hip.stft, dev)
    hop = hip.stft.stft_fn.hop_length
    res = {"metric": "mel_loss_fwd_bwd_ms", "stft": [1024, 256, 1024, 80, 22050, 0.0, 8000.0], "iters": args.iters,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "note": "one GPU, one process, one session; forward + backward with respect to the prediction; ragged sample "
                   "counts on the device; median of iters after warmup.  torch_vectorised reflects at the padded length and "
                   "adds 1e-9 under the square root (tools/vocoder_bench.py docstring), so its loss and gradient differ from "
                   "the HIP module's by that approximation", "shapes": {}}
    g = torch.Generator().manual_seed(12)
    for B in (16, 32):
        S = 8192
        lengths = torch.linspace(S // 3, S, B).round().long()
        lens = lengths.to(dev)
        keep = (torch.arange(S)[None, :] < lengths[:, None]).float()
        clean = (0.3 * torch.randn(B, S, generator=g) * keep).to(dev)
        pred = ((clean.cpu() + 0.1 * torch.randn(B, S, generator=g)) * keep).clamp(-1, 1).to(dev)
        with torch.no_grad():
            target = mel_spectrogram(clean, hip.stft, lens)
        row, grads = {}, {}
        for key, fn in (("hip", hip), ("torch_vectorised", stock)):
            def step():
                p = pred.detach().requires_grad_(True)
                loss = fn(p, target, lens)
                loss.backward()
                return loss.detach(), p.grad
            ms = timed(step, args.iters, args.warmup)
            launches, syncs = count_launches_and_syncs(step)
            loss, grads[key] = step()
            row[key] = {"fwd_bwd_ms": round(ms, 3), "launches": launches, "host_syncs": syncs, "loss": float(loss)}
        row["torch_vectorised"]["over_hip"] = round(row["torch_vectorised"]["fwd_bwd_ms"] / row["hip"]["fwd_bwd_ms"], 3)
        row["torch_vectorised"]["grad_rel_l2_vs_hip"] = float((grads["torch_vectorised"] - grads["hip"]).norm() / grads["hip"].norm())
        res["shapes"][f"B{B}_S{S}"] = row
        print(json.dumps({f"B{B}_S{S}": row}), file=sys.stderr, flush=True)
    # the V1 training step of --train with 45 * mel + sc + mag (HIP STFT loss in both forms)
    gen = HiFiGANGenerator(V1)
    gen.load_state_dict(random_state(gen, 5, 0.2, 0.6))
    gen = gen.to(dev).train()
    stft_loss = MultiResolutionSTFTLoss().to(dev)
    res["train_step"] = {}
    for B in (16, 32):
        Tm = 32
        S = Tm * gen.hop
        mel = (torch.randn(B, 80, Tm, generator=g) - 2.0).to(dev)
        target = (torch.rand(B, S, generator=g) * 2 - 1).to(dev)
        lens = torch.linspace(Tm // 3, Tm, B).round().long().tolist()
        frames = torch.tensor(lens, device=dev, dtype=torch.int32)
        samples = frames * gen.hop
        ratios = samples.float() / S
        row = {}
        for key, mel_fn in (("hip_mel_loss", hip), ("torch_vectorised_mel_loss", stock)):
            def step():
                gen.zero_grad(set_to_none=True)
                audio = gen(mel, lens)[:, 0]
                sc, mag = stft_loss(audio, target, ratios)
                (45 * mel_fn(audio, mel, samples, frames) + sc + mag).backward()
            row[key + "_step_ms"] = round(timed(step, args.iters, args.warmup), 3)
            row[key + "_launches"], row[key + "_host_syncs"] = count_launches_and_syncs(step)
        row["torch_over_hip"] = round(row["torch_vectorised_mel_loss_step_ms"] / row["hip_mel_loss_step_ms"], 3)
        res["train_step"][f"B{B}_T{Tm}"] = row
        print(json.dumps({f"train_B{B}_T{Tm}": row}), file=sys.stderr, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    print(json.dumps(res))


def stock_mpd(mpd, dev):
    """the multi-period discriminator and its three losses with torch.nn.functional.conv2d in fp32 under torch autograd, on
    the HIP module's own parameters -> {"vectorised": (d_loss, g_losses), "reference_form": (d_loss, g_losses)} with
    d_loss(y, y_hat, ratios) -> the discriminator loss alone and g_losses(y, y_hat, ratios) -> (fm, gen) alone, so that each
    step runs what that step needs and nothing else.  vectorised: real and generated audio stacked in one pass, masks from
    the formula, nothing read back.  reference_form: one pass per signal as MultiPeriodDiscriminator.forward writes it, the
    reference's mask builder with its .item() (get_mask_from_lengths) and gan_discriminator_loss's two .item() calls per
    discriminator; gan_generator_loss and gan_feature_loss have none of their own."""
    import torch.nn.functional as F
    from rad_mmm_amd.vocoder import fold_weight_norm

    def forward(x):
        outs, fmaps = [], []
        for d in mpd.discriminators:
            p = d.period
            h = x
            if h.shape[2] % p:
                h = F.pad(h, (0, p - h.shape[2] % p), "reflect")
            h = h.view(h.shape[0], 1, h.shape[2] // p, p)
            fm = []
            for i, m in enumerate(d.convs):
                h = F.leaky_relu(F.conv2d(h, fold_weight_norm(m.weight_v, m.weight_g), m.bias, (3 if i < 4 else 1, 1), (2, 0)), 0.1)
                fm.append(h)
            m = d.conv_post
            h = F.conv2d(h, fold_weight_norm(m.weight_v, m.weight_g), m.bias, 1, (1, 0))
            fm.append(h)
            outs.append(h.flatten(1))
            fmaps.append(fm)
        return outs, fmaps

    def both(y, y_hat, item):
        if item:
            return forward(y) + forward(y_hat)
        B = y.shape[0]
        outs, fmaps = forward(torch.cat([y, y_hat], 0))
        return ([o[:B] for o in outs], [[m[:B] for m in fm] for fm in fmaps],
                [o[B:] for o in outs], [[m[B:] for m in fm] for fm in fmaps])

    def mask_of(ratios, size, item):
        n = (ratios * size).ceil().long()
        if item:
            size = int(n.max().item())                        # get_mask_from_lengths of the reference
        return (torch.arange(size, device=dev)[None, :] < n[:, None]).float()

    def d_loss(y, y_hat, ratios, item):
        rs, _, gs, _ = both(y, y_hat, item)
        disc = 0.0
        for dr, dg in zip(rs, gs):
            m = mask_of(ratios, dr.shape[1], item)
            r_loss, g_loss = (((1 - dr) ** 2) * m).sum() / m.sum(), ((dg ** 2) * m).sum() / m.sum()
            if item:
                r_loss.item(), g_loss.item()
            disc = disc + r_loss + g_loss
        return disc

    def g_losses(y, y_hat, ratios, item):
        _, frs, gs, fgs = both(y, y_hat, item)
        fm = gen = 0.0
        for dg, fr, fg in zip(gs, frs, fgs):
            for r, g in zip(fr, fg):
                m = mask_of(ratios, r.shape[2], item)[:, None, :, None]
                fm = fm + ((r - g).abs() * m).sum() / (m.sum() * r.shape[1] * r.shape[3])
            m = mask_of(ratios, dg.shape[1], item)
            gen = gen + (((1 - dg) ** 2) * m).sum() / m.sum()
        return fm, gen
    return {"vectorised": (lambda y, yh, r: d_loss(y, yh, r, False), lambda y, yh, r: g_losses(y, yh, r, False)),
            "reference_form": (lambda y, yh, r: d_loss(y, yh, r, True), lambda y, yh, r: g_losses(y, yh, r, True))}


def stock_msd(msd, dev):
    """the multi-scale discriminator and its three losses with torch.nn.functional.conv1d(groups=) in fp32 under torch
    autograd, on the HIP module's own parameters, in stock_mpd's two forms.  Both fold weight norm and spectral norm with the
    module's torch ops (a training-mode call of the spectral-norm member advances its power iteration, once per signal, as
    in the reference).  vectorised: the weight-normed members see real and generated audio stacked in one pass; the
    spectral-norm member has one weight set per signal in training mode and runs them apart."""
    import torch.nn.functional as F
    from rad_mmm_amd.discriminators import MSD_KERNELS, MSD_STRIDES

    def member(d, x):
        ws = d._weights()
        fm = []
        for l in range(7):
            x = F.leaky_relu(F.conv1d(x, ws[2 * l], ws[2 * l + 1], MSD_STRIDES[l], MSD_KERNELS[l] // 2, 1, d.groups[l]), 0.1)
            fm.append(x)
        x = F.conv1d(x, ws[14], ws[15], 1, 1)
        fm.append(x)
        return x.flatten(1), fm

    def both(y, y_hat, item):
        rs, frs, gs, fgs = [], [], [], []
        for i, d in enumerate(msd.discriminators):
            if i:
                y, y_hat = F.avg_pool1d(y, 4, 2, 2), F.avg_pool1d(y_hat, 4, 2, 2)
            if item or (d.use_spectral_norm and d.training):
                (r, fr), (g, fg) = member(d, y), member(d, y_hat)
            else:
                B = y.shape[0]
                o, fm = member(d, torch.cat([y, y_hat], 0))
                r, fr, g, fg = o[:B], [m[:B] for m in fm], o[B:], [m[B:] for m in fm]
            rs.append(r), frs.append(fr), gs.append(g), fgs.append(fg)
        return rs, frs, gs, fgs

    def mask_of(ratios, size, item):
        n = (ratios * size).ceil().long()
        if item:
            size = int(n.max().item())                        # get_mask_from_lengths of the reference
        return (torch.arange(size, device=dev)[None, :] < n[:, None]).float()

    def d_loss(y, y_hat, ratios, item):
        rs, _, gs, _ = both(y, y_hat, item)
        disc = 0.0
        for dr, dg in zip(rs, gs):
            m = mask_of(ratios, dr.shape[1], item)
            r_loss, g_loss = (((1 - dr) ** 2) * m).sum() / m.sum(), ((dg ** 2) * m).sum() / m.sum()
            if item:
                r_loss.item(), g_loss.item()
            disc = disc + r_loss + g_loss
        return disc

    def g_losses(y, y_hat, ratios, item):
        _, frs, gs, fgs = both(y, y_hat, item)
        fm = gen = 0.0
        for dg, fr, fg in zip(gs, frs, fgs):
            for r, g in zip(fr, fg):
                m = mask_of(ratios, r.shape[2], item)[:, None, :]
                fm = fm + ((r - g).abs() * m).sum() / (m.sum() * r.shape[1])
            m = mask_of(ratios, dg.shape[1], item)
            gen = gen + (((1 - dg) ** 2) * m).sum() / m.sum()
        return fm, gen
    return {"vectorised": (lambda y, yh, r: d_loss(y, yh, r, False), lambda y, yh, r: g_losses(y, yh, r, False)),
            "reference_form": (lambda y, yh, r: d_loss(y, yh, r, True), lambda y, yh, r: g_losses(y, yh, r, True))}


def msd_bench(args, dev):
    from rad_mmm_amd.discriminators import MultiScaleDiscriminator
    torch.manual_seed(3)
    msd = MultiScaleDiscriminator().to(dev).train()
    note = ("one GPU, one process, one session; fp32; ragged len_ratios on the device (the last item full); median of iters "
            "after warmup; training mode, so the spectral-norm member advances its power iteration in every form.  d_step: "
            "discriminator loss forward + parameter gradients, y_hat detached.  g_side: feature + generator loss forward + "
            "gradient of y_hat, parameters frozen.  torch_*: the same discriminator with torch.nn.functional.conv1d(groups=) "
            "(MIOpen) under torch autograd, each step computing only the losses of that step; torch_vectorised stacks real "
            "and generated audio in one pass for the weight-normed members")
    return disc_bench(args, dev, msd, stock_msd(msd, dev), "msd_step_ms", note)


def mpd_bench(args, dev):
    from rad_mmm_amd.discriminators import MultiPeriodDiscriminator
    torch.manual_seed(3)
    mpd = MultiPeriodDiscriminator().to(dev).train()
    note = ("one GPU, one process, one session; fp32; ragged len_ratios on the device (the last item full); median of "
            "iters after warmup.  d_step: discriminator loss forward + parameter gradients, y_hat detached.  g_side: "
            "feature + generator loss forward + gradient of y_hat, parameters frozen.  torch_*: the same "
            "discriminator with torch.nn.functional.conv2d (MIOpen) under torch autograd, each step computing only "
            "the losses of that step; torch_vectorised stacks real and generated audio in one pass")
    return disc_bench(args, dev, mpd, stock_mpd(mpd, dev), "mpd_step_ms", note)


def disc_bench(args, dev, mpd, stock, metric, note):
    res = {"metric": metric, "iters": args.iters, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "note": note, "shapes": {}}
    g = torch.Generator().manual_seed(13)
    for B in (16, 32):
        T = 8192
        ratios = (torch.linspace(T // 3, T, B).round() / T).to(dev)
        y = (torch.rand(B, 1, T, generator=g) * 2 - 1).to(dev)
        y_hat = (y.cpu() + 0.3 * torch.randn(B, 1, T, generator=g)).clamp(-1, 1).to(dev)
        row = {}
        for key, fn in (("hip", None), ("torch_vectorised", stock["vectorised"]), ("torch_reference_form", stock["reference_form"])):
            def d_step():
                mpd.zero_grad(set_to_none=True)
                loss = mpd.discriminator_loss(y, y_hat, ratios)[0] if fn is None else fn[0](y, y_hat, ratios)
                loss.backward()
                return loss.detach()

            def g_side():
                p = y_hat.detach().requires_grad_(True)
                fm, gen = mpd.generator_losses(y, p, ratios) if fn is None else fn[1](y, p, ratios)
                (fm + gen).backward()
                return fm.detach(), gen.detach(), p.grad
            out = {}
            for name, step, frozen in (("d_step", d_step, False), ("g_side", g_side, True)):
                for q in mpd.parameters():
                    q.requires_grad_(not frozen)
                ms = timed(step, args.iters, args.warmup)
                launches, syncs = count_launches_and_syncs(step)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                got = step()
                torch.cuda.synchronize()
                out[name] = {"ms": round(ms, 3), "launches": launches, "host_syncs": syncs,
                             "peak_allocated_mb": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)}
                if name == "d_step":
                    out[name]["loss"] = float(got)
                else:
                    out[name].update(fm=float(got[0]), gen=float(got[1]))
                    out["_grad"] = got[2]
            row[key] = out
            torch.cuda.empty_cache()
        for key in ("torch_vectorised", "torch_reference_form"):
            for name in ("d_step", "g_side"):
                row[key][name]["over_hip"] = round(row[key][name]["ms"] / row["hip"][name]["ms"], 3)
            row[key]["g_side"]["grad_rel_l2_vs_hip"] = float((row[key]["_grad"] - row["hip"]["_grad"]).norm() / row["hip"]["_grad"].norm())
        for key in row:
            del row[key]["_grad"]
        res["shapes"][f"B{B}_T{T}"] = row
        print(json.dumps({f"B{B}_T{T}": row}), file=sys.stderr, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    print(json.dumps(res))


def _mpd_batch(B, dev, g):
    T = 8192
    ratios = (torch.linspace(T // 3, T, B).round() / T).to(dev)
    y = (torch.rand(B, 1, T, generator=g) * 2 - 1).to(dev)
    y_hat = (y.cpu() + 0.3 * torch.randn(B, 1, T, generator=g)).clamp(-1, 1).to(dev)
    return y, y_hat, ratios


def mpd_leg(args, dev):
    """one leg of --mpd --precision h3 in this process: leg a is precision "fp32" (the launches and bits of the module
    before the mode existed), leg b precision "h3"; one JSON line"""
    from rad_mmm_amd.discriminators import MultiPeriodDiscriminator
    torch.manual_seed(3)
    mpd = MultiPeriodDiscriminator().to(dev).train()
    mpd.precision = "fp32" if args.leg == "a" else "h3"
    res = {"leg": args.leg, "precision": mpd.precision, "device": torch.cuda.get_device_name(0), "shapes": {}}
    g = torch.Generator().manual_seed(13)
    for B in (16, 32):
        y, y_hat, ratios = _mpd_batch(B, dev, g)

        def d_step(**kw):
            mpd.zero_grad(set_to_none=True)
            loss = mpd.discriminator_loss(y, y_hat, ratios, **kw)[0]
            loss.backward()
            return loss.detach()

        def g_side(**kw):
            p = y_hat.detach().requires_grad_(True)
            fm, gen = mpd.generator_losses(y, p, ratios, **kw)
            (fm + gen).backward()
            return fm.detach(), gen.detach(), p.grad
        row = {}
        for name, step, frozen in (("d_step", d_step, False), ("g_side", g_side, True)):
            for q in mpd.parameters():
                q.requires_grad_(not frozen)
            ms = timed(step, args.iters, args.warmup)
            launches, syncs = count_launches_and_syncs(step)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            got = step()
            torch.cuda.synchronize()
            row[name] = {"ms": round(ms, 3), "launches": launches, "host_syncs": syncs,
                         "peak_allocated_mb": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)}
            if name == "d_step":
                row[name]["loss"] = float(got)
                if args.leg == "b":
                    grads = torch.cat([q.grad.reshape(-1) for q in mpd.parameters()])
                    d_step(precision="fp32")
                    ref = torch.cat([q.grad.reshape(-1) for q in mpd.parameters()])
                    row[name]["param_grad_rel_l2_vs_fp32"] = float((grads - ref).norm() / ref.norm())
            else:
                row[name].update(fm=float(got[0]), gen=float(got[1]))
                if args.leg == "b":
                    ref = g_side(precision="fp32")[2]
                    row[name]["audio_grad_rel_l2_vs_fp32"] = float((got[2] - ref).norm() / ref.norm())
        if args.leg == "b":
            row["saturated"] = mpd.grad_saturated()
            row["plan"] = [[m for m, _ in d.values()] for d in mpd.precision_plan(B=B, T=8192)]
        res["shapes"][f"B{B}_T8192"] = row
        print(json.dumps({f"B{B}_T8192": row}), file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    print(json.dumps(res))


def _abba(args, flags):
    """legs a b b a, each in a fresh process (this process never opens the GPU) -> the four result lines"""
    import subprocess
    runs = []
    for leg in "abba":
        out = subprocess.run([sys.executable, os.path.abspath(__file__), *flags, "--leg", leg, "--iters", str(args.iters),
                              "--warmup", str(args.warmup)], check=True, stdout=subprocess.PIPE, text=True).stdout
        runs.append(json.loads(out.strip().splitlines()[-1]))
    return runs


def _merge_legs(runs, field, ratio_of):
    """per shape and leg: the last run's figures, both runs' times, their mean and spread; ratio_of: (step name or None)"""
    shapes = {}
    for shape in runs[0]["shapes"]:
        row = {}
        for r in runs:
            e = row.setdefault(r["leg"], {})
            for name, v in r["shapes"][shape].items():
                if isinstance(v, dict) and field in v:
                    d = e.setdefault(name, dict(v, **{field: []}))
                    d[field].append(v[field])
                else:
                    e[name] = v
        for e in row.values():
            for d in e.values():
                if isinstance(d, dict) and field in d:
                    d[field + "_mean"] = round(sum(d[field]) / len(d[field]), 3)
                    d[field + "_spread"] = round(max(d[field]) - min(d[field]), 3)
        for name in ratio_of:
            a, b = row["a"][name], row["b"][name]
            b["fp32_over_h3"] = round(a[field + "_mean"] / b[field + "_mean"], 3)
            b["faster_than_fp32_beyond_the_spread"] = bool(a[field + "_mean"] - b[field + "_mean"] > max(a[field + "_spread"], b[field + "_spread"]))
        shapes[shape] = {"fp32": row["a"], "h3": row["b"]}
    return shapes


def mpd_h3_bench(args):
    """--mpd --precision h3: precision "h3" (leg b) against precision "fp32" (leg a), order a b b a"""
    runs = _abba(args, ["--mpd", "--precision", "h3"])
    res = {"metric": "mpd_step_ms", "iters": args.iters, "warmup": args.warmup, "device": runs[0]["device"], "order": "a b b a",
           "note": "one GPU, one fresh process per leg, one session; the reference's widths, ragged len_ratios on the device (the "
                   "last item full), the batches of profiles/mpd.json; median of iters after warmup.  a: precision 'fp32' -- the "
                   "code path, launches and bits of the module before the mode existed.  b: precision 'h3'.  d_step: "
                   "discriminator loss forward + parameter gradients, y_hat detached.  g_side: feature + generator loss forward "
                   "+ gradient of y_hat, parameters frozen.  ms: both runs of the leg; ms_spread: their difference",
           "shapes": _merge_legs(runs, "ms", ("d_step", "g_side"))}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


def gan_step_h3_leg(args, dev):
    """one leg of --gan-step --mpd-precision h3: HiFiGANTrainingStep with mpd_precision "fp32" (a) or "h3" (b)"""
    from rad_mmm_amd.discriminators import MultiPeriodDiscriminator, MultiScaleDiscriminator
    from rad_mmm_amd.mel_loss import MelSpectrogramLoss
    from rad_mmm_amd.stft_loss import MultiResolutionSTFTLoss
    from rad_mmm_amd.vocoder_step import HiFiGANTrainingStep
    gen = HiFiGANGenerator(V1)
    gen.load_state_dict(random_state(gen, 5, 0.2, 0.6))
    torch.manual_seed(3)
    gen, mpd, msd = gen.to(dev).train(), MultiPeriodDiscriminator().to(dev).train(), MultiScaleDiscriminator().to(dev).train()
    obj = HiFiGANTrainingStep(gen, mpd, msd, stft_loss=MultiResolutionSTFTLoss().to(dev), mel_loss=MelSpectrogramLoss().to(dev),
                              mpd_precision="fp32" if args.leg == "a" else "h3")
    res = {"leg": args.leg, "mpd_precision": mpd.precision, "device": torch.cuda.get_device_name(0), "shapes": {}}
    g = torch.Generator().manual_seed(17)
    hop = gen.hop
    for B in (16, 32):
        T = 32
        lens = [int(v) for v in torch.linspace(T // 3, T, B).round()]
        mel = (torch.randn(B, 80, T, generator=g) - 2.0).to(dev)
        target = torch.rand(B, 1, T * hop, generator=g) * 2 - 1
        for b, n in enumerate(lens):
            target[b, :, n * hop:] = 0.0
        target = target.to(dev)
        step = lambda: obj.training_step(mel, lens, target)["g_total"]
        torch.cuda.empty_cache()
        ms = timed(step, args.iters, args.warmup)
        launches, syncs = count_launches_and_syncs(step)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        loss = step()
        torch.cuda.synchronize()
        row = {"step": {"step_ms": round(ms, 3), "launches": launches, "host_syncs": syncs,
                        "peak_allocated_mb": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1), "g_total": float(loss)}}
        if args.leg == "b":
            row["saturated"] = mpd.grad_saturated()
        res["shapes"][f"B{B}_T{T}"] = row
        print(json.dumps({f"B{B}_T{T}": row}), file=sys.stderr, flush=True)
    print(json.dumps(res))


def gan_step_h3_bench(args):
    """--gan-step --mpd-precision h3: the whole step with the multi-period discriminator in "h3" (b) against "fp32" (a)"""
    runs = _abba(args, ["--gan-step", "--mpd-precision", "h3"])
    return {"metric": "hifigan_gan_step_ms", "config": "V1", "frames": 32, "iters": args.iters, "warmup": args.warmup,
            "device": runs[0]["device"], "order": "a b b a",
            "note": "HiFiGANTrainingStep, one fresh process per leg, ragged host lens, the batches of profiles/"
                    "hifigan_gan_step.json; a: mpd_precision 'fp32', b: mpd_precision 'h3'",
            "shapes": _merge_legs(runs, "step_ms", ("step",))}


def gan_step_leg(args, dev):
    """one leg of --gan-step in this process: one JSON line"""
    from rad_mmm_amd.discriminators import MultiPeriodDiscriminator, MultiScaleDiscriminator
    from rad_mmm_amd.mel_loss import MelSpectrogramLoss
    from rad_mmm_amd.stft_loss import MultiResolutionSTFTLoss
    gen = HiFiGANGenerator(V1)
    gen.load_state_dict(random_state(gen, 5, 0.2, 0.6))
    torch.manual_seed(3)
    gen, mpd, msd = gen.to(dev).train(), MultiPeriodDiscriminator().to(dev).train(), MultiScaleDiscriminator().to(dev).train()
    loss_fn, mel_loss = MultiResolutionSTFTLoss().to(dev), MelSpectrogramLoss().to(dev)
    n_params = sum(p.numel() for m in (gen, mpd, msd) for p in m.parameters())
    hop = gen.hop
    d_params = list(mpd.parameters()) + list(msd.parameters())
    if args.leg == "a":
        from rad_mmm_amd.vocoder_step import HiFiGANTrainingStep
        obj = HiFiGANTrainingStep(gen, mpd, msd, stft_loss=loss_fn, mel_loss=mel_loss)
        forms = {"a": lambda mel, lens, target: obj.training_step(mel, lens, target)["g_total"]}
    else:
        opt_g = torch.optim.AdamW(gen.parameters(), 2e-4, betas=(0.8, 0.99))
        opt_d = torch.optim.AdamW(d_params, 2e-4, betas=(0.8, 0.99))

        def recipe(mel, lens, target, frozen=False):
            lens = torch.as_tensor(lens, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
            audio = gen(mel, lens)
            ratios = lens / lens.max()
            opt_d.zero_grad()
            loss_p, _, _ = mpd.discriminator_loss(target, audio.detach(), ratios)
            loss_s, _, _ = msd.discriminator_loss(target, audio.detach(), ratios)
            (loss_p + loss_s).backward()
            opt_d.step()
            opt_g.zero_grad()
            for p in d_params:
                p.requires_grad_(not frozen)
            fm_p, gen_p = mpd.generator_losses(target, audio, ratios)
            fm_s, gen_s = msd.generator_losses(target, audio, ratios)
            sc, mag = loss_fn(audio[:, 0], target[:, 0], ratios)
            total = 45 * mel_loss(audio[:, 0], mel, lens * hop, lens) + fm_p + fm_s + gen_p + gen_s + sc + mag
            total.backward()
            opt_g.step()
            for p in d_params:
                p.requires_grad_(True)
            return total.detach()
        forms = {"b": recipe, "b_frozen": lambda mel, lens, target: recipe(mel, lens, target, True)}
    res = {"leg": args.leg, "device": torch.cuda.get_device_name(0), "parameters": n_params, "shapes": {}}
    g = torch.Generator().manual_seed(17)
    for B in (16, 32):
        T = 32
        lens = [int(v) for v in torch.linspace(T // 3, T, B).round()]
        mel = (torch.randn(B, 80, T, generator=g) - 2.0).to(dev)
        target = torch.rand(B, 1, T * hop, generator=g) * 2 - 1
        for b, n in enumerate(lens):
            target[b, :, n * hop:] = 0.0
        target = target.to(dev)
        row = {}
        for key, fn in forms.items():
            step = lambda: fn(mel, lens, target)
            torch.cuda.empty_cache()
            ms = timed(step, args.iters, args.warmup)
            launches, syncs = count_launches_and_syncs(step)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            loss = step()
            torch.cuda.synchronize()
            row[key] = {"step_ms": round(ms, 3), "launches": launches, "host_syncs": syncs,
                        "peak_allocated_mb": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1), "g_total": float(loss)}
        res["shapes"][f"B{B}_T{T}"] = row
        print(json.dumps({f"B{B}_T{T}": row}), file=sys.stderr, flush=True)
    print(json.dumps(res))


def gan_step_bench(args):
    """--gan-step: legs a b b a, each in a fresh process; this process never opens the GPU"""
    import subprocess
    runs = []
    for leg in "abba":
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--gan-step", "--leg", leg, "--iters", str(args.iters),
                              "--warmup", str(args.warmup)], check=True, stdout=subprocess.PIPE, text=True).stdout
        runs.append(json.loads(out.strip().splitlines()[-1]))
    res = {"metric": "hifigan_gan_step_ms", "config": "V1", "frames": 32, "iters": args.iters, "warmup": args.warmup,
           "device": runs[0]["device"], "parameters": runs[0]["parameters"], "order": "a b b a",
           "note": "one GPU, one fresh process per leg, one session; fp32; ragged host lens; median of iters after warmup.  "
                   "a: HiFiGANTrainingStep (two FlatAdam, discriminators frozen during the G side).  b: the README recipe "
                   "as written with two torch.optim.AdamW.  b_frozen: the recipe with the discriminators' parameters "
                   "frozen during the G side (same process as b).  step_ms: both runs of the leg and their mean",
           "shapes": {}}
    for shape in runs[0]["shapes"]:
        row = {}
        for r in runs:
            for key, v in r["shapes"][shape].items():
                e = row.setdefault(key, dict(v, step_ms=[]))
                e["step_ms"].append(v["step_ms"])
        for e in row.values():
            e["step_ms_mean"] = round(sum(e["step_ms"]) / len(e["step_ms"]), 3)
        for key in ("b", "b_frozen"):
            row[key]["over_a"] = round(row[key]["step_ms_mean"] / row["a"]["step_ms_mean"], 3)
        res["shapes"][shape] = row
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--train", action="store_true", help="time one V1 training step against stock torch autograd")
    ap.add_argument("--stft-loss", action="store_true", help="time the multi-resolution STFT loss against stock torch")
    ap.add_argument("--mel-loss", action="store_true", help="time the mel L1 loss against stock torch")
    ap.add_argument("--mpd", action="store_true", help="time the multi-period discriminator's D step and G side against "
                                                       "stock torch")
    ap.add_argument("--msd", action="store_true", help="time the multi-scale discriminator's D step and G side against "
                                                       "stock torch")
    ap.add_argument("--d-step-only", action="store_true", help="--msd, or --mpd --precision h3: run the module's D step at 32 x 8192 a few times and "
                                                               "exit (the workload of a kernel trace)")
    ap.add_argument("--gan-step", action="store_true", help="time the whole HiFi-GAN fine-tuning step: HiFiGANTrainingStep "
                                                            "against the README recipe with torch.optim.AdamW")
    ap.add_argument("--leg", choices=("a", "b"), default=None, help="--gan-step: run this leg in this process (the driver "
                                                                    "starts one process per leg)")
    ap.add_argument("--precision", choices=("fp32", "f16", "h3"), default="fp32",
                    help="the generator's inference mode (fp32 / f16); with --mpd: h3 times the multi-period discriminator's "
                         "precision 'h3' against 'fp32', legs a b b a in fresh processes, into profiles/mpd_h3.json")
    ap.add_argument("--mpd-precision", choices=("fp32", "h3"), default="fp32",
                    help="--gan-step: h3 times HiFiGANTrainingStep(mpd_precision='h3') against 'fp32', legs a b b a; the result "
                         "is added to --out (default profiles/mpd_h3.json) under 'gan_step'")
    ap.add_argument("--config", choices=("V1", "V3"), default=None, help="only this config")
    ap.add_argument("--shape", default=None, help="only this BxT, e.g. 32x800")
    ap.add_argument("--out", default=None, help="--stft-loss / --mel-loss / --mpd / --msd: result file (default profiles/"
                                                "stft_loss.json / mel_loss.json / mpd.json / msd.json)")
    args = ap.parse_args()
    h3_mpd, h3_step = args.mpd and args.precision == "h3", args.gan_step and args.mpd_precision == "h3"
    if args.precision == "h3" and not args.mpd:
        ap.error("--precision h3 is the multi-period discriminator's mode: use it with --mpd")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "mpd_h3.json" if h3_mpd or h3_step else "hifigan_gan_step.json" if args.gan_step
                                else "msd.json" if args.msd else "mpd.json" if args.mpd else "mel_loss.json" if args.mel_loss
                                else "stft_loss.json")
    if h3_mpd and args.leg is None and not args.d_step_only:
        return mpd_h3_bench(args)
    if h3_step and args.leg is None:
        part = gan_step_h3_bench(args)
        res = json.load(open(args.out)) if os.path.exists(args.out) else {}
        res["gan_step"] = part
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
        print(json.dumps(part))
        return
    if args.gan_step and args.leg is None:
        return gan_step_bench(args)
    dev = torch.device("cuda:0")
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    if h3_step:
        return gan_step_h3_leg(args, dev)
    if args.gan_step:
        return gan_step_leg(args, dev)
    if h3_mpd and args.d_step_only:         # the workload of a kernel trace: the D step at 32 x 8192 in precision "h3"
        from rad_mmm_amd.discriminators import MultiPeriodDiscriminator
        torch.manual_seed(3)
        mpd = MultiPeriodDiscriminator().to(dev).train()
        mpd.precision = "h3"
        y, y_hat, ratios = _mpd_batch(32, dev, torch.Generator().manual_seed(13))
        for _ in range(args.warmup + args.iters):
            mpd.zero_grad(set_to_none=True)
            mpd.discriminator_loss(y, y_hat, ratios)[0].backward()
        torch.cuda.synchronize()
        return
    if h3_mpd:
        return mpd_leg(args, dev)
    if args.train:
        return train_bench(args, dev)
    if args.stft_loss:
        return stft_loss_bench(args, dev)
    if args.mel_loss:
        return mel_loss_bench(args, dev)
    if args.mpd:
        return mpd_bench(args, dev)
    if args.msd and args.d_step_only:
        from rad_mmm_amd.discriminators import MultiScaleDiscriminator
        torch.manual_seed(3)
        msd = MultiScaleDiscriminator().to(dev).train()
        g = torch.Generator().manual_seed(13)
        y = (torch.rand(32, 1, 8192, generator=g) * 2 - 1).to(dev)
        y_hat = (y.cpu() + 0.3 * torch.randn(32, 1, 8192, generator=g)).clamp(-1, 1).to(dev)
        ratios = (torch.linspace(8192 // 3, 8192, 32).round() / 8192).to(dev)
        for _ in range(args.warmup + args.iters):
            msd.zero_grad(set_to_none=True)
            msd.discriminator_loss(y, y_hat, ratios)[0].backward()
        torch.cuda.synchronize()
        return
    if args.msd:
        return msd_bench(args, dev)
    res = {"metric": "vocoder_ms", "precision": args.precision, "configs": {}}
    shapes = ((32, 800), (1, 800)) if args.shape is None else (tuple(int(v) for v in args.shape.split("x")),)
    for name, cfg in (("V1", V1), ("V3", V3)):
        if args.config not in (None, name):
            continue
        gen = HiFiGANGenerator(cfg)
        sd = random_state(gen, 5, 0.2, 0.6)
        gen.load_state_dict(sd)
        gen = gen.to(dev).eval()
        den = Denoiser(gen).to(dev)
        den._bias(dev)                       # on the fp32 path, before the switch
        gen.precision = args.precision
        plan = gen.precision_plan()
        g = torch.Generator().manual_seed(6)
        for B, T in shapes:
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
            if args.precision != "fp32":
                a32 = gen(mel, lens, precision="fp32")[:, 0]
                row["rel_l2_vs_fp32"] = float((audio - a32).norm() / a32.norm())
                row["plan"] = [m for m, _ in plan]
                del a32
            # per-stage: device events between the stages of one call
            ev = []
            lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
            for _ in range(2):
                ev = []
                gen._run(mel, lens_d, ev, precision=args.precision)
            torch.cuda.synchronize()
            stages = []
            for (sname, flop, byt), e0, e1 in zip(stage_costs(gen, cfg, B, T, plan), ev[:-1], ev[1:]):
                ms = e0.elapsed_time(e1)
                # an f16 stage: its transposed conv (fp32 MFMA) and its resblock convs (f16 MFMA) each at their own peak
                f16 = sname.startswith("stage") and plan[int(sname[5:]) - 1][0] == "f16"
                if f16:
                    i = int(sname[5:]) - 1
                    up = 2.0 * (B * T * int(np.prod(cfg["upsample_rates"][:i]))) * (cfg["upsample_initial_channel"] >> i) * \
                        (cfg["upsample_initial_channel"] >> (i + 1)) * cfg["upsample_kernel_sizes"][i]
                    t_c = up / (FP32_MFMA_TF * 1e12) + (flop - up) / (F16_MFMA_TF * 1e12)
                else:
                    t_c = flop / (FP32_MFMA_TF * 1e12)
                t_m = byt / (HBM_TBS * 1e12)
                roof = ("f16_mfma" if f16 else "fp32_mfma") if t_c >= t_m else "hbm"
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
