"""Host models of HiFi-GAN's precision "f16" (rad_mmm_amd/vocoder.py, csrc/vocoder_f16.hip).

conv_f16_ref: a float64 model of radmmm_voc_conv_f16's contract (include/radmmm_hip.h) on the operands as stored: the
operand rounding h(lrelu(in_scale * x)) is reproduced bit for bit (float32 arithmetic, the clamp, astype(float16)), the
sum over taps and channels is float64.

generator_f16_ref: tests/_vocoder_ref.generator_ref in float64 with exactly those operand roundings in the resblock convs
of the stages a plan marks "f16" and nothing else changed: the emulation, i.e. the definition of the mode.

The inputs the GPU tests use are built here as well (cases), so the CPU tests can check them (tests/test_vocoder_f16_cpu.py
picks the seeds: the emulation's error must be well above fp32's, or a factor test against it would mean nothing)."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from _vocoder_ref import _new_keys, _w, generator_ref, load_fixture, random_state
from rad_mmm_amd.vocoder import LRELU_SLOPE, PRECISIONS  # noqa: F401  (the mode's names and the slope are the package's)

W_SCALE = 256.0            # rad_mmm_amd.ops.W_SCALE (tests/test_vocoder_f16_cpu.py checks it)
F16_CLAMP = 60000.0        # csrc/split_pack.h clamp_f16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def h16(x, in_scale=1.0, in_slope=1.0):
    """float32 array -> float16 array: the kernel's operand, bit for bit"""
    v = np.asarray(x, dtype=np.float32) * np.float32(in_scale)
    v = np.where(v >= 0, v, np.float32(in_slope) * v).astype(np.float32)
    return np.clip(v, np.float32(-F16_CLAMP), np.float32(F16_CLAMP)).astype(np.float16)


def conv_f16_ref(X, Wh, bias, B, T, C, taps, dil, lens=None, add=None, Y2=None, y2_accum=False, in_scale=1.0,
                 in_slope=1.0, acc_scale=1.0):
    """X [B*T, ldx] float32, Wh [taps, C, ldw] float16, bias [C], add [B*T, ldadd] or None, Y2 [B*T, ldy2] (the previous
    content, read only with y2_accum) -> dict of float64 [B*T, C] arrays:
       y     the output (zeros at and past the lengths)
       y2    the second output
       mag   acc_scale * sum |w| |a| (the scale of the accumulation's rounding error), 0 at and past the lengths
    Nothing at or past a length enters a result (NaN there stays out)."""
    lens = [T] * B if lens is None else [int(n) for n in lens]
    a = np.zeros((B, T, C))
    x3 = np.asarray(X).reshape(B, T, -1)
    for b, n in enumerate(lens):
        a[b, :n] = h16(x3[b, :n, :C], in_scale, in_slope).astype(np.float64)
    W = np.asarray(Wh)[:, :, :C].astype(np.float64)
    v, mag = np.zeros((B, T, C)), np.zeros((B, T, C))
    for tap in range(taps):
        s = (tap - taps // 2) * dil
        sh = np.zeros_like(a)
        lo, hi = max(0, -s), min(T, T - s)
        if lo < hi:
            sh[:, lo:hi] = a[:, lo + s:hi + s]
        v += sh @ W[tap].T
        mag += np.abs(sh) @ np.abs(W[tap]).T
    v, mag = v * acc_scale, mag * acc_scale
    v = v + np.asarray(bias, dtype=np.float64)[:C]
    y = np.zeros((B, T, C))
    add3 = None if add is None else np.asarray(add).reshape(B, T, -1)
    for b, n in enumerate(lens):
        y[b, :n] = v[b, :n] + (add3[b, :n, :C] if add3 is not None else 0.0)
        mag[b, n:] = 0.0
    y = y.reshape(B * T, C)
    y2 = y + np.asarray(Y2)[:, :C].astype(np.float64) if y2_accum else y.copy()
    return {"y": y, "y2": y2, "mag": mag.reshape(B * T, C)}


def _mode_of(entry):
    mode = entry if isinstance(entry, str) else entry[0]
    assert mode in PRECISIONS, mode
    return mode


def _conv16(x, w, bias, dilation, padding):
    """conv1d(leaky_relu(x)) with the kernel's operand roundings: the activations go through fp32 (as they are stored),
    the leaky-relu is fp32, both operands are rounded to fp16 (the weight times W_SCALE, from its fp32 fold), float64 sum"""
    a = torch.from_numpy(h16(x.float().numpy(), 1.0, LRELU_SLOPE).astype(np.float64))
    wf = (w.float() * W_SCALE).clamp(-F16_CLAMP, F16_CLAMP).half().double() / W_SCALE
    return F.conv1d(a, wf, bias, dilation=dilation, padding=padding)


def generator_f16_ref(sd, cfg, mel, plan):
    """generator_ref (mel [1, 80, T] -> audio [1, 1, T*hop], float64) with the resblock convs of the stages whose plan
    entry is "f16" (a name, or (name, reason) as HiFiGANGenerator.precision_plan returns) replaced by _conv16"""
    sd = _new_keys(sd)
    b = lambda n: sd[n + ".bias"].double()

    def conv(x, name, dilation, padding, f16):
        if f16:
            return _conv16(x, _w(sd, name), b(name), dilation, padding)
        return F.conv1d(F.leaky_relu(x, LRELU_SLOPE), _w(sd, name), b(name), dilation=dilation, padding=padding)

    x = F.conv1d(mel.double(), _w(sd, "conv_pre"), b("conv_pre"), padding=3)
    nk = len(cfg["resblock_kernel_sizes"])
    for i, (u, k) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
        f16 = _mode_of(plan[i]) == "f16"
        x = F.leaky_relu(x, LRELU_SLOPE)
        x = F.conv_transpose1d(x, _w(sd, f"ups.{i}"), b(f"ups.{i}"), stride=u, padding=(k - u) // 2)
        xs = None
        for j, (ks, ds) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"])):
            pre = f"resblocks.{i}.{j}"
            y = x
            if cfg["resblock"] == "1":
                for n, d in enumerate(ds):
                    t = conv(y, f"{pre}.convs1.{n}", d, (ks * d - d) // 2, f16)
                    t = conv(t, f"{pre}.convs2.{n}", 1, (ks - 1) // 2, f16)
                    y = t + y
            else:
                for n, d in enumerate(ds):
                    t = conv(y, f"{pre}.convs.{n}", d, (ks * d - d) // 2, f16)
                    y = t + y
            xs = y if xs is None else xs + y
        x = xs / nk
    x = F.leaky_relu(x)
    x = F.conv1d(x, _w(sd, "conv_post"), b("conv_post"), padding=3)
    return torch.tanh(x)


def rel_l2(a, b):
    return float((a - b).norm() / b.norm())


# ---- the inputs of tests/test_vocoder_f16_gpu.py --------------------------------------------------------------------
R1_WIDE = dict(resblock="1", upsample_rates=[4, 4], upsample_kernel_sizes=[8, 8], upsample_initial_channel=64,
               resblock_kernel_sizes=[3, 5, 7], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]],
               gaussian_blur={"p_blurring": 0.0})
# one V1-width resblock stage: conv_pre to 512 channels, one transposed conv to 256, V1's three resblocks, conv_post
V1_STAGE = dict(resblock="1", upsample_rates=[2], upsample_kernel_sizes=[4], upsample_initial_channel=512,
                resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]],
                gaussian_blur={"p_blurring": 0.0})
SEEDS = {"r1_wide": (11, 12), "v1_stage": (21, 22)}          # (weights, mel)


def _model(cfg, sd):
    from rad_mmm_amd.vocoder import HiFiGANGenerator
    g = HiFiGANGenerator(cfg)
    if sd is not None:
        g.load_state_dict(sd)
    return g


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(cfg, sd, mel [B, 80, T] float32, lens, plan (names per stage), refs [{exact, f16}] per item, float64)"""
    if name == "r1":
        with np.load(os.path.join(GOLDEN, "vocoder_gen_r1.npz")) as f:
            d = {k: f[k] for k in f.files}
        cfg, sd = load_fixture(d)
        mel, lens = torch.from_numpy(d["mel"]), [int(n) for n in d["lens"]]
    else:
        cfg = {"r1_wide": R1_WIDE, "v1_stage": V1_STAGE}[name]
        ws, ms = SEEDS[name]
        sd = random_state(_model(cfg, None), ws)
        lens = {"r1_wide": [13, 2, 7], "v1_stage": [80, 37]}[name]
        mel = torch.randn(len(lens), 80, max(lens), generator=torch.Generator().manual_seed(ms)) - 2.0
    plan = [m for m, _ in _model(cfg, sd).precision_plan("f16")]
    refs = [{"exact": generator_ref(sd, cfg, mel[b:b + 1, :, :n])[0, 0],
             "f16": generator_f16_ref(sd, cfg, mel[b:b + 1, :, :n], plan)[0, 0]} for b, n in enumerate(lens)]
    return dict(cfg=cfg, sd=sd, mel=mel, lens=lens, plan=plan, refs=refs)
