"""Restatement of the HiFi-GAN multi-period discriminator and the three GAN losses in torch on the CPU, any
dtype (float64 is the yardstick, float32 measures what fp32 arithmetic alone costs), any widths, gradients by autograd.
Written from the formulas, not by calling the reference: tests/test_mpd_cpu.py holds it to the reference's fixtures.

A discriminator of period p: reflect-pad the audio on the right to a multiple of p, fold x[b, 0, h, w] = audio[b, h*p + w],
four convs along h of 5 taps, stride 3, zero pad 2, one of 5 taps, stride 1, pad 2, each followed by leaky relu of slope
0.1, then conv_post of 3 taps, pad 1, one channel.  The feature maps are the five activated outputs and conv_post's; the
output is conv_post's flattened over (h, w).

Losses, item b counting n = ceil(len_ratios[b] * size) of `size` (everything when len_ratios is None):
    feature   sum over maps of  sum_{b, c, h < n_b, w} |r - g| / (sum_b n_b * C * p),        size = the map's rows
    disc      sum over discriminators of  sum_{i < n_b} (1 - dr)^2 / sum_b n_b + sum_{i < n_b} dg^2 / sum_b n_b
    gen       sum over discriminators of  sum_{i < n_b} (1 - dg)^2 / sum_b n_b,              size = the flattened length

`variant` plants ONE deliberate error (tests/test_mpd_cpu.py shows that the GPU tests' bars see each of them):
    fold_transposed  x[b, 0, h, w] = audio[b, w*H + h]          edge_pad     replicate instead of reflect
    zero_pad1        the first conv padded by 1, not 2           stride2      stride 2 instead of 3
    slope001         leaky-relu slope 0.01                      floor        floor instead of ceil in the counts
    mask_h           the outputs masked by rows h instead of flattened positions
    norm_no_cp       the feature normaliser without C * p       factor2      upstream feature_loss's factor 2
    detach_real      the real branch of the feature loss detached
"""
import math

import torch
import torch.nn.functional as F

PERIODS = (2, 3, 5, 7, 11)
VARIANTS = ("fold_transposed", "edge_pad", "zero_pad1", "stride2", "slope001", "floor", "mask_h", "norm_no_cp", "factor2",
            "detach_real")


def fold_weight(sd, prefix):
    """weight of one conv from a state dict: weight_g * weight_v / ||weight_v[i]|| (weight norm over dim 0) or weight"""
    if prefix + "weight_g" in sd:
        v, g = sd[prefix + "weight_v"], sd[prefix + "weight_g"]
        n = v.reshape(v.shape[0], -1).pow(2).sum(1).sqrt().reshape(-1, 1, 1, 1)
        return v * (g / n)
    return sd[prefix + "weight"]


def disc_forward(sd, prefix, period, x, variant=None, inputs=None):
    """x [B, 1, T] -> (output [B, H*p], [six maps [B, C, H, p]]); inputs: a list that receives every leaky-relu input"""
    B, _, T = x.shape
    p = period
    if T % p:
        n_pad = p - T % p
        if T <= n_pad:
            raise ValueError(f"{T} samples cannot be reflect-padded by {n_pad}")
        if variant == "edge_pad":
            tail = x[:, :, -1:].expand(B, 1, n_pad)
        else:
            tail = x[:, :, T - 1 - torch.arange(1, n_pad + 1)]
        x = torch.cat([x, tail], 2)
    H = x.shape[2] // p
    x = x.reshape(B, 1, p, H).transpose(2, 3) if variant == "fold_transposed" else x.reshape(B, 1, H, p)
    slope = 0.01 if variant == "slope001" else 0.1
    fmap = []
    for l in range(5):
        st = 1 if l == 4 else (2 if variant == "stride2" else 3)
        x = F.conv2d(x, fold_weight(sd, f"{prefix}convs.{l}."), sd[f"{prefix}convs.{l}.bias"], (st, 1),
                     (1 if variant == "zero_pad1" and l == 0 else 2, 0))
        if inputs is not None:
            inputs.append(x.detach().double().reshape(-1))
        x = torch.where(x > 0, x, slope * x)
        fmap.append(x)
    x = F.conv2d(x, fold_weight(sd, prefix + "conv_post."), sd[prefix + "conv_post.bias"], 1, (1, 0))
    fmap.append(x)
    return x.reshape(B, -1), fmap


def mpd_forward(sd, y, y_hat, periods=PERIODS, variant=None, inputs=None):
    rs, gs, frs, fgs = [], [], [], []
    for i, p in enumerate(periods):
        r, fr = disc_forward(sd, f"discriminators.{i}.", p, y, variant, inputs)
        g, fg = disc_forward(sd, f"discriminators.{i}.", p, y_hat, variant, inputs)
        rs.append(r), gs.append(g), frs.append(fr), fgs.append(fg)
    return rs, gs, frs, fgs


def counts(len_ratios, size, variant=None):
    """[B] int64: ceil(len_ratios * size) evaluated in len_ratios' dtype, clamped to [0, size]"""
    v = len_ratios * size
    return (v.floor() if variant == "floor" else v.ceil()).long().clamp(0, size)


def _mask(n, size, dtype):
    return (torch.arange(size, device=n.device)[None, :] < n[:, None]).to(dtype)


def feature_loss(fmap_rs, fmap_gs, len_ratios=None, variant=None):
    loss = 0.0
    for dr, dg in zip(fmap_rs, fmap_gs):
        for r, g in zip(dr, dg):
            if variant == "detach_real":
                r = r.detach()
            B, C, H, p = r.shape
            d = (r - g).abs()
            if len_ratios is None:
                term = d.sum() / (B * C * H * p)
            else:
                n = counts(len_ratios, H, variant)
                norm = n.sum().to(r.dtype) * (1 if variant == "norm_no_cp" else C * p)
                term = (d * _mask(n, H, r.dtype)[:, None, :, None]).sum() / norm
            loss = loss + term
    return 2 * loss if variant == "factor2" else loss


def _adv_terms(d, len_ratios, p, variant):
    """(mask [B, N], normaliser) of one discriminator output [B, N]"""
    B, N = d.shape
    if len_ratios is None:
        return torch.ones(B, N, dtype=d.dtype, device=d.device), float(B * N)
    if variant == "mask_h":
        n = counts(len_ratios, N // p, variant)
        m = _mask(n, N // p, d.dtype)[:, :, None].expand(B, N // p, p).reshape(B, N)
        return m, m.sum()
    n = counts(len_ratios, N, variant)
    return _mask(n, N, d.dtype), n.sum().to(d.dtype)


def discriminator_loss(rs, gs, len_ratios=None, periods=PERIODS, variant=None):
    """-> (loss, r_losses [n], g_losses [n])"""
    r_l, g_l = [], []
    for dr, dg, p in zip(rs, gs, periods):
        m, n = _adv_terms(dr, len_ratios, p, variant)
        r_l.append((((1 - dr) ** 2) * m).sum() / n)
        g_l.append(((dg ** 2) * m).sum() / n)
    r_l, g_l = torch.stack(r_l), torch.stack(g_l)
    return (r_l + g_l).sum(), r_l, g_l


def generator_loss(gs, len_ratios=None, periods=PERIODS, variant=None):
    loss = 0.0
    for dg, p in zip(gs, periods):
        m, n = _adv_terms(dg, len_ratios, p, variant)
        loss = loss + (((1 - dg) ** 2) * m).sum() / n
    return loss


def run(sd, y, y_hat, len_ratios=None, dtype=torch.float64, periods=PERIODS, variant=None, w_fm=2.0, w_gen=1.0, w_disc=1.0,
        inputs=None):
    """One backward of L = w_fm * fm + w_gen * gen + w_disc * disc.  sd: state dict (numpy or torch); y, y_hat [B, 1, T];
    len_ratios is used in the dtype it comes in (the counts are part of the semantics).  -> dict with fm, gen, disc,
    r_losses, g_losses, the outputs out_r / out_g (lists), and grad[<parameter name>], grad["y_hat"], as float64 numpy;
    grad_y is the gradient of the real audio (through the discriminator and feature losses)."""
    P = {k: torch.as_tensor(v).to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    y = torch.as_tensor(y).to(dtype).clone().requires_grad_(True)
    yh = torch.as_tensor(y_hat).to(dtype).clone().requires_grad_(True)
    lr = None if len_ratios is None else torch.as_tensor(len_ratios)
    rs, gs, frs, fgs = mpd_forward(P, y, yh, periods, variant, inputs)
    fm = feature_loss(frs, fgs, lr, variant)
    gen = generator_loss(gs, lr, periods, variant)
    disc, r_l, g_l = discriminator_loss(rs, gs, lr, periods, variant)
    (w_fm * fm + w_gen * gen + w_disc * disc).backward()
    grad = {k: v.grad.double().numpy() for k, v in P.items()}
    grad["y_hat"] = yh.grad.double().numpy()
    return {"fm": float(fm.detach()), "gen": float(gen.detach()), "disc": float(disc.detach()), "r_losses": r_l.detach().double().numpy(),
            "g_losses": g_l.detach().double().numpy(), "out_r": [r.detach().double().numpy() for r in rs],
            "out_g": [g.detach().double().numpy() for g in gs], "grad": grad, "grad_y": y.grad.double().numpy(),
            "fmap_r": [[m.detach() for m in f] for f in frs], "fmap_g": [[m.detach() for m in f] for f in fgs]}


def make_state(channels, periods=PERIODS, seed=0, gain=3.0):
    """the fixtures' weight recipe at any widths: torch's default Conv2d init under manual_seed(seed), weight_g = gain *
    ||weight_v[i]||, biases U(-0.3, 0.3) -> state dict of float32 tensors with the reference's keys"""
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    for i, _ in enumerate(periods):
        cin = 1
        for l, (c, k) in enumerate(list(zip(channels, (5,) * 5)) + [(1, 3)]):
            pre = f"discriminators.{i}." + (f"convs.{l}." if l < 5 else "conv_post.")
            bound = 1.0 / math.sqrt(cin * k)
            v = (torch.rand(c, cin, k, 1, generator=gen) * 2 - 1) * bound
            sd[pre + "weight_g"] = gain * v.reshape(c, -1).norm(dim=1).reshape(c, 1, 1, 1)
            sd[pre + "weight_v"] = v
            sd[pre + "bias"] = (torch.rand(c, generator=gen) * 2 - 1) * 0.3
            cin = c
    return sd


def kink_ratios(sd, y, y_hat, len_ratios=None, periods=PERIODS):
    """(smallest |leaky-relu input| of the float64 run / largest |x32 - x64|, the same for r - g over the counted rows of
    every feature map): above KINK_FACTOR no kink decision differs between fp32 and float64"""
    got = {}
    for dt in (torch.float64, torch.float32):
        P = {k: torch.as_tensor(v).to(dt) for k, v in sd.items()}
        inputs = []
        with torch.no_grad():
            _, _, frs, fgs = mpd_forward(P, torch.as_tensor(y).to(dt), torch.as_tensor(y_hat).to(dt), periods, None, inputs)
        diffs = []
        for fr, fg in zip(frs, fgs):
            for r, g in zip(fr, fg):
                d = (r - g).double()
                if len_ratios is not None:
                    n = counts(torch.as_tensor(len_ratios), r.shape[2])
                    d = d[_mask(n, r.shape[2], torch.bool)[:, None, :, None].expand_as(d)]
                diffs.append(d.reshape(-1))
        got[dt] = (torch.cat(inputs), torch.cat(diffs))
    (i64, d64), (i32, d32) = got[torch.float64], got[torch.float32]
    return (float(i64.abs().min() / (i32 - i64).abs().max()), float(d64.abs().min() / (d32 - d64).abs().max()))


def _dW(sd, grad, prefix):
    """(dW, v / ||v||) of a one-channel conv, dW recovered from the float64 gradients of weight_v and weight_g:
    dW = dv * ||v|| / g + v / ||v|| * dg"""
    v, g = torch.as_tensor(sd[prefix + "weight_v"]).double(), torch.as_tensor(sd[prefix + "weight_g"]).double()
    assert v.shape[0] == 1
    n = v.norm()
    return torch.as_tensor(grad[prefix + "weight_v"]) * n / g + v / n * torch.as_tensor(grad[prefix + "weight_g"]), v / n


def weight_g_condition(sd, grad, prefix):
    """sum |t| / |sum t| over the terms t = dW * v / ||v|| of a one-channel conv's weight_g gradient"""
    dW, vh = _dW(sd, grad, prefix)
    t = dW * vh
    return float(t.abs().sum() / t.sum().abs())


def weight_g_amplification(sd, grad, prefix):
    """||dW|| / |<dW, v / ||v||>|: the weight_g gradient is <dW, v^>, so an error e * ||dW|| of dW (relative L2 e) moves
    it by at most e * ||dW|| (Cauchy-Schwarz, ||v^|| = 1), i.e. by at most e times this number relative to itself"""
    dW, vh = _dW(sd, grad, prefix)
    return float(dW.norm() / (dW * vh).sum().abs())


KINK_FACTOR = 8.0


def relative_l2(a, b):
    import numpy as np
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
