"""float64 gradients of the reference's WaveGlow training loss: forward_ref / nll_ref of _waveglow_fwd_ref.py on
requires_grad leaves (the folded weights, or weight_g / weight_v through the float64 fold of _vocoder_ref._w), autograd
does the rest.  Pinned against the reference by tests/golden/waveglow_bwd_tiny.npz (tests/test_waveglow_bwd_cpu.py)."""
import numpy as np
import torch

from _waveglow_fwd_ref import forward_ref
from _waveglow_ref import HOP


def leaves_of(sd):
    """state_dict (either form) -> float64 leaves that require a gradient, same keys"""
    return {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()}


def numerator_ref(leaves, cfg, mel, audio, sigma=1.0):
    """sum z^2 / (2 sigma^2) - sum log_s - n_groups * sum_k log|det W_k| of ONE utterance (the likelihood before its
    normalisation) and its number of group steps"""
    z, log_s_sums, logdets = forward_ref(leaves, cfg, mel, audio)
    n_groups = z.size(2)
    return (z * z).sum() / (2.0 * sigma * sigma) - sum(log_s_sums) - n_groups * sum(logdets), n_groups


def loss_ref(leaves, cfg, mel, audio, lens, sigma=1.0):
    """the ragged loss of WaveGlow.analyze / nll_loss: the items' numerators, each item run alone at its own length,
    over sum_b n_groups[b] * n_group (with equal lengths: the reference's WaveGlowLoss)"""
    num, n = 0.0, 0
    for b, t in enumerate(lens):
        nb, gb = numerator_ref(leaves, cfg, mel[b:b + 1, :, :t], audio[b:b + 1, :t * HOP], sigma)
        num, n = num + nb, n + gb
    return num / (n * cfg["n_group"])


def grads_ref(sd, cfg, mel, audio, lens, sigma=1.0):
    """-> (loss, {name: float64 gradient}) with the keys of sd"""
    leaves = leaves_of(sd)
    loss = loss_ref(leaves, cfg, mel, audio, lens, sigma)
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in leaves.items()}


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def unfolded(sd_folded, normed_names):
    """folded state_dict -> the weight-normed form (g = the rows' norms, v = the weight) for the convs in normed_names"""
    out = {}
    for k, v in sd_folded.items():
        base = k[:-len(".weight")] if k.endswith(".weight") else None
        if base in normed_names:
            out[base + ".weight_g"] = v.reshape(v.shape[0], -1).norm(dim=1).reshape(-1, 1, 1)
            out[base + ".weight_v"] = v.clone()
        else:
            out[k] = v
    return out
