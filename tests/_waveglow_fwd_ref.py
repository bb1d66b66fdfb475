"""float64 restatement of the reference's WaveGlow.forward and WaveGlowLoss (vocoders/waveglow_for_LIMMITS23/glow.py:43-59,
207-249) with torch.nn.functional, one utterance at a time, written against wn_ref of _waveglow_ref.py.  Pinned against
the reference by tests/golden/waveglow_fwd_tiny.npz (tests/test_waveglow_fwd_cpu.py)."""
import torch
import torch.nn.functional as F

from _waveglow_ref import group_cond_ref, wn_ref


def forward_ref(sd, cfg, mel, audio):
    """mel [1, n_mel, T], audio [1, T*HOP] -> (z [1, n_group, Tg], [sum of log_s per flow], [log|det W_k| per flow]),
    float64; sd holds the folded keys"""
    ng = cfg["n_group"]
    spect = group_cond_ref(sd, cfg, mel)
    x = audio.double().unfold(1, ng, ng).permute(0, 2, 1)
    out, log_s_sums, logdets = [], [], []
    for k in range(cfg["n_flows"]):
        if k % cfg["n_early_every"] == 0 and k > 0:
            out.append(x[:, :cfg["n_early_size"]])
            x = x[:, cfg["n_early_size"]:]
        W = sd[f"convinv.{k}.conv.weight"][:, :, 0].double()
        logdets.append(torch.linalg.slogdet(W)[1])
        x = F.conv1d(x, W[:, :, None])
        nh = x.size(1) // 2
        x0, x1 = x[:, :nh], x[:, nh:]
        o = wn_ref(sd, k, cfg, x0, spect)
        b, log_s = o[:, :nh], o[:, nh:]
        x = torch.cat([x0, torch.exp(log_s) * x1 + b], 1)
        log_s_sums.append(log_s.sum())
    out.append(x)
    return torch.cat(out, 1), log_s_sums, logdets


def nll_ref(z, log_s_sums, logdets, sigma=1.0):
    """WaveGlowLoss for ONE utterance (or a batch of equal lengths given its summed terms): nats per sample"""
    n_groups = z.size(0) * z.size(2)
    total = (z * z).sum() / (2.0 * sigma * sigma) - sum(log_s_sums) - n_groups * sum(logdets)
    return total / z.numel()


def noise_from_z_ref(cfg, z):
    """z [1, n_group, Tg] -> the draws of infer_ref's `noise`: the channels left after every early exit, then the early
    blocks from the latest exit to the earliest"""
    n_early = cfg["n_early_size"]
    exits = len([k for k in range(cfg["n_flows"]) if k % cfg["n_early_every"] == 0 and k > 0])
    lo = exits * n_early
    out = [z[:, lo:]]
    while lo > 0:
        out.append(z[:, lo - n_early:lo])
        lo -= n_early
    return out
