"""fp64 restatement of the reference's HiFi-GAN Generator and STFT Denoiser with torch.nn.functional (one utterance
at a time, as the reference runs them), for the vocoder tests.  Pinned against the reference by
tests/golden/vocoder_*.npz (tests/test_vocoder_cpu.py)."""
import json

import numpy as np
import torch
import torch.nn.functional as F

V1 = dict(resblock="1", upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=512,
          resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]],
          gaussian_blur={"p_blurring": 0.0})
V3 = dict(resblock="2", upsample_rates=[8, 8, 4], upsample_kernel_sizes=[16, 16, 8], upsample_initial_channel=256,
          resblock_kernel_sizes=[3, 5, 7], resblock_dilation_sizes=[[1, 2], [2, 6], [3, 12]],
          gaussian_blur={"p_blurring": 0.0})


def random_state(gen_module, seed, g_lo=0.5, g_hi=1.5):
    """weight_v ~ N(0, 1), weight_g ~ U(g_lo, g_hi), bias ~ N(0, 0.1) (as make_golden_vocoder.py)"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in gen_module.state_dict().items():
        if k.endswith("weight_v"):
            sd[k] = torch.randn(v.shape, generator=g)
        elif k.endswith("weight_g"):
            sd[k] = g_lo + (g_hi - g_lo) * torch.rand(v.shape, generator=g)
        else:
            sd[k] = 0.1 * torch.randn(v.shape, generator=g)
    return sd


def load_fixture(d):
    cfg = json.loads(str(d["config"]))
    sd = {k[3:]: torch.from_numpy(v) for k, v in d.items() if k.startswith("sd/")}
    return cfg, sd


def _w(sd, name):
    if name + ".weight_g" in sd:
        v, g = sd[name + ".weight_v"].double(), sd[name + ".weight_g"].double()
        n = v.reshape(v.shape[0], -1).norm(dim=1).reshape((-1,) + (1,) * (v.dim() - 1))
        return v * (g / n)
    return sd[name + ".weight"].double()


def _new_keys(sd):
    out = {}
    for k, v in sd.items():
        p = k.split(".")
        if p[0] == "resblocks" and len(p) == 5:
            k = f"resblocks.{int(p[1]) // 3}.{int(p[1]) % 3}.{'.'.join(p[2:])}"
        out[k] = v
    return out


def generator_ref(sd, cfg, mel):
    """mel [1, 80, T] -> audio [1, 1, T*hop], fp64"""
    sd = _new_keys(sd)
    b = lambda n: sd[n + ".bias"].double()
    x = F.conv1d(mel.double(), _w(sd, "conv_pre"), b("conv_pre"), padding=3)
    nk = len(cfg["resblock_kernel_sizes"])
    for i, (u, k) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
        x = F.leaky_relu(x, 0.1)
        x = F.conv_transpose1d(x, _w(sd, f"ups.{i}"), b(f"ups.{i}"), stride=u, padding=(k - u) // 2)
        xs = None
        for j, (ks, ds) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"])):
            pre = f"resblocks.{i}.{j}"
            y = x
            if cfg["resblock"] == "1":
                for n, d in enumerate(ds):
                    t = F.leaky_relu(y, 0.1)
                    t = F.conv1d(t, _w(sd, f"{pre}.convs1.{n}"), b(f"{pre}.convs1.{n}"), dilation=d,
                                 padding=(ks * d - d) // 2)
                    t = F.leaky_relu(t, 0.1)
                    t = F.conv1d(t, _w(sd, f"{pre}.convs2.{n}"), b(f"{pre}.convs2.{n}"), padding=(ks - 1) // 2)
                    y = t + y
            else:
                for n, d in enumerate(ds):
                    t = F.leaky_relu(y, 0.1)
                    t = F.conv1d(t, _w(sd, f"{pre}.convs.{n}"), b(f"{pre}.convs.{n}"), dilation=d,
                                 padding=(ks * d - d) // 2)
                    y = t + y
            xs = y if xs is None else xs + y
        x = xs / nk
    x = F.leaky_relu(x)
    x = F.conv1d(x, _w(sd, "conv_post"), b("conv_post"), padding=3)
    return torch.tanh(x)


def _bases(n_fft=1024, hop=256):
    cutoff = n_fft // 2 + 1
    fb = np.fft.fft(np.eye(n_fft))
    fourier = np.vstack([np.real(fb[:cutoff]), np.imag(fb[:cutoff])])
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)
    fwd = torch.from_numpy(fourier * win)[:, None, :]
    inv = torch.from_numpy(np.linalg.pinv((n_fft / hop) * fourier).T * win)[:, None, :]
    return fwd, inv, win ** 2, cutoff


def stft_mag_ref(audio, n_fft=1024, hop=256):
    """audio [1, S] -> (magnitude, phase) [1, cutoff, F], fp64"""
    fwd, _, _, cutoff = _bases(n_fft, hop)
    x = F.pad(audio.double()[:, None, None, :], (n_fft // 2, n_fft // 2, 0, 0), mode="reflect")[:, 0]
    ft = F.conv1d(x, fwd, stride=hop)
    re, im = ft[:, :cutoff], ft[:, cutoff:]
    return torch.sqrt(re ** 2 + im ** 2), torch.atan2(im, re)


def denoise_ref(audio, bias_spec, strength, n_fft=1024, hop=256):
    """audio [1, S], bias_spec [cutoff] -> [S // hop * hop], fp64"""
    _, inv, winsq, cutoff = _bases(n_fft, hop)
    mag, ph = stft_mag_ref(audio, n_fft, hop)
    mag = torch.clamp(mag - bias_spec.double()[None, :, None] * strength, 0.0)
    y = F.conv_transpose1d(torch.cat([mag * torch.cos(ph), mag * torch.sin(ph)], 1), inv, stride=hop)
    nf = mag.shape[-1]
    n = n_fft + hop * (nf - 1)
    ws = np.zeros(n)
    for i in range(nf):
        s = i * hop
        ws[s:min(n, s + n_fft)] += winsq[:max(0, min(n_fft, n - s))]
    nz = ws > np.finfo(np.float32).tiny
    y = y[0, 0]
    y[torch.from_numpy(nz)] /= torch.from_numpy(ws[nz])
    y = y * (float(n_fft) / hop)
    return y[n_fft // 2:-(n_fft // 2)]
