"""fp64 restatement of the reference's WaveGlow.infer and its Denoiser with torch.nn.functional (one utterance at a
time, as the reference runs them), for the WaveGlow tests.  Pinned against the reference by tests/golden/waveglow_*.npz
(tests/test_waveglow_cpu.py).  The STFT is the one of _vocoder_ref (tacotron2/stft.py and audio_processing.py agree)."""
import json

import numpy as np
import torch
import torch.nn.functional as F

from _vocoder_ref import _w, denoise_ref, stft_mag_ref  # noqa: F401  (re-exported for the tests)

HOP, UP_KERNEL = 256, 1024
TINY = dict(n_mel_channels=8, n_flows=6, n_group=8, n_early_every=2, n_early_size=2,
            WN_config=dict(n_layers=4, n_channels=32, kernel_size=3))
SHIPPED_WN = dict(n_layers=8, n_channels=256, kernel_size=3)


def load_fixture(d):
    """-> (config, state_dict as fp32 tensors); 'sd/' arrays are stored as float16 values, exactly"""
    cfg = json.loads(str(d["config"]))
    sd = {k[3:]: torch.from_numpy(v.astype(np.float32)) for k, v in d.items() if k.startswith("sd/")}
    if "up_a" in d:                       # the denoiser fixture's upsample weight: an outer product, expanded here
        sd["upsample.weight"] = expand_upsample(d["up_a"], d["up_v"])
    return cfg, sd


def expand_upsample(a, v):
    """[n_mel, n_mel] x [k] -> the ConvTranspose1d weight [n_mel, n_mel, k], fp32 product of the fp32 factors"""
    a = torch.from_numpy(np.asarray(a, dtype=np.float32))
    v = torch.from_numpy(np.asarray(v, dtype=np.float32))
    return a[:, :, None] * v[None, None, :]


def channel_plan(cfg):
    """per flow k: number of channels the flow works on"""
    n_rem, out = cfg["n_group"], []
    for k in range(cfg["n_flows"]):
        if k % cfg["n_early_every"] == 0 and k > 0:
            n_rem -= cfg["n_early_size"]
        out.append(n_rem)
    return out


def noise_channels(cfg):
    plan = channel_plan(cfg)
    early = [k for k in reversed(range(cfg["n_flows"])) if k % cfg["n_early_every"] == 0 and k > 0]
    return [plan[-1]] + [cfg["n_early_size"]] * len(early)


def random_state(cfg, seed, end_std=0.05):
    """folded-key state_dict: weights ~ N(0, 1/fan_in) so that activations stay O(1) at any width, biases ~ N(0, 0.1),
    end ~ N(0, end_std), convinv orthogonal (seeded CPU generator)"""
    g = torch.Generator().manual_seed(seed)
    n_mel, ng = cfg["n_mel_channels"], cfg["n_group"]
    wn = cfg["WN_config"]
    C, L, ks = wn["n_channels"], wn["n_layers"], wn["kernel_size"]

    def w(*shape, fan):
        return torch.randn(*shape, generator=g) / np.sqrt(fan)

    sd = {"upsample.weight": w(n_mel, n_mel, UP_KERNEL, fan=4 * n_mel), "upsample.bias": 0.1 * torch.randn(n_mel, generator=g)}
    for k, c in enumerate(channel_plan(cfg)):
        nh = c // 2
        p = f"WN.{k}."
        sd[p + "start.weight"], sd[p + "start.bias"] = w(C, nh, 1, fan=nh), 0.1 * torch.randn(C, generator=g)
        sd[p + "cond_layer.weight"] = w(2 * C * L, n_mel * ng, 1, fan=n_mel * ng)
        sd[p + "cond_layer.bias"] = 0.1 * torch.randn(2 * C * L, generator=g)
        for i in range(L):
            sd[p + f"in_layers.{i}.weight"] = w(2 * C, C, ks, fan=C * ks)
            sd[p + f"in_layers.{i}.bias"] = 0.1 * torch.randn(2 * C, generator=g)
            n = 2 * C if i < L - 1 else C
            sd[p + f"res_skip_layers.{i}.weight"] = w(n, C, 1, fan=C)
            sd[p + f"res_skip_layers.{i}.bias"] = 0.1 * torch.randn(n, generator=g)
        sd[p + "end.weight"] = end_std * torch.randn(2 * nh, C, 1, generator=g) / np.sqrt(C / 32)
        sd[p + "end.bias"] = end_std * torch.randn(2 * nh, generator=g)
        q = torch.linalg.qr(torch.randn(c, c, generator=g))[0]
        sd[f"convinv.{k}.conv.weight"] = q.reshape(c, c, 1).contiguous()
    return sd


def wn_ref(sd, k, cfg, audio0, spect):
    wn = cfg["WN_config"]
    C, L, ks = wn["n_channels"], wn["n_layers"], wn["kernel_size"]
    p = f"WN.{k}."
    b = lambda n: sd[p + n + ".bias"].double()
    audio = F.conv1d(audio0, _w(sd, p + "start"), b("start"))
    output = torch.zeros_like(audio)
    cond = F.conv1d(spect, _w(sd, p + "cond_layer"), b("cond_layer"))
    for i in range(L):
        d = 2 ** i
        a = F.conv1d(audio, _w(sd, p + f"in_layers.{i}"), b(f"in_layers.{i}"), dilation=d, padding=(ks * d - d) // 2)
        a = a + cond[:, 2 * C * i:2 * C * (i + 1)]
        acts = torch.tanh(a[:, :C]) * torch.sigmoid(a[:, C:])
        rs = F.conv1d(acts, _w(sd, p + f"res_skip_layers.{i}"), b(f"res_skip_layers.{i}"))
        if i < L - 1:
            audio = audio + rs[:, :C]
            output = output + rs[:, C:]
        else:
            output = output + rs
    return F.conv1d(output, sd[p + "end.weight"].double(), b("end"))


def group_cond_ref(sd, cfg, mel):
    """mel [1, n_mel, T] -> the grouped conditioning [1, n_mel*n_group, T*HOP/n_group], fp64"""
    ng = cfg["n_group"]
    spect = F.conv_transpose1d(mel.double(), sd["upsample.weight"].double(), sd["upsample.bias"].double(), stride=HOP)
    spect = spect[:, :, :-(UP_KERNEL - HOP)]
    spect = spect.unfold(2, ng, ng).permute(0, 2, 1, 3)
    return spect.contiguous().view(spect.size(0), spect.size(1), -1).permute(0, 2, 1)


def infer_ref(sd, cfg, mel, sigma, noise):
    """mel [1, n_mel, T], noise: the draws [1, ch, Tg] in the reference's order -> audio [1, T*HOP], fp64"""
    spect = group_cond_ref(sd, cfg, mel)
    noise = [z.double() for z in noise]
    audio = sigma * noise[0]
    zi = 1
    for k in reversed(range(cfg["n_flows"])):
        nh = audio.size(1) // 2
        a0, a1 = audio[:, :nh], audio[:, nh:]
        out = wn_ref(sd, k, cfg, a0, spect)
        s, b = out[:, nh:], out[:, :nh]
        a1 = (a1 - b) / torch.exp(s)
        audio = torch.cat([a0, a1], 1)
        Winv = torch.linalg.inv(sd[f"convinv.{k}.conv.weight"][:, :, 0].double())
        audio = F.conv1d(audio, Winv[:, :, None])
        if k % cfg["n_early_every"] == 0 and k > 0:
            audio = torch.cat((sigma * noise[zi], audio), 1)
            zi += 1
    return audio.permute(0, 2, 1).contiguous().view(audio.size(0), -1)


def bias_spec_ref(sd, cfg):
    """the denoiser's bias spectrum [cutoff], fp64"""
    Tg = 88 * HOP // cfg["n_group"]
    zeros = [torch.zeros(1, ch, Tg) for ch in noise_channels(cfg)]
    audio = infer_ref(sd, cfg, torch.zeros(1, cfg["n_mel_channels"], 88), 0.0, zeros)
    return stft_mag_ref(audio)[0][0, :, 0]
