#!/usr/bin/env python3
"""Generate tests/golden/waveglow_*.npz by RUNNING THE REFERENCE's WaveGlow.infer and Denoiser
(vocoders/waveglow_for_LIMMITS23/glow.py, denoiser.py, tacotron2/stft.py) on the CPU:

    python tests/golden/make_golden_waveglow.py [--ref /root/reference]

Same stand-ins as make_golden_vocoder.py (librosa is absent; pad_center / tiny / normalize(norm=None) are restated in
make_golden.py).  The reference draws its noise with torch.cuda.FloatTensor(...).normal_() and moves its STFT with
.cuda(): those names are replaced by CPU factories that record every draw, the reference's own code then runs
unmodified and the draws land in the fixture.  Each WN.end is re-initialised with N(0, 0.05) weights and biases (the
reference's zeros would make every coupling the identity).  Every weight is rounded to a float16 value BEFORE it is
loaded into the reference model and stored as float16, exactly (that halves the files; the arithmetic is fp32).  The
fixtures hold the config, the weight-normed state_dict, the inputs, the recorded draws and the reference's outputs of
each item run alone at its own length.
"""
import argparse
import copy
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

TINY = dict(n_mel_channels=8, n_flows=6, n_group=8, n_early_every=2, n_early_size=2,
            WN_config=dict(n_layers=4, n_channels=32, kernel_size=3))
DEN = dict(n_mel_channels=80, n_flows=6, n_group=8, n_early_every=2, n_early_size=2,
           WN_config=dict(n_layers=2, n_channels=16, kernel_size=3))


class Draws:
    """stand-in for torch.cuda.FloatTensor: FloatTensor(*shape).normal_() draws on the CPU and is recorded; with
    `replay` set the recorded draws come back in order, cast to `dtype` (the float64 run of the same utterance)"""
    record, replay, dtype, gen = [], None, None, None

    def __init__(self, *shape):
        self.shape = shape

    def normal_(self):
        import torch
        if Draws.replay is not None:
            return Draws.replay.pop(0).to(Draws.dtype)
        z = torch.randn(*self.shape, generator=Draws.gen)
        Draws.record.append(z)
        return z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    from make_golden import install_stubs, save
    install_stubs()
    import librosa.util as lu
    lu.normalize = lambda S, norm=None, **k: S
    wg_dir = os.path.join(args.ref, "vocoders", "waveglow_for_LIMMITS23")
    sys.path[:0] = [wg_dir, os.path.join(wg_dir, "tacotron2")]
    os.chdir("/tmp")
    import torch
    torch.cuda.FloatTensor = Draws
    torch.nn.Module.cuda = lambda self, *a, **k: self
    torch.Tensor.cuda = lambda self, *a, **k: self
    from glow import WaveGlow
    from denoiser import Denoiser
    torch.set_grad_enabled(False)
    Draws.gen = torch.Generator().manual_seed(1234)

    def build(cfg, seed, upsample=None):
        torch.manual_seed(seed)
        m = WaveGlow(**json.loads(json.dumps(cfg)))
        g = torch.Generator().manual_seed(seed + 1)
        for wn in m.WN:
            wn.end.weight.data = 0.05 * torch.randn(wn.end.weight.shape, generator=g)
            wn.end.bias.data = 0.05 * torch.randn(wn.end.bias.shape, generator=g)
        if upsample is not None:
            m.upsample.weight.data = upsample
        for p in m.parameters():
            p.data = p.data.half().float()
        sd = {k: v.clone() for k, v in m.state_dict().items()}          # weight-normed keys
        m = WaveGlow.remove_weightnorm(m)
        return m.eval(), sd

    def sd_arrays(sd, skip=()):
        out = {}
        for k, v in sd.items():
            if k in skip:
                continue
            h = v.numpy().astype(np.float16)
            assert np.array_equal(h.astype(np.float32), v.numpy()), k
            out["sd/" + k] = h
        return out

    # ---- waveglow_tiny.npz ------------------------------------------------------------------------------------
    m, sd = build(TINY, 31)
    m64 = copy.deepcopy(m).double()
    for inv in m64.convinv:         # the reference caches W.float().inverse(): give the float64 copy a float64 cache
        inv.W_inverse = inv.conv.weight.squeeze().inverse()[..., None]
    lens, sigma = [7, 4], 0.8
    T, ng = max(lens), TINY["n_group"]
    Tg = T * 256 // ng
    mel = torch.randn(len(lens), 8, T, generator=torch.Generator().manual_seed(32)) - 2.0
    audio = np.zeros((len(lens), T * 256), np.float32)
    noise, worst, peak = None, 0.0, 0.0
    for b, n in enumerate(lens):
        Draws.record, Draws.replay = [], None
        y = m.infer(mel[b:b + 1, :, :n], sigma=sigma)[0]
        draws = Draws.record
        Draws.replay, Draws.dtype = [z.clone() for z in draws], torch.float64
        y64 = m64.infer(mel[b:b + 1, :, :n].double(), sigma=sigma)[0]
        Draws.replay = None
        worst = max(worst, (y.double() - y64).abs().max().item())
        peak = max(peak, y64.abs().max().item())
        audio[b, :n * 256] = y.numpy()
        if noise is None:
            noise = [np.zeros((len(lens), z.shape[1], Tg), np.float32) for z in draws]
        for dst, z in zip(noise, draws):
            dst[b, :, :z.shape[2]] = z[0].numpy()
    print(f"waveglow_tiny: reference float32 vs float64 max-abs {worst:.3e} at |ref| max {peak:.3f}")
    assert worst <= 1e-5
    save("waveglow_tiny.npz", config=np.array(json.dumps(TINY)), mel=mel.numpy(), lens=np.array(lens),
         sigma=np.array(sigma), audio=audio, f32_vs_f64=np.array(worst),
         **{f"noise{i}": z for i, z in enumerate(noise)}, **sd_arrays(sd))

    # ---- waveglow_denoiser.npz ----------------------------------------------------------------------------------
    g = torch.Generator().manual_seed(41)
    up_a = (torch.randn(80, 80, generator=g) / 80 ** 0.5).half().float()
    up_v = (torch.randn(1024, generator=g) * 0.5).half().float()
    # the product of two float16 values is exact in fp32, but not a float16 value: the weight travels as its factors
    m, sd = build(DEN, 43, upsample=None)
    m.upsample.weight.data = up_a[:, :, None] * up_v[None, None, :]
    Draws.record, Draws.replay = [], None
    den = Denoiser(m)
    lens = [4 * 256, 6 * 256 + 100]
    S = max(lens)
    audio = torch.zeros(len(lens), S)
    for b, n in enumerate(lens):
        audio[b, :n] = 0.3 * torch.randn(n, generator=g) + 0.5 * torch.sin(torch.arange(n) * (0.05 + 0.02 * b))
    out = {}
    for tag, strength in (("s0p1", 0.1), ("s0p001", 0.001)):
        y = np.zeros((len(lens), S), np.float32)
        for b, n in enumerate(lens):
            r = den(audio[b:b + 1, :n], strength=strength)[0, 0].numpy()
            y[b, :r.shape[0]] = r
        out["out_" + tag] = y
    save("waveglow_denoiser.npz", config=np.array(json.dumps(DEN)), audio=audio.numpy(), lens=np.array(lens),
         bias_spec=den.bias_spec[0, :, 0].numpy(), up_a=up_a.numpy(), up_v=up_v.numpy(),
         **out, **sd_arrays(sd, skip=("upsample.weight",)))


if __name__ == "__main__":
    main()
