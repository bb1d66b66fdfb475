#!/usr/bin/env python3
"""Generate tests/golden/vocoder_*.npz by RUNNING THE REFERENCE's HiFi-GAN Generator, Denoiser and STFT
(vocoders/hifigan_models.py, vocoders/hifigan_denoiser.py, audio_processing.py) on the CPU:

    python tests/golden/make_golden_vocoder.py [--ref /root/reference]

Same stand-ins as make_golden.py (librosa is absent; pad_center / tiny / normalize(norm=None) are restated there).
Weights are random from a seed (weight_v ~ N(0, 1), weight_g ~ U(0.5, 1.5), bias ~ N(0, 0.1)) so that every layer
carries signal; the fixtures hold the config, the state_dict, the inputs and the reference's per-utterance outputs.
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

# small resblock '1' config with three kernels per stage (the old checkpoint key format needs N // 3, N % 3)
CFG_R1 = dict(resblock="1", upsample_rates=[4, 4], upsample_kernel_sizes=[8, 8], upsample_initial_channel=32,
              resblock_kernel_sizes=[3, 5, 7], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]],
              gaussian_blur={"p_blurring": 0.0})
# V3's rates / kernels / resblock '2' at reduced channels (hop 256, the denoiser's)
CFG_R2 = dict(resblock="2", upsample_rates=[8, 8, 4], upsample_kernel_sizes=[16, 16, 8], upsample_initial_channel=32,
              resblock_kernel_sizes=[3, 5, 7], resblock_dilation_sizes=[[1, 2], [2, 6], [3, 12]],
              gaussian_blur={"p_blurring": 0.0})


def randomize(gen, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in gen.state_dict().items():
        if k.endswith("weight_v"):
            sd[k] = torch.randn(v.shape, generator=g)
        elif k.endswith("weight_g"):
            sd[k] = 0.5 + torch.rand(v.shape, generator=g)
        else:
            sd[k] = 0.1 * torch.randn(v.shape, generator=g)
    return sd


def old_keys(sd):
    """resblocks.{i}.{j}.* -> resblocks.{3i + j}.* (the checkpoint format Generator.load_state_dict remaps)"""
    out = {}
    for k, v in sd.items():
        p = k.split(".")
        if p[0] == "resblocks":
            k = ".".join(["resblocks", str(int(p[1]) * 3 + int(p[2]))] + p[3:])
        out[k] = v
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    from make_golden import install_stubs, save
    install_stubs()
    import librosa.util as lu
    lu.normalize = lambda S, norm=None, **k: S
    sys.path[:0] = [args.ref, os.path.join(args.ref, "vocoders")]
    os.chdir("/tmp")
    import torch
    from hifigan_env import AttrDict
    from hifigan_models import Generator
    from hifigan_denoiser import Denoiser
    torch.manual_seed(0)
    torch.set_grad_enabled(False)

    gens = {}
    for name, cfg, seed, lens, old in (("r1", CFG_R1, 11, [12, 7, 1], True), ("r2", CFG_R2, 12, [9, 5, 3], False)):
        h = AttrDict(json.loads(json.dumps(cfg)))
        gen = Generator(h)
        sd = randomize(gen, seed)
        gen.load_state_dict(old_keys(sd) if old else sd)
        gen.eval()
        gens[name] = gen
        T = max(lens)
        g = torch.Generator().manual_seed(seed + 100)
        mel = torch.randn(len(lens), 80, T, generator=g) - 2.0
        hop = int(np.prod(cfg["upsample_rates"]))
        audio = np.zeros((len(lens), T * hop), np.float32)
        for b, n in enumerate(lens):
            audio[b, :n * hop] = gen(mel[b:b + 1, :, :n])[0, 0].numpy()
        stored = old_keys(sd) if old else sd
        arrs = {"sd/" + k: v.numpy() for k, v in stored.items()}
        save(f"vocoder_gen_{name}.npz", config=np.array(json.dumps(cfg)), mel=mel.numpy(), lens=np.array(lens),
             audio=audio, old_keys=np.array(old), **arrs)

    # denoiser on the resblock '2' generator (hop 256): bias spectrum + two strengths, per item at its own length
    den = Denoiser(gens["r2"])
    g = torch.Generator().manual_seed(21)
    lens = [4 * 256, 3 * 256, 9 * 256 + 100]
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
    save("vocoder_denoiser.npz", audio=audio.numpy(), lens=np.array(lens), bias_spec=den.bias_spec[0, :, 0].numpy(),
         **out)


if __name__ == "__main__":
    main()
