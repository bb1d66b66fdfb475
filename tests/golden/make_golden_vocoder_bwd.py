#!/usr/bin/env python3
"""Generate tests/golden/vocoder_gen_bwd_r1.npz / _r2.npz by RUNNING THE REFERENCE's HiFi-GAN Generator
(vocoders/hifigan_models.py:172-247) and torch autograd on the CPU:

    python tests/golden/make_golden_vocoder_bwd.py --ref <checkout of the reference>

It reads config and sd/* from vocoder_gen_r1.npz / vocoder_gen_r2.npz (make_golden_vocoder.py) and stores none of them
again.  The reference's Generator is built with that config, weight norm left on (the state of a training
checkpoint), loaded with sd/*, and run on each utterance of a ragged batch at its own length, as the reference runs
them (lengths [4, 2, 1] frames for r1, [3, 2, 1] for r2: the one-frame item is the edge case), once in float64 and once
in float32, with the loss

    L = sum_b sum_t (y_b[t] - target_b[t])^2 / N,   N = the number of valid samples, target random and stored.

The kink condition.  The generator is full of leaky-relu kinks: an input whose sign differs between float64 and fp32
moves the affected gradients by about 1e-3.  The script therefore searches mel seeds (mel ~ N(-2, 1), seed
MEL_SEED0 + n) for the first one where no leaky-relu input of the float64 run is closer to 0 than KINK_FACTOR times the
largest |x32 - x64| that the reference's own float32 run shows on any leaky-relu input; it asserts this and stores both
numbers (kink_min_abs, kink_max_dev) with the seed.

The fixture holds mel, lens, target, loss64, loss32, mel_seed, the two kink numbers and, per parameter <name> of the
reference (weight_g / weight_v) and for mel:
    grad/<name>        the float64 gradient, stored as float32
    f32_vs_f64/<name>  ||grad32 - grad64|| / ||grad64||: the reference's own float32 deviation
The generator asserts that no gradient is identically zero and that each file stays below 1 MiB.

One thread and a zip archive with fixed time stamps: two runs write the same bytes.
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
KINK_FACTOR = 8.0
MEL_SEED0 = 500
MAX_SEEDS = 400
CASES = (("r1", [4, 2, 1], 31), ("r2", [3, 2, 1], 32))       # fixture, lengths in frames, seed of the target


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project")
    args = ap.parse_args()
    from make_golden import install_stubs
    from make_golden_waveglow_fwd import save
    install_stubs()
    sys.path[:0] = [args.ref, os.path.join(args.ref, "vocoders")]
    os.chdir("/tmp")
    import torch
    import torch.nn.functional as F
    torch.set_num_threads(1)
    from hifigan_env import AttrDict
    from hifigan_models import Generator

    seen = []
    stock_lrelu = F.leaky_relu

    def recording_lrelu(x, *a, **k):
        seen.append(x.detach().double().reshape(-1))
        return stock_lrelu(x, *a, **k)

    for name, lens, tseed in CASES:
        d = np.load(os.path.join(HERE, f"vocoder_gen_{name}.npz"))
        cfg = json.loads(str(d["config"]))
        sd = {k[3:]: torch.from_numpy(d[k].astype(np.float32)) for k in d.files if k.startswith("sd/")}
        hop = int(np.prod(cfg["upsample_rates"]))
        B, T = len(lens), max(lens)
        N = sum(lens) * hop
        torch.manual_seed(0)
        models = {}
        for dt in (torch.float64, torch.float32):
            m = Generator(AttrDict(json.loads(json.dumps(cfg))))
            m.load_state_dict({k: v.clone() for k, v in sd.items()})
            models[dt] = m.to(dt).train()
        target = torch.rand(B, T * hop, generator=torch.Generator().manual_seed(tseed)) * 2 - 1        # float32, as stored

        def run(dt, mel):
            """-> (loss, {name: grad float64 numpy}, every leaky-relu input of the run)"""
            m = models[dt]
            m.zero_grad()
            x = mel.to(dt).clone().requires_grad_(True)
            del seen[:]
            F.leaky_relu = recording_lrelu
            try:
                loss = 0.0
                for b, n in enumerate(lens):
                    y = m(x[b:b + 1, :, :n])[0, 0]
                    loss = loss + ((y - target[b, :n * hop].to(dt)) ** 2).sum() / N
            finally:
                F.leaky_relu = stock_lrelu
            loss.backward()
            g = {k: p.grad.double().numpy() for k, p in m.named_parameters()}
            g["mel"] = x.grad.double().numpy()
            return float(loss.item()), g, torch.cat(seen)

        for n in range(MAX_SEEDS):
            mel = torch.randn(B, 80, T, generator=torch.Generator().manual_seed(MEL_SEED0 + n)) - 2.0
            loss64, g64, in64 = run(torch.float64, mel)
            loss32, g32, in32 = run(torch.float32, mel)
            assert in64.shape == in32.shape
            # inputs past an item's length do not exist here: every utterance runs at its own length
            min_abs, max_dev = float(in64.abs().min()), float((in32 - in64).abs().max())
            if min_abs > KINK_FACTOR * max_dev:
                break
        else:
            raise SystemExit(f"{name}: no mel seed in {MAX_SEEDS} meets the kink condition")
        assert min_abs > KINK_FACTOR * max_dev
        for b, nb in enumerate(lens):            # what lies past a length took part in nothing
            assert not g64["mel"][b, :, nb:].any()
        arrs = {"mel": mel.numpy(), "lens": np.array(lens), "target": target.numpy(),
                "loss64": np.array(loss64), "loss32": np.array(loss32), "mel_seed": np.array(MEL_SEED0 + n),
                "kink_min_abs": np.array(min_abs), "kink_max_dev": np.array(max_dev)}
        worst = 0.0
        for k in sorted(g64):
            assert np.abs(g64[k]).max() > 0, k
            dev = np.linalg.norm(g32[k] - g64[k]) / np.linalg.norm(g64[k])
            worst = max(worst, dev)
            arrs["grad/" + k] = g64[k].astype(np.float32)
            arrs["f32_vs_f64/" + k] = np.array(dev)
        print(f"vocoder_gen_bwd_{name}: mel seed {MEL_SEED0 + n} (tried {n + 1}), min |leaky-relu input| {min_abs:.3e} "
              f"against max |x32 - x64| {max_dev:.3e}; loss {loss64:.9f} (float32 {loss32:.9f}); {len(g64)} gradients, "
              f"the reference's float32 against float64: worst relative L2 {worst:.3e}")
        save(f"vocoder_gen_bwd_{name}.npz", **arrs)
        size = os.path.getsize(os.path.join(HERE, f"vocoder_gen_bwd_{name}.npz"))
        assert size < 1 << 20, size


if __name__ == "__main__":
    main()
