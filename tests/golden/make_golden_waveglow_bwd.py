#!/usr/bin/env python3
"""Generate tests/golden/waveglow_bwd_tiny.npz by RUNNING THE REFERENCE's training step
(vocoders/waveglow_for_LIMMITS23/train.py:128-139: WaveGlowLoss(sigma)(model((mel, audio))).backward(), glow.py:43-59,
207-249) on the CPU:

    python tests/golden/make_golden_waveglow_bwd.py --ref <checkout of the reference>

It reads config, sd/*, mel, audio and eq_T from waveglow_fwd_tiny.npz (make_golden_waveglow_fwd.py) and stores none of
them again.  The reference's WaveGlow is built with that config, weight norm left on (the state of a training run),
loaded with sd/*, and run on the equal-length batch (the first eq_T frames of both items) with sigma = 1: once in
float64 and once in float32.

The fixture holds, per stored parameter <name> (the reference's names, weight_g / weight_v where it weight-norms):
    grad/<name>        the float64 gradient, stored as float32
    f32_vs_f64/<name>  ||grad32 - grad64|| / ||grad64||: the reference's own float32 deviation
and loss64 / loss32.  Stored: every parameter of flows 0 (8 channels), 2 (the first flow after an early exit, 6
channels, n_half 3) and 5 (the last, 4 channels); convinv, start and end of every flow; upsample.weight and
upsample.bias.  The generator asserts that no stored gradient is identically zero and that the file stays below 1 MiB.

One thread and a zip archive with fixed time stamps: two runs write the same bytes.
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
HOP = 256
FULL_FLOWS = (0, 2, 5)


def stored(name):
    if name.startswith("upsample.") or name.startswith("convinv."):
        return True
    k = int(name.split(".")[1])
    return k in FULL_FLOWS or name.split(".")[2] in ("start", "end")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project")
    args = ap.parse_args()
    from make_golden import install_stubs
    from make_golden_waveglow_fwd import save
    install_stubs()
    wg_dir = os.path.join(args.ref, "vocoders", "waveglow_for_LIMMITS23")
    sys.path[:0] = [wg_dir, os.path.join(wg_dir, "tacotron2")]
    os.chdir("/tmp")
    import torch
    torch.set_num_threads(1)
    from glow import WaveGlow, WaveGlowLoss

    d = np.load(os.path.join(HERE, "waveglow_fwd_tiny.npz"))
    cfg = json.loads(str(d["config"]))
    sd = {k[3:]: torch.from_numpy(d[k].astype(np.float32)) for k in d.files if k.startswith("sd/")}
    n = int(d["eq_T"])
    mel, audio = torch.from_numpy(d["mel"][:, :, :n].copy()), torch.from_numpy(d["audio"][:, :n * HOP].copy())

    torch.manual_seed(0)
    m32, m64 = WaveGlow(**cfg), WaveGlow(**cfg).double()
    m32.load_state_dict(sd)
    m64.load_state_dict({k: v.double() for k, v in sd.items()})
    crit = WaveGlowLoss(sigma=1.0)
    grads, losses = [], []
    for m, dt in ((m64, torch.float64), (m32, torch.float32)):
        m.train()
        loss = crit(m((mel.to(dt), audio.to(dt))))
        loss.backward()
        losses.append(loss.item())
        grads.append({k: p.grad.double().numpy() for k, p in m.named_parameters()})
    assert set(grads[0]) == set(sd)
    arrs = {"loss64": np.array(losses[0]), "loss32": np.array(losses[1])}
    worst = 0.0
    for k in sorted(grads[0]):
        if not stored(k):
            continue
        g64, g32 = grads[0][k], grads[1][k]
        assert np.abs(g64).max() > 0, k
        dev = np.linalg.norm(g32 - g64) / np.linalg.norm(g64)
        worst = max(worst, dev)
        arrs["grad/" + k] = g64.astype(np.float32)
        arrs["f32_vs_f64/" + k] = np.array(dev)
    print(f"waveglow_bwd_tiny: loss {losses[0]:.9f} (float32 {losses[1]:.9f}), {len(arrs) // 2 - 1} gradients, the "
          f"reference's float32 against float64: worst relative L2 {worst:.3e}")
    save("waveglow_bwd_tiny.npz", **arrs)
    size = os.path.getsize(os.path.join(HERE, "waveglow_bwd_tiny.npz"))
    assert size < 1 << 20, size


if __name__ == "__main__":
    main()
