#!/usr/bin/env python3
"""Generate tests/golden/msd_t97.npz / msd_t64.npz by RUNNING THE REFERENCE's MultiScaleDiscriminator.forward
(vocoders/hifigan_models.py:313-371), its three GAN losses (loss.py:29-83) and torch autograd on the CPU, in float64 and in
float32:

    python tests/golden/make_golden_msd.py --ref <checkout of the reference>

Narrowing.  The reference hard-codes the widths 128 .. 1024 (no fixture of that size).  The script builds the reference's
class and replaces each DiscriminatorS's convs / conv_post with layers of widths (8, 8, 16, 16, 32, 32, 16) -> 1 in groups
(1, 2, 2, 4, 4, 4, 1) with the same kernels, strides and pads: 4 or 8 channels per group on either side of every grouped
conv, the narrowest the grouped kernels take.  spectral_norm wraps member 0's layers, weight_norm the others'; the
reference's forward code (pools, loop, flatten) is what runs.  Weights: the default init under torch.manual_seed(0), every
weight_g times 3, biases U(-0.3, 0.3).  `default_keys` / `default_shapes` hold the state_dict of the reference's UNMODIFIED
class.  The models run in training mode, so member 0 advances weight_u / weight_v twice per forward; the state dict is
reloaded before each run and `sd_after/<name>` holds those buffers after the float64 run.

Two fixtures: B = 2, T = 97, len_ratios [1.0, 0.7] (every pool sees an odd length) and B = 3, T = 64, len_ratios
[1.0, 0.7, 0.5] (the last maps of every member have one frame); y, y_hat ~ U(-1, 1).  The loss is L = 2 * fm + gen + disc in
one backward (the 2 only keeps the terms distinguishable).

The kink condition is make_golden_mpd.py's: the script searches input seeds from 0 for the first one where, in the float64
run, the smallest |leaky-relu input| exceeds KINK_FACTOR times the largest |x32 - x64| of the reference's own float32 run,
and likewise the smallest |r - g| over every element of every feature map; it asserts both and stores the numbers.

Stored per fixture: y, y_hat, len_ratios, sd/<name> (float32), sd_after/<name> (float64), fm / gen / disc / r_losses /
g_losses as <name>64 and <name>32, out_r/<i>, out_g/<i> (float64 stored as float32), grad/<name> for every parameter and
y_hat (float64 stored as float32), f32_vs_f64/<name>: the reference's own float32 relative-L2 deviation.  No gradient is
identically zero and each file stays below 1 MiB (both asserted).
"""
import argparse
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
KINK_FACTOR = 8.0
MAX_SEEDS = 400
WIDTHS = (8, 8, 16, 16, 32, 32, 16)
GROUPS = (1, 2, 2, 4, 4, 4, 1)
KERNELS = (15, 41, 41, 41, 41, 41, 5)
STRIDES = (1, 2, 2, 4, 4, 1, 1)
GAIN = 3.0
CASES = (("t97", 97, [1.0, 0.7]), ("t64", 64, [1.0, 0.7, 0.5]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project")
    args = ap.parse_args()
    from make_golden import install_stubs
    from make_golden_waveglow_fwd import save
    install_stubs()
    try:
        import distutils.version  # noqa: F401
    except ImportError:                                   # removed from newer Pythons; the reference compares versions with it
        from packaging.version import Version
        dv = types.ModuleType("distutils.version")
        dv.LooseVersion = lambda s: Version(str(s).split("+")[0])
        sys.modules["distutils"] = types.ModuleType("distutils")
        sys.modules["distutils.version"] = dv
    sys.path[:0] = [args.ref, os.path.join(args.ref, "vocoders")]
    os.chdir("/tmp")
    import torch
    import torch.nn.functional as F
    torch.set_num_threads(1)
    import warnings
    warnings.filterwarnings("ignore")
    from torch.nn import Conv1d
    from torch.nn.utils import spectral_norm, weight_norm
    import hifigan_models as HM
    import loss as RL

    torch.manual_seed(0)
    full = HM.MultiScaleDiscriminator()
    default_keys = list(full.state_dict().keys())
    default_shapes = [list(v.shape) for v in full.state_dict().values()]
    del full

    def narrowed():
        torch.manual_seed(0)
        base = HM.MultiScaleDiscriminator()
        bias_gen = torch.Generator().manual_seed(1)
        for i, d in enumerate(base.discriminators):
            norm_f = spectral_norm if i == 0 else weight_norm
            cin, convs = 1, []
            for c, g, k, st in zip(WIDTHS, GROUPS, KERNELS, STRIDES):
                convs.append(norm_f(Conv1d(cin, c, k, st, groups=g, padding=k // 2)))
                cin = c
            d.convs = torch.nn.ModuleList(convs)
            d.conv_post = norm_f(Conv1d(cin, 1, 3, 1, padding=1))
            with torch.no_grad():
                for m in list(d.convs) + [d.conv_post]:
                    if hasattr(m, "weight_g"):
                        m.weight_g.mul_(GAIN)
                    m.bias.copy_((torch.rand(m.bias.shape, generator=bias_gen) * 2 - 1) * 0.3)
        return base

    sd = {k: v.detach().clone() for k, v in narrowed().state_dict().items()}
    models = {dt: narrowed().to(dt).train() for dt in (torch.float64, torch.float32)}

    seen = []
    stock_lrelu = F.leaky_relu

    def recording_lrelu(x, *a, **k):
        seen.append(x.detach().double().reshape(-1))
        return stock_lrelu(x, *a, **k)

    def run(dt, y, y_hat, ratios):
        m = models[dt]
        m.load_state_dict(sd)                   # a training-mode run moves weight_u / weight_v
        m.zero_grad()
        yy = y.to(dt)
        yh = y_hat.to(dt).clone().requires_grad_(True)
        del seen[:]
        F.leaky_relu = recording_lrelu
        try:
            rs, gs, frs, fgs = m(yy, yh)
        finally:
            F.leaky_relu = stock_lrelu
        fm = RL.gan_feature_loss(frs, fgs, ratios)
        gen, _ = RL.gan_generator_loss(gs, ratios)
        disc, r_l, g_l = RL.gan_discriminator_loss(rs, gs, ratios)
        (2 * fm + gen + disc).backward()
        g = {k: p.grad.double().numpy() for k, p in m.named_parameters()}
        g["y_hat"] = yh.grad.double().numpy()
        diffs = torch.cat([(r - g_).detach().double().reshape(-1) for fr, fg in zip(frs, fgs) for r, g_ in zip(fr, fg)])
        after = {k: v.detach().double().numpy().copy() for k, v in m.state_dict().items() if k.endswith(("weight_u", "weight_v"))
                 and k.startswith("discriminators.0.")}
        return {"fm": float(fm), "gen": float(gen), "disc": float(disc), "r_losses": np.array(r_l, dtype=np.float64),
                "g_losses": np.array(g_l, dtype=np.float64), "grad": g, "inputs": torch.cat(seen), "diffs": diffs, "after": after,
                "out_r": [r.detach().double().numpy() for r in rs], "out_g": [x.detach().double().numpy() for x in gs]}

    for name, T, rat in CASES:
        B = len(rat)
        ratios = torch.tensor(rat, dtype=torch.float32)
        best = 0.0
        for seed in range(MAX_SEEDS):
            gen = torch.Generator().manual_seed(seed)
            y = torch.rand(B, 1, T, generator=gen) * 2 - 1
            y_hat = torch.rand(B, 1, T, generator=gen) * 2 - 1
            r64, r32 = run(torch.float64, y, y_hat, ratios), run(torch.float32, y, y_hat, ratios)
            kmin, kdev = float(r64["inputs"].abs().min()), float((r32["inputs"] - r64["inputs"]).abs().max())
            dmin, ddev = float(r64["diffs"].abs().min()), float((r32["diffs"] - r64["diffs"]).abs().max())
            best = max(best, min(kmin / kdev, dmin / ddev))
            if kmin > KINK_FACTOR * kdev and dmin > KINK_FACTOR * ddev:
                break
        else:
            raise SystemExit(f"{name}: no seed in {MAX_SEEDS} meets the kink condition (best ratio {best:.2f})")
        assert kmin > KINK_FACTOR * kdev and dmin > KINK_FACTOR * ddev
        arrs = {"y": y.numpy(), "y_hat": y_hat.numpy(), "len_ratios": ratios.numpy(), "seed": np.array(seed),
                "kink_min_abs": np.array(kmin), "kink_max_dev": np.array(kdev), "diff_min_abs": np.array(dmin),
                "diff_max_dev": np.array(ddev), "widths": np.array(WIDTHS), "groups": np.array(GROUPS),
                "default_keys": np.array(default_keys),
                "default_shapes": np.array([",".join(map(str, s)) for s in default_shapes])}
        for k, v in sd.items():
            arrs["sd/" + k] = v.numpy().astype(np.float32)
        for k, v in r64["after"].items():
            arrs["sd_after/" + k] = v
        assert len(r64["after"]) == 16
        for k in ("fm", "gen", "disc", "r_losses", "g_losses"):
            arrs[k + "64"], arrs[k + "32"] = np.array(r64[k], dtype=np.float64), np.array(r32[k], dtype=np.float64)
        for i in range(len(r64["out_r"])):
            arrs[f"out_r/{i}"] = r64["out_r"][i].astype(np.float32)
            arrs[f"out_g/{i}"] = r64["out_g"][i].astype(np.float32)
        worst = 0.0
        for k in sorted(r64["grad"]):
            g64, g32 = r64["grad"][k], r32["grad"][k]
            assert np.abs(g64).max() > 0, k
            dev = np.linalg.norm(g32 - g64) / np.linalg.norm(g64)
            worst = max(worst, dev)
            arrs["grad/" + k] = g64.astype(np.float32)
            arrs["f32_vs_f64/" + k] = np.array(dev)
        print(f"msd_{name}: seed {seed}, {r64['inputs'].numel()} leaky-relu inputs, min |x| {kmin:.3e} against max |x32 - x64| "
              f"{kdev:.3e}; min |r - g| {dmin:.3e} against {ddev:.3e}; fm {r64['fm']:.9f} gen {r64['gen']:.9f} disc "
              f"{r64['disc']:.9f}; the reference's float32 against float64: worst relative L2 {worst:.3e}, y_hat "
              f"{float(arrs['f32_vs_f64/y_hat']):.3e}")
        save(f"msd_{name}.npz", **arrs)
        size = os.path.getsize(os.path.join(HERE, f"msd_{name}.npz"))
        assert size < 1 << 20, size


if __name__ == "__main__":
    main()
