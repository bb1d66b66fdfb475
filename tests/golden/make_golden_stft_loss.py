#!/usr/bin/env python3
"""Generate tests/golden/stft_loss_*.npz by RUNNING THE REFERENCE's MultiResolutionSTFTLoss (stft_loss.py:261-314) and
torch autograd on the CPU, in float64 and in float32:

    python tests/golden/make_golden_stft_loss.py --ref <checkout of the reference>

Shape: resolutions fft (64, 128, 32), hop (12, 24, 5), win (40, 100, 16); T = 600; x ~ N(0, 1), y = x + 0.5 N(0, 1), both
zero past each item's length.  Four cases: lengths [600, 333, 40] with len_ratios = lengths / 600 ("ragged") and lengths
[600, 333] with lens=None ("global"), each with a_weighting False ("log") and True ("log1p").

The kink condition.  |log y - log x| has a kink wherever two magnitudes agree and the clamp one at a bin power of 1e-7:
a bin on the other side in float32 moves the gradients by up to 2.5e-4.  The script searches seeds from 0 for the first
one where, over the valid frames of every resolution in the float64 run,
  * every non-zero bin power p keeps |log(p / 1e-7)| > CLAMP_MARGIN, and
  * no |dlog| on a live bin (not both magnitudes clamped) is smaller than KINK_FACTOR times the largest |dlog32 - dlog64|
    of the reference's own float32 run on the live bins,
asserts both and stores the numbers (clamp_margin, dlog_min, dlog_dev) with the seed.  It also asserts that no
len_ratios[b] * F lies within 1e-3 of an integer unless the item has the full length.

Stored per case: x, y, len_ratios (float32; absent for the global cases), lengths, sc64, mag64, sc32, mag32, the float64
gradients grad/{sc,mag}_{x,y} of each loss with respect to each argument, and f32_vs_f64/{...}: the reference's own
float32 relative-L2 deviation of each; `state_dict_keys` holds the names of the reference module's state_dict.

One thread and a zip archive with fixed time stamps: two runs write the same bytes.
"""
import argparse
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
FFT, HOP, WIN = (64, 128, 32), (12, 24, 5), (40, 100, 16)
T = 600
CLAMP = 1e-7
CLAMP_MARGIN = 1e-3
KINK_FACTOR = 8.0
MAX_SEEDS = 5000
NOISE = 0.5
CASES = (("ragged_log", [600, 333, 40], True, False), ("ragged_log1p", [600, 333, 40], True, True),
         ("global_log", [600, 333], False, False), ("global_log1p", [600, 333], False, True))


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
    sys.path[:0] = [args.ref]
    os.chdir("/tmp")
    import torch
    torch.set_num_threads(1)
    import warnings
    warnings.filterwarnings("ignore")
    import stft_loss as R

    def raw_power(sig, mod):
        z = torch.stft(sig, mod.fft_size, mod.shift_size, mod.win_length, mod.window.to(sig.dtype), return_complex=True)
        return (z.real ** 2 + z.imag ** 2).transpose(2, 1)                     # [B, F, bins]

    for name, lengths, ragged, a_w in CASES:
        B = len(lengths)
        ratios = torch.tensor(lengths, dtype=torch.float32) / T if ragged else None
        mods = {dt: R.MultiResolutionSTFTLoss(list(FFT), list(HOP), list(WIN), a_weighting=a_w).to(dt)
                for dt in (torch.float64, torch.float32)}
        if ragged:
            for hop in HOP:
                v = (ratios * (1 + T // hop)).double()
                for b in range(B):
                    assert lengths[b] == T or abs(float(v[b]) - round(float(v[b]))) > 1e-3, (hop, b, float(v[b]))

        def run(dt, x32, y32):
            out = {}
            for which in ("sc", "mag"):
                x, y = x32.to(dt).clone().requires_grad_(True), y32.to(dt).clone().requires_grad_(True)
                sc, mag = mods[dt](x, y, ratios)
                (sc if which == "sc" else mag).backward()
                out[which] = float(sc if which == "sc" else mag)
                out[which + "_x"], out[which + "_y"] = x.grad.double().numpy(), y.grad.double().numpy()
            return out

        def margins(x32, y32):
            clamp_margin, dl_min, dl_dev = np.inf, np.inf, 0.0
            for m64, m32 in zip(mods[torch.float64].stft_losses, mods[torch.float32].stft_losses):
                F = 1 + T // m64.shift_size
                nf = (ratios * F).ceil().long() if ragged else torch.full((B,), F)
                valid = torch.arange(F)[None, :] < nf[:, None]
                dls, live = [], None
                for dt, m in ((torch.float64, m64), (torch.float32, m32)):
                    px, py = raw_power(x32.to(dt), m)[valid], raw_power(y32.to(dt), m)[valid]
                    xm, ym = R.stft(x32.to(dt), m.fft_size, m.shift_size, m.win_length, m.window)[valid], \
                        R.stft(y32.to(dt), m.fft_size, m.shift_size, m.win_length, m.window)[valid]
                    dls.append((torch.log(ym + 1) - torch.log(xm + 1) if a_w else torch.log(ym) - torch.log(xm)).double())
                    if dt is torch.float64:
                        live = ~((px < CLAMP) & (py < CLAMP))
                        for p in (px, py):
                            nz = p[p > 0]
                            clamp_margin = min(clamp_margin, float((nz / CLAMP).log().abs().min()))
                dl_min = min(dl_min, float(dls[0][live].abs().min()))
                dl_dev = max(dl_dev, float((dls[1] - dls[0])[live].abs().max()))
            return clamp_margin, dl_min, dl_dev

        for seed in range(MAX_SEEDS):
            g = torch.Generator().manual_seed(seed)
            x = torch.randn(B, T, generator=g)
            y = x + NOISE * torch.randn(B, T, generator=g)
            for b, n in enumerate(lengths):
                x[b, n:] = 0
                y[b, n:] = 0
            clamp_margin, dl_min, dl_dev = margins(x, y)
            if clamp_margin > CLAMP_MARGIN and dl_min > KINK_FACTOR * dl_dev:
                break
        else:
            raise SystemExit(f"{name}: no seed in {MAX_SEEDS} meets the kink condition")
        assert clamp_margin > CLAMP_MARGIN and dl_min > KINK_FACTOR * dl_dev
        r64, r32 = run(torch.float64, x, y), run(torch.float32, x, y)
        arrs = {"x": x.numpy(), "y": y.numpy(), "lengths": np.array(lengths), "seed": np.array(seed),
                "clamp_margin": np.array(clamp_margin), "dlog_min": np.array(dl_min), "dlog_dev": np.array(dl_dev),
                "sc64": np.array(r64["sc"]), "mag64": np.array(r64["mag"]), "sc32": np.array(r32["sc"]),
                "mag32": np.array(r32["mag"]),
                "state_dict_keys": np.array(sorted(mods[torch.float32].state_dict().keys()))}
        if ragged:
            arrs["len_ratios"] = ratios.numpy()
        worst = 0.0
        for k in ("sc_x", "sc_y", "mag_x", "mag_y"):
            assert np.abs(r64[k]).max() > 0, k
            dev = np.linalg.norm(r32[k] - r64[k]) / np.linalg.norm(r64[k])
            worst = max(worst, dev)
            arrs["grad/" + k] = r64[k]
            arrs["f32_vs_f64/" + k] = np.array(dev)
        print(f"stft_loss_{name}: seed {seed}, clamp margin {clamp_margin:.3e}, min |dlog| {dl_min:.3e} against float32 "
              f"deviation {dl_dev:.3e}; sc {r64['sc']:.9f} (float32 {r32['sc']:.9f}), mag {r64['mag']:.9f} (float32 "
              f"{r32['mag']:.9f}); the reference's float32 gradients against float64: worst relative L2 {worst:.3e}")
        save(f"stft_loss_{name}.npz", **arrs)
        assert os.path.getsize(os.path.join(HERE, f"stft_loss_{name}.npz")) < 1 << 20


if __name__ == "__main__":
    main()
