#!/usr/bin/env python3
"""Generate tests/golden/mel_loss_*.npz by RUNNING THE REFERENCE's TacotronSTFT (audio_processing.py) under torch autograd
on the CPU, in float64 and in float32:

    python tests/golden/make_golden_mel_loss.py --ref <checkout of the reference>

The differentiable value is composed from the reference's own methods without the `.data` detach of mel_spectrogram:
stft_fn.transform -> torch.matmul(mel_basis, .) -> spectral_normalize, applied per item at x[b, :lens[b]], under
F.l1_loss over the valid frames n[b] = min(1 + lens[b] // hop, Ft, frames[b]).  Same stand-ins as make_golden_collate.py
(make_golden.install_stubs); librosa.filters.mel returns the filterbank of the case: `mel_22k` of mel_basis_hf.npz for the
shipped geometry, the repo's mel_filterbank(22050, 64, 12, 0, None) for the small ones.  Nothing of the reference's source
is written into this repo.

Cases:
    small      64 / 16 / 64, 12 mels, B = 3, S = 400, lens [400, 333, 33] (a multiple of the hop, one that is not, and
               h + 1 where a sample has both mirrors); target a mel with Ft = F - 1 and frames [25, 20, 2]
    small_win  64 / 16 / 48, 12 mels, B = 2, S = 400, lens None; target given as audio (grad/t stored too).  The reference's
               STFT refuses win_length < filter_length, so its module is built at 64 / 16 / 64 and its forward_basis buffer is
               replaced by the DFT basis times the centre-padded 48-sample window (scipy get_window and pad_center, as its
               constructor composes them); transform, matmul and spectral_normalize are the reference's.
    shipped    1024 / 256 / 1024, 80 mels, fmax 8000, B = 2, S = 8192, lens [8192, 5000]; target a mel

Signals: two sines plus a white-noise floor; target = mel(x + 0.05 N(0, 1)) (float64 run, stored as float32) or that audio.
x is zero past lens[b].

The kink condition.  log(max(melp, 1e-5)) has a kink at the clamp and |mel - target| one at 0.  The script searches seeds
from 0 for the first one where, in the float64 run over the frames that enter the loss, every element keeps
|melp - 1e-5| and |mel - target| above KINK_FACTOR = 100 times ITS OWN float32-against-float64 deviation (of melp, and of
mel - target), and stores seed, clamp_margin and kink_margin (the smallest such ratios).  No element is excluded from any
comparison.  If no seed in MAX_SEEDS qualifies the script stops: raise NOISE, do not add an exclusion.

Stored per case: geometry (n_fft, hop, win, n_mel), mel_basis, x, target, lens and frames (absent = None), loss64, loss32,
grad/x (and grad/t) in float64, f32_vs_f64/loss and f32_vs_f64/grad_x (grad_t): the reference's own float32 deviation,
relative, L2 for the gradients.  One thread and fixed time stamps: two runs write the same bytes.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

CLIP = 1e-5
KINK_FACTOR = 100.0
MAX_SEEDS = 5000
NOISE = 0.05
SR = 22050
CASES = (
    dict(name="small", geom=(64, 16, 64, 12), B=3, S=400, lens=[400, 333, 33], frames=[25, 20, 2], ft_cut=1, audio=False),
    dict(name="small_win", geom=(64, 16, 48, 12), B=2, S=400, lens=None, frames=None, ft_cut=0, audio=True),
    dict(name="shipped", geom=(1024, 256, 1024, 80), B=2, S=8192, lens=[8192, 5000], frames=None, ft_cut=0, audio=False),
)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project")
    args = ap.parse_args()
    from make_golden import install_stubs
    from make_golden_waveglow_fwd import save
    install_stubs()
    from rad_mmm_amd.audio_processing import mel_filterbank
    mel_22k = np.load(os.path.join(HERE, "mel_basis_hf.npz"))["mel_22k"]
    current = {}
    sys.modules["librosa.filters"].mel = lambda *a, **k: current["mel_basis"]
    sys.path[:0] = [args.ref]
    os.chdir("/tmp")
    import torch
    import torch.nn.functional as F
    torch.set_num_threads(1)
    import audio_processing as R
    from scipy.signal import get_window

    for case in CASES:
        name, (n_fft, hop, win, n_mel), B, S = case["name"], case["geom"], case["B"], case["S"]
        lens = case["lens"] if case["lens"] is not None else [S] * B
        current["mel_basis"] = mel_22k if n_fft == 1024 else mel_filterbank(SR, n_fft, n_mel, 0.0, None)
        assert current["mel_basis"].shape == (n_mel, n_fft // 2 + 1)
        stft32 = R.TacotronSTFT(n_fft, hop, n_fft, n_mel, SR, 0.0, 8000.0 if n_fft == 1024 else None)
        if win != n_fft:
            cutoff = n_fft // 2 + 1
            fb = np.fft.fft(np.eye(n_fft))
            fb = torch.FloatTensor(np.vstack([np.real(fb[:cutoff, :]), np.imag(fb[:cutoff, :])])[:, None, :])
            w = torch.from_numpy(sys.modules["librosa.util"].pad_center(get_window("hann", win, fftbins=True), n_fft)).float()
            stft32.stft_fn.forward_basis = (fb * w).float()
        import copy
        mods = {torch.float32: stft32, torch.float64: copy.deepcopy(stft32).double()}
        Fr = 1 + S // hop
        Ft = Fr - case["ft_cut"]
        n = [min(1 + lens[b] // hop, Ft, case["frames"][b] if case["frames"] else Ft) for b in range(B)]

        def mel_of(sig, b, dt):
            m = mods[dt]
            magn, _ = m.stft_fn.transform(sig[b:b + 1, :lens[b]])
            melp = torch.matmul(m.mel_basis, magn)
            return melp[0], m.spectral_normalize(melp)[0]               # [n_mel, frames of the item]

        def run(dt, x32, t32, need_grad=True):
            """-> loss, grad_x, grad_t, melp and mel - target over the frames that enter the loss"""
            x = x32.to(dt).clone().requires_grad_(need_grad)
            t = t32.to(dt).clone().requires_grad_(need_grad and case["audio"])
            pred, tgt, melps = [], [], []
            for b in range(B):
                melp, mel = mel_of(x, b, dt)
                pred.append(mel[:, :n[b]])
                melps.append(melp[:, :n[b]])
                if case["audio"]:
                    tp, tm = mel_of(t, b, dt)
                    tgt.append(tm[:, :n[b]])
                    melps.append(tp[:, :n[b]])
                else:
                    tgt.append(t[b, :, :n[b]])
            pred, tgt = torch.cat(pred, 1), torch.cat(tgt, 1)
            loss = F.l1_loss(pred, tgt)
            out = dict(loss=float(loss.detach()), melp=torch.cat(melps, 1).detach().double().numpy(),
                       diff=(pred - tgt).detach().double().numpy())
            if need_grad:
                loss.backward()
                out["grad_x"] = x.grad.double().numpy()
                if case["audio"]:
                    out["grad_t"] = t.grad.double().numpy()
            return out

        def signals(seed):
            rng = np.random.RandomState(seed)
            k = np.arange(S) / SR
            x = np.zeros((B, S))
            for b in range(B):
                for _ in range(2):
                    x[b] += rng.uniform(0.1, 0.3) * np.sin(2 * np.pi * rng.uniform(200, 4000) * k + rng.uniform(0, 2 * np.pi))
                x[b] += 0.02 * rng.randn(S)
            y = x + NOISE * rng.randn(B, S)
            for b in range(B):
                x[b, lens[b]:] = 0
                y[b, lens[b]:] = 0
            x32, y32 = torch.from_numpy(x.astype(np.float32)), torch.from_numpy(y.astype(np.float32))
            if case["audio"]:
                return x32, y32
            t = torch.zeros(B, n_mel, Ft, dtype=torch.float64)
            with torch.no_grad():
                for b in range(B):
                    m = mel_of(y32.double(), b, torch.float64)[1]
                    k = min(m.shape[1], Ft)
                    t[b, :, :k] = m[:, :k]
            return x32, t.float()

        tiny = np.finfo(np.float64).tiny
        for seed in range(MAX_SEEDS):
            x32, t32 = signals(seed)
            with torch.no_grad():
                a, b32 = run(torch.float64, x32, t32, False), run(torch.float32, x32, t32, False)
            clamp_margin = float((np.abs(a["melp"] - CLIP) / np.maximum(np.abs(b32["melp"] - a["melp"]), tiny)).min())
            kink_margin = float((np.abs(a["diff"]) / np.maximum(np.abs(b32["diff"] - a["diff"]), tiny)).min())
            if clamp_margin > KINK_FACTOR and kink_margin > KINK_FACTOR:
                break
        else:
            raise SystemExit(f"{name}: no seed in {MAX_SEEDS} meets the kink condition: raise NOISE")
        r64, r32 = run(torch.float64, x32, t32), run(torch.float32, x32, t32)
        arrs = {"geometry": np.array([n_fft, hop, win, n_mel]), "mel_basis": current["mel_basis"].astype(np.float32),
                "x": x32.numpy(), "target": t32.numpy(), "seed": np.array(seed), "clamp_margin": np.array(clamp_margin),
                "kink_margin": np.array(kink_margin), "melp_min": np.array(a["melp"].min()),
                "diff_min": np.array(np.abs(a["diff"]).min()), "n": np.array(n),
                "loss64": np.array(r64["loss"]), "loss32": np.array(r32["loss"]),
                "f32_vs_f64/loss": np.array(abs(r32["loss"] - r64["loss"]) / abs(r64["loss"]))}
        if case["lens"] is not None:
            arrs["lens"] = np.array(case["lens"])
        if case["frames"] is not None:
            arrs["frames"] = np.array(case["frames"])
        text = []
        for k in ("x", "t") if case["audio"] else ("x",):
            g64, g32 = r64["grad_" + k], r32["grad_" + k]
            assert np.isfinite(g64).all() and np.abs(g64).max() > 0
            dev = np.linalg.norm(g32 - g64) / np.linalg.norm(g64)
            arrs["grad/" + k] = g64
            arrs["f32_vs_f64/grad_" + k] = np.array(dev)
            text.append(f"grad_{k} {dev:.3e}")
        print(f"mel_loss_{name}: seed {seed}, clamp margin {clamp_margin:.1f}, kink margin {kink_margin:.1f} (x own float32 "
              f"deviation), smallest melp {a['melp'].min():.3e}, smallest |mel - target| {np.abs(a['diff']).min():.3e}; loss "
              f"{r64['loss']:.9f} (float32 {r32['loss']:.9f}, deviation {float(arrs['f32_vs_f64/loss']):.3e}); the reference's "
              f"float32 gradients against float64: {', '.join(text)}")
        save(f"mel_loss_{name}.npz", **arrs)
        assert os.path.getsize(os.path.join(HERE, f"mel_loss_{name}.npz")) < 1 << 20


if __name__ == "__main__":
    main()
