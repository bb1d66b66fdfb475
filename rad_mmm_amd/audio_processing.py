"""STFT -> mel -> log front end on the GPU (reference audio_processing.py:119-154, 192-255).

`TacotronSTFT(filter_length, hop_length, win_length, n_mel_channels, sampling_rate, mel_fmin,
mel_fmax).mel_spectrogram(y)` as in the reference, forward only (the reference runs it without
grad inside DataLoader workers).  The windowed DFT basis is built exactly like the reference's
conv1d weights; the mel filterbank restates librosa 0.8.0 `filters.mel` (Slaney scale, Slaney
norm), which the reference imports -- pinned to an independent librosa-validated implementation
(tests/golden/mel_basis_hf.npz: librosa itself is absent from the reference tree and the image).
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from . import ops
from ._lib import fp32_region, lib, check, ptr, stream


def _hann_periodic(n: int) -> np.ndarray:
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def windowed_dft_basis(n_fft: int, win_length: int) -> np.ndarray:
    """[2*(n_fft/2+1), n_fft] fp32: rows re then im of the DFT, times the centre-padded periodic
    hann window (audio_processing.py:200-223)."""
    cutoff = n_fft // 2 + 1
    fb = np.fft.fft(np.eye(n_fft))
    basis = np.vstack([np.real(fb[:cutoff]), np.imag(fb[:cutoff])]).astype(np.float32)
    w = _hann_periodic(win_length)
    lp = (n_fft - win_length) // 2
    w = np.pad(w, (lp, n_fft - win_length - lp)).astype(np.float32)
    return basis * w[None, :]


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    f_sp = 200.0 / 3
    min_log_hz, logstep = 1000.0, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_hz / f_sp + np.log(np.maximum(f, 1e-10) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp = 200.0 / 3
    min_log_hz, logstep = 1000.0, np.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filterbank(sr, n_fft, n_mels, fmin, fmax) -> np.ndarray:
    """Slaney-scale, Slaney-normalised triangular filterbank [n_mels, n_fft/2+1]."""
    if fmax is None:
        fmax = sr / 2.0
    fftfreqs = np.linspace(0, sr / 2.0, 1 + n_fft // 2)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    wts = np.zeros((n_mels, 1 + n_fft // 2))
    for i in range(n_mels):
        wts[i] = np.maximum(0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    enorm = 2.0 / (mel_f[2: n_mels + 2] - mel_f[:n_mels])
    return (wts * enorm[:, None]).astype(np.float32)


class STFT(nn.Module):
    """Magnitude STFT (reference STFT.transform; inverse/griffin-lim are out of scope)."""

    def __init__(self, filter_length=800, hop_length=200, win_length=800, window="hann"):
        super().__init__()
        assert window == "hann" and win_length <= filter_length
        self.filter_length, self.hop_length, self.win_length = filter_length, hop_length, win_length
        self.register_buffer("forward_basis", torch.from_numpy(windowed_dft_basis(filter_length, win_length)))


class TacotronSTFT(nn.Module):
    def __init__(self, filter_length=1024, hop_length=256, win_length=1024, n_mel_channels=80,
                 sampling_rate=22050, mel_fmin=0.0, mel_fmax=None):
        super().__init__()
        self.n_mel_channels = n_mel_channels
        self.sampling_rate = sampling_rate
        self.stft_fn = STFT(filter_length, hop_length, win_length)
        self.register_buffer("mel_basis", torch.from_numpy(
            mel_filterbank(sampling_rate, filter_length, n_mel_channels, mel_fmin, mel_fmax)))

    @fp32_region
    def mel_spectrogram(self, y: torch.Tensor) -> torch.Tensor:
        """y [B, S] in [-1, 1] -> [B, n_mel, 1 + S//hop] log-mel (clamp 1e-5)."""
        if not y.is_cuda:
            raise RuntimeError("rad_mmm_amd.audio_processing runs on an MI355X only (no CPU path)")
        assert float(y.min()) >= -1 and float(y.max()) <= 1
        s = self.stft_fn
        return ops.stft_mel(y.float(), s.forward_basis, self.mel_basis, s.filter_length, s.hop_length, 1e-5)

    @fp32_region
    def mel_spectrogram_ragged(self, y: torch.Tensor, lens, out: torch.Tensor = None, *, lens_device: torch.Tensor = None,
                               frames_device: torch.Tensor = None, offsets: torch.Tensor = None, scale: float = 1.0,
                               energy: torch.Tensor = None, scaled_energy: bool = True, audio_out: torch.Tensor = None,
                               scratch: torch.Tensor = None) -> torch.Tensor:
        """Log-mel of utterances of different lengths in one call: [B, n_mel, Tmax], Tmax = 1 + max(lens) // hop, row b
        holding the 1 + lens[b] // hop frames `mel_spectrogram` gives for that utterance alone (each reflect-padded at its
        own two ends) and exact zeros after them.  No range assert and no synchronisation.

        y: [B, Smax] float in [-1, 1] on the device; or, with `offsets` (int64 device tensor [B], first sample of each item),
        a packed 1-D int16 / float32 buffer, multiplied by `scale`.  lens: HOST sample counts (sequence or CPU tensor), each
        > filter_length // 2; lens_device / frames_device: the same counts and 1 + lens // hop as int32 device tensors when the
        caller has them (else they are uploaded through pinned memory).  energy [B, Tmax], audio_out [B, 1, Smax]: filled
        in the same pass when given (data.get_energy_average of the rows; the scaled, zero-padded samples).  scratch: fp32
        device buffer of radmmm_collate_scratch_floats elements to reuse."""
        if not y.is_cuda:
            raise RuntimeError("rad_mmm_amd.audio_processing runs on an MI355X only (no CPU path)")
        s = self.stft_fn
        n_fft, hop, n_mel = s.filter_length, s.hop_length, self.n_mel_channels
        lens_host = torch.as_tensor(lens, dtype=torch.int64, device="cpu")
        B = int(lens_host.numel())
        Smax = int(lens_host.max())
        if int(lens_host.min()) <= n_fft // 2:
            raise ValueError(f"mel_spectrogram_ragged: every utterance needs more than filter_length // 2 = {n_fft // 2} samples")
        if offsets is None:
            if y.dim() != 2 or y.shape[0] != B or y.shape[1] < Smax:
                raise ValueError("mel_spectrogram_ragged: y must be [B, S] with S >= max(lens) (or packed, with offsets)")
            y = y.float().contiguous()
            offsets = torch.arange(B, device=y.device, dtype=torch.int64) * y.shape[1]
        elif y.dim() != 1 or y.dtype not in (torch.int16, torch.float32) or not y.is_contiguous():
            raise ValueError("mel_spectrogram_ragged: a packed buffer is 1-D contiguous int16 or float32")
        if lens_device is None:
            lens_device = lens_host.to(torch.int32).pin_memory().to(y.device, non_blocking=True)
        if frames_device is None:
            frames_device = torch.div(lens_device, hop, rounding_mode="floor").to(torch.int32) + 1
        Tmax = 1 + Smax // hop
        if out is None:
            out = torch.empty(B, n_mel, Tmax, device=y.device, dtype=torch.float32)
        elif tuple(out.shape) != (B, n_mel, Tmax) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f"mel_spectrogram_ragged: out must be contiguous fp32 [{B}, {n_mel}, {Tmax}]")
        for name, t, shape in (("energy", energy, (B, Tmax)), ("audio_out", audio_out, (B, 1, Smax))):
            if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous()):
                raise ValueError(f"mel_spectrogram_ragged: {name} must be contiguous fp32 {list(shape)}")
        need = int(lib.radmmm_collate_scratch_floats(B, Smax, n_fft, hop, n_mel))
        if scratch is None or scratch.numel() < need:
            scratch = torch.empty(need, device=y.device, dtype=torch.float32)
        check(lib.radmmm_collate_unpack_pad(ptr(y), 1 if y.dtype == torch.int16 else 0, ptr(offsets), ptr(lens_device),
                                            ptr(scratch), ptr(audio_out), B, Smax, n_fft, float(scale), stream()),
              "collate_unpack_pad")
        check(lib.radmmm_collate_mel(ptr(s.forward_basis), ptr(self.mel_basis), ptr(frames_device), ptr(out), ptr(energy),
                                     ptr(scratch), B, Smax, n_fft, hop, n_mel, 1e-5, 1 if scaled_energy else 0, stream()),
              "collate_mel")
        return out
