"""One HiFi-GAN fine-tuning step as an object: the generator, both discriminators, the mel L1 and the
optional multi-resolution STFT loss, and two fused AdamW optimizers (optim.FlatAdam, decoupled), in upstream HiFi-GAN's
order -- one generator forward, the D step on the detached audio, the G side on the stepped discriminators.  Every term is
a HIP kernel path of this package; with host lengths a step never waits for the device.  Checkpoints are upstream's file
pair (`g_XXXXXXXX` / `do_XXXXXXXX`), which load_hifigan_vocoder, load_mpd and load_msd read back."""
from __future__ import annotations

import os
from typing import Dict, Optional

import torch

from .discriminators import _check_precision
from .mel_loss import MelSpectrogramLoss
from .optim import FlatAdam
from .vocoder import HiFiGANGenerator, _lens_arg


class HiFiGANTrainingStep:
    """HiFiGANTrainingStep(generator, mpd, msd, stft_loss=None, mel_loss=None, lr, betas, weight_decay, lr_decay,
    mel_weight, clip): the modules are on the GPU; they are put in training mode and their parameters become views of the
    optimizers' flat buffers.  Defaults are upstream's `torch.optim.AdamW(params, 2e-4, betas=(0.8, 0.99))` (weight decay
    0.01, torch's) and `ExponentialLR(gamma=0.999)` per epoch.  mel_loss: None builds MelSpectrogramLoss() (the default
    TacotronSTFT) on the generator's device; its hop must be the generator's.  stft_loss: None leaves the two spectral terms
    out of the generator's loss.  clip: each optimizer clips its own global gradient norm to it (a total that is not finite
    skips that optimizer's step on the device).  mpd_precision: None leaves the multi-period discriminator's mode as the
    model has it ("fp32" unless it was set, e.g. by load_mpd(path, precision="h3")); "fp32" or "h3" sets it
    (MultiPeriodDiscriminator.precision; a checkpoint does not store it).  In "h3" the discriminator's saturation word is the
    `skip` of BOTH optimizers -- the audio gradient of the G side flows through the same fp16 pairs -- so a step in which a
    pair clamped changes no parameter, moment or step count, without a device -> host read; the word stays raised until the
    caller reads it with mpd.grad_saturated() (and lowers mpd.grad_scale)."""

    def __init__(self, generator: HiFiGANGenerator, mpd, msd, stft_loss=None, mel_loss=None, lr: float = 2e-4,
                 betas=(0.8, 0.99), weight_decay: float = 0.01, lr_decay: float = 0.999, mel_weight: float = 45.0,
                 clip: Optional[float] = None, mpd_precision: Optional[str] = None):
        if mpd_precision is not None:
            _check_precision(mpd_precision)
        dev = next(generator.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("HiFiGANTrainingStep: move the modules to the GPU first (there is no CPU path)")
        if mpd_precision is not None:
            mpd.precision = mpd_precision
        self.generator, self.mpd, self.msd = generator.train(), mpd.train(), msd.train()
        self.stft_loss = stft_loss
        self.mel_loss = mel_loss if mel_loss is not None else MelSpectrogramLoss().to(dev)
        hop = int(self.mel_loss.stft.stft_fn.hop_length)
        if hop != generator.hop:
            raise ValueError(f"HiFiGANTrainingStep: the mel loss has hop {hop}, the generator {generator.hop}")
        self.mel_weight, self.lr_decay, self.clip = float(mel_weight), float(lr_decay), clip
        kw = dict(lr=lr, betas=betas, weight_decay=weight_decay, decoupled=True)
        self.optim_g = FlatAdam(generator.named_parameters(), **kw)
        self._d_params = [p for m in (mpd, msd) for p in m.parameters() if p.requires_grad]
        self.optim_d = FlatAdam([(f"mpd.{n}", p) for n, p in mpd.named_parameters()]
                                + [(f"msd.{n}", p) for n, p in msd.named_parameters()], **kw)
        self.steps = 0
        self.epoch = 0

    def _optim_step(self, opt: FlatAdam) -> None:
        if self.clip is not None:
            opt.clip_grad_norm(self.clip)
        if getattr(self.mpd, "precision", "fp32") == "h3":      # a clamped fp16 pair of the discriminator makes the step a no-op, on the device
            opt.step(skip=self.mpd.saturation_flag())
        else:
            opt.step()

    def training_step(self, mel: torch.Tensor, lens, audio: torch.Tensor) -> Dict[str, torch.Tensor]:
        """mel [B, 80, T], lens in frames (host: no synchronisation; or device), audio [B, 1, T * hop] -> the terms of both
        steps and both totals as 0-d device tensors."""
        gen, mpd, msd = self.generator, self.mpd, self.msd
        hop = gen.hop
        lens_d, _ = _lens_arg(lens, mel.shape[0], mel.shape[2], mel.device)
        audio_hat = gen(mel, lens)
        ratios = lens_d / lens_d.max()                                    # on the device
        # D step
        self.optim_d.zero_grad()
        d_p, _, _ = mpd.discriminator_loss(audio, audio_hat.detach(), ratios)
        d_s, _, _ = msd.discriminator_loss(audio, audio_hat.detach(), ratios)
        d_total = d_p + d_s
        d_total.backward()
        self._optim_step(self.optim_d)
        # G side, on the stepped discriminators; their parameters are frozen so that only the audio gradient is computed
        self.optim_g.zero_grad()
        for p in self._d_params:
            p.requires_grad_(False)
        try:
            fm_p, gen_p = mpd.generator_losses(audio, audio_hat, ratios)
            fm_s, gen_s = msd.generator_losses(audio, audio_hat, ratios)
            if self.stft_loss is not None:
                sc, mag = self.stft_loss(audio_hat[:, 0], audio[:, 0], ratios)
            l_mel = self.mel_loss(audio_hat[:, 0], mel, lens_d * hop, lens_d)
            g_total = self.mel_weight * l_mel + fm_p + fm_s + gen_p + gen_s
            out = {"mel": l_mel, "fm_mpd": fm_p, "fm_msd": fm_s, "gen_mpd": gen_p, "gen_msd": gen_s}
            if self.stft_loss is not None:
                g_total = g_total + sc + mag
                out["sc"], out["mag"] = sc, mag
            g_total.backward()
        finally:
            for p in self._d_params:
                p.requires_grad_(True)
        self._optim_step(self.optim_g)
        self.steps += 1
        out.update(d_mpd=d_p, d_msd=d_s, d_total=d_total, g_total=g_total)
        return {k: v.detach() for k, v in out.items()}

    def end_epoch(self) -> None:
        """upstream's per-epoch ExponentialLR: both learning rates times lr_decay"""
        self.optim_g.lr *= self.lr_decay
        self.optim_d.lr *= self.lr_decay
        self.epoch += 1

    def validation_step(self, mel: torch.Tensor, lens, audio: torch.Tensor) -> torch.Tensor:
        """the mel L1 of the generated audio against `mel` (upstream's validation error), under no_grad and in eval mode;
        the generator's mode is restored"""
        gen = self.generator
        was = gen.training
        gen.eval()
        try:
            with torch.no_grad():
                lens_d, _ = _lens_arg(lens, mel.shape[0], mel.shape[2], mel.device)
                return self.mel_loss(gen(mel, lens)[:, 0], mel, lens_d * gen.hop, lens_d)
        finally:
            gen.train(was)

    # ---- upstream's checkpoint pair --------------------------------------------------------------------------------------
    def save_checkpoint(self, directory: str):
        """directory/g_{steps:08d} = {"generator"}, directory/do_{steps:08d} = {"mpd", "msd", "optim_g", "optim_d", "steps",
        "epoch"} -> the two paths"""
        os.makedirs(directory, exist_ok=True)
        g_path = os.path.join(directory, f"g_{self.steps:08d}")
        do_path = os.path.join(directory, f"do_{self.steps:08d}")
        cpu = lambda sd: {k: v.detach().cpu() for k, v in sd.items()}
        torch.save({"generator": cpu(self.generator.state_dict())}, g_path)
        torch.save({"mpd": cpu(self.mpd.state_dict()), "msd": cpu(self.msd.state_dict()),
                    "optim_g": self.optim_g.state_dict(), "optim_d": self.optim_d.state_dict(), "steps": self.steps,
                    "epoch": self.epoch}, do_path)
        return g_path, do_path

    def load_checkpoint(self, directory: str, steps: Optional[int] = None) -> int:
        """steps=None: the newest do_* of the directory.  The parameters are written in place (they stay views of the flat
        buffers).  -> the checkpoint's step count"""
        if steps is None:
            found = sorted(int(f[3:]) for f in os.listdir(directory) if f.startswith("do_") and f[3:].isdigit())
            if not found:
                raise FileNotFoundError(f"no do_* checkpoint in {directory}")
            steps = found[-1]
        g = torch.load(os.path.join(directory, f"g_{steps:08d}"), map_location="cpu")
        do = torch.load(os.path.join(directory, f"do_{steps:08d}"), map_location="cpu")
        self.generator.load_state_dict(g["generator"])
        self.mpd.load_state_dict(do["mpd"])
        self.msd.load_state_dict(do["msd"])
        self.optim_g.load_state_dict(do["optim_g"])
        self.optim_d.load_state_dict(do["optim_d"])
        self.steps, self.epoch = int(do["steps"]), int(do.get("epoch", 0))
        return self.steps
