"""Batched text-to-speech synthesis: token ids -> mel -> waveform for a whole padded batch (reference
TTSModel.sample_full, reconstruct_from_batch_attributes and mel_descale, tts_lightning_modules.py:286-437, 547-549).

The modules are the package's own (encoder.Encoder, attribute_predictors.ConvLSTMLinearDAP, decoders.RADMMMFlow,
vocoder.vocode); the glue the reference runs in Python per utterance and per token is new HIP (csrc/synth.hip):
  synth_durations  duration quantisation clamp(round(d), 1) * mask, prefix sums and frame counts
  synth_regulate   LengthRegulator as one gather into the channels-last rows the frame-rate predictors read
  synth_f0         voiced gate, f0 * voiced and the shift-stats renormalisation, decided on the device
A synthesis call reads the device once: the B frame counts, which size everything downstream.

Deliberate differences from the reference:
  - a predicted duration is capped at 65536 frames per token (the reference has no guard against non-finite or absurd
    predictions);
  - the shift statistics pool only frames inside each utterance's length (the reference pools every padded frame whose
    voiced logit is positive: padded frames carry the voiced predictor's dense bias there); with fewer than 2 voiced frames
    (or sigma == 0) f0 stays unshifted, where the reference produces NaN;
  - reconstruct_from_batch_attributes honours a given `durations` (the reference ignores the argument);
  - the vocoder receives out_lens // g * g frames, the frames the decoder produced.
Raw strings, the text processor and the reference's `language` argument are out of scope ("text front end"):
the entry points take token ids."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from ._lib import lib, check, ptr, stream, fp32_region
from .common import SequenceLength

LD_PAD = 32          # channel padding of the regulated rows: attribute_predictors._rows' layout
F0_PARTS = 64        # workgroups of radmmm_synth_f0_stats


def mel_descale(mel):
    """tts_lightning_modules.py:547-549"""
    from .tts_step import TTSTrainingStep
    return TTSTrainingStep.mel_descale(mel)


# ---------------------------------------------------------------------------------------------------- kernels
def synth_durations(x: torch.Tensor, text_lens: Optional[torch.Tensor], integer_mode: bool = False):
    """x [B, Tt] or [B, 1, Tt] fp32 (unit stride along tokens, any item stride: the predictor's output is read in place)
    -> (dur int32 [B, Tt], inclusive prefix sums int32 [B, Tt], out_lens int32 [B]).  Tokens at or past text_lens[b] get
    0 frames; the others clamp(rint(x), 1) (integer_mode: x itself, no rounding, no clamp to 1), at most 65536."""
    if x.dim() == 3:
        x = x[:, 0]
    if x.dtype != torch.float32 or x.stride(1) != 1:
        x = x.float().contiguous()
    B, Tt = x.shape
    item_stride = x.stride(0) if B > 1 else Tt
    dur = torch.empty(B, Tt, device=x.device, dtype=torch.int32)
    cum = torch.empty_like(dur)
    out_lens = torch.empty(B, device=x.device, dtype=torch.int32)
    tl = None if text_lens is None else text_lens.to(device=x.device, dtype=torch.int32).contiguous()
    check(lib.radmmm_synth_durations(ptr(x), item_stride, ptr(tl), B, Tt, 1 if integer_mode else 0, ptr(dur), ptr(cum),
                                     ptr(out_lens), stream()), "radmmm_synth_durations")
    return dur, cum, out_lens


def synth_regulate(txt: torch.Tensor, cum: torch.Tensor, out_lens: torch.Tensor, Tmax: int) -> torch.Tensor:
    """txt [B, Tt, C] (the encoder's native layout; read in place with unit channel stride and 16-byte rows, any item
    stride) -> frame rows [B * Tmax, round_up(C, 32)], the layout of attribute_predictors._rows(context): text frame j
    repeated dur[j] times, zeros past out_lens[b] and in the pad channels.  A pure copy.  Tt <= 16384 (the prefix sums
    are staged in LDS); larger raises."""
    B, Tt, C = txt.shape
    ldc = (C + LD_PAD - 1) // LD_PAD * LD_PAD
    if C % 4:                                   # the kernel copies float4s: widen to C4 zero channels (inside ldc's padding)
        txt = torch.nn.functional.pad(txt.float(), (0, (-C) % 4))
    elif (txt.dtype != torch.float32 or txt.stride(2) != 1 or txt.stride(1) % 4 or (B > 1 and txt.stride(0) % 4)
            or txt.data_ptr() % 16):
        txt = txt.float().contiguous()
    C4 = txt.shape[2]
    rows = torch.empty(B * Tmax, ldc, device=txt.device, dtype=torch.float32)
    item_stride = txt.stride(0) if B > 1 else Tt * txt.stride(1)
    check(lib.radmmm_synth_regulate(ptr(txt), item_stride, txt.stride(1), Tt, C4, ptr(cum), ptr(out_lens), B, Tmax,
                                    ptr(rows), ldc, stream()), "radmmm_synth_regulate")
    return rows


def rows_as_context(rows: torch.Tensor, B: int, C: int) -> torch.Tensor:
    """[B * T, ldc] frame rows -> the [B, C, T] context (a strided view, no copy)"""
    return rows.view(B, -1, rows.shape[1])[:, :, :C].transpose(1, 2)


def synth_f0(f0: torch.Tensor, voiced_logit: torch.Tensor, energy: torch.Tensor, lens32: torch.Tensor,
             f0_mean: Optional[torch.Tensor] = None, f0_std: Optional[torch.Tensor] = None):
    """f0, voiced logits, energy [B, T] or [B, 1, T] (unit stride along frames) -> contiguous (f0, energy, voiced) [B, T]:
    voiced = sigmoid(v) > 0.5 inside lens32[b]; f0 * voiced; with f0_mean / f0_std [B] the shift-stats renormalisation
    (f0 - mu) / sigma * f0_std[b] + f0_mean[b] on the voiced frames, mu / sigma pooled over the batch's voiced frames."""
    def flat(t):
        t = t[:, 0] if t.dim() == 3 else t
        return t if (t.dtype == torch.float32 and t.stride(1) == 1) else t.float().contiguous()
    f0, voiced_logit, energy = flat(f0), flat(voiced_logit), flat(energy)
    B, T = f0.shape

    def istride(t):
        return t.stride(0) if B > 1 else T
    out = torch.empty(3, B, T, device=f0.device, dtype=torch.float32)
    parts = None
    if f0_mean is not None:
        f0_mean = f0_mean.to(device=f0.device, dtype=torch.float32).reshape(B).contiguous()
        f0_std = f0_std.to(device=f0.device, dtype=torch.float32).reshape(B).contiguous()
        parts = torch.empty(3 * F0_PARTS, device=f0.device, dtype=torch.float64)
        check(lib.radmmm_synth_f0_stats(ptr(f0), istride(f0), ptr(voiced_logit), istride(voiced_logit), ptr(lens32), B, T,
                                        ptr(parts), F0_PARTS, stream()), "radmmm_synth_f0_stats")
    check(lib.radmmm_synth_f0_apply(ptr(f0), istride(f0), ptr(voiced_logit), istride(voiced_logit), ptr(energy),
                                    istride(energy), ptr(lens32), B, T, ptr(parts), F0_PARTS, ptr(f0_mean), ptr(f0_std),
                                    ptr(out[0]), ptr(out[1]), ptr(out[2]), stream()), "radmmm_synth_f0_apply")
    return out[0], out[1], out[2]


# ---------------------------------------------------------------------------------------------------- pipeline
def _frames_host(out_lens: torch.Tensor, g: int, vocode: bool) -> torch.Tensor:
    """the ONE device -> host read of a synthesis call, and the checks that need it (before any decoder work)"""
    host = out_lens.cpu().long()
    for b, n in enumerate(host.tolist()):
        if n < g:
            raise ValueError(f"utterance {b} has {n} frames: the decoder needs at least n_group_size = {g}")
        if vocode and n // g * g < 3:
            raise ValueError(f"utterance {b} has {n} frames: the vocoder's denoiser needs at least 3")
    return host


def _check_residual(residual, B, C0, Tg, sigma, like):
    if residual is None:
        return torch.randn(B, C0, Tg, device=like.device) * sigma
    if tuple(residual.shape) != (B, C0, Tg):
        raise ValueError(f"residual must have shape [B, n_mel * n_group_size, Tmax // n_group_size] = {[B, C0, Tg]}, "
                         f"got {list(residual.shape)}")
    return residual.to(like.device).float()


def _require_cuda(**tensors):
    for name, t in tensors.items():
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"{name} is a CPU tensor: synthesis runs on the GPU (move the ids and the model there)")


def _accent_used(model) -> bool:
    preds = (model.f0_predictor, model.energy_predictor, model.voiced_predictor, model.duration_predictor)
    return bool(model.use_accent_emb_for_encoder or getattr(model.decoder, "use_accent_emb_for_decoder", False)
                or any(getattr(p, "use_accent_embedding", False) for p in preds if p is not None))


def _vocode(model, mel, frames_host, vocode):
    if not vocode:
        return None
    return model.vocode_mels(mel, frames_host)


@torch.no_grad()
@fp32_region
def sample_full(model, text, text_lengths, speaker_ids, decoder_speaker_ids=None, f0_speaker_ids=None,
                energy_speaker_ids=None, duration_speaker_ids=None, accent_ids=None, f0_mean=None, f0_std=None,
                shift_stats=True, sigma=1.0, residual=None, vocode=True) -> Dict[str, object]:
    """TTSModel.sample_full (tts_lightning_modules.py:286-384) for a padded batch of token ids.
    model: a TTSTrainingStep with the four attribute predictors; text [B, L] token ids, text_lengths [B] (host or
    device), speaker / accent ids [B]; f0_mean / f0_std [B] with shift_stats: renormalise the predicted f0 to these
    statistics.  residual: the decoder's noise [B, n_mel * g, Tmax // g], already scaled by sigma (default: sampled).
    Returns {mel (descaled) [B, n_mel, Tmax // g * g], out_lens [B] (host), durations [B, L], f0, energy, voiced [B, Tmax],
    residual, audio (list of numpy waveforms, out_lens[b] // g * g * hop samples each, or None)}."""
    for name in ("duration", "f0", "energy", "voiced"):
        if getattr(model, f"{name}_predictor") is None:
            raise ValueError(f"sample_full needs a {name} predictor (model.{name}_predictor is None)")
    if accent_ids is None and _accent_used(model):
        raise ValueError("sample_full: this model uses accent embeddings: pass accent_ids")
    if vocode and model.synth_vocoder is None:
        raise RuntimeError("sample_full: attach a vocoder first (step.synth_vocoder = load_hifigan_vocoder(...)) or pass "
                           "vocode=False")
    _require_cuda(text=text, speaker_ids=speaker_ids, decoder_speaker_ids=decoder_speaker_ids,
                  f0_speaker_ids=f0_speaker_ids, energy_speaker_ids=energy_speaker_ids,
                  duration_speaker_ids=duration_speaker_ids, accent_ids=accent_ids)
    dev = text.device
    if not model.text_embeddings.weight.is_cuda:
        raise RuntimeError("sample_full: the model is on the CPU: synthesis runs on the GPU")
    dec = model.decoder
    g = dec.n_group_size
    B = text.shape[0]
    if text_lengths.is_cuda:
        in_lens = SequenceLength(text_lengths)                                # (a device -> host read)
    else:                                                                     # pinned + async: no synchronisation
        lens_host = text_lengths.long()
        in_lens = SequenceLength(lens_host.pin_memory().to(dev, non_blocking=True), lens_host)
    max_in = int(in_lens.lengths_host.max())

    def spk(ids):
        return model.encode_speaker(speaker_ids if ids is None else ids)
    dec_spk, f0_spk, en_spk, dur_spk = spk(decoder_speaker_ids), spk(f0_speaker_ids), spk(energy_speaker_ids), \
        spk(duration_speaker_ids)
    accent_vecs = model.encode_accent(accent_ids) if accent_ids is not None else None
    txt_enc, _ = model.encode_text(text, in_lens.lengths, accent_vecs if model.use_accent_emb_for_encoder else None, max_in)

    # durations: predictor, quantisation, ONE read of the frame counts
    d_pred = model.duration_predictor.infer(txt_enc, dur_spk, in_lens, accent_emb=accent_vecs)
    dur, cum, out32 = synth_durations(d_pred, in_lens.lengths)
    frames = _frames_host(out32, g, vocode)
    Tmax = int(frames.max())
    enc_rows = txt_enc.transpose(1, 2)                                   # [B, L, C]: the encoder's own layout, a view
    C = enc_rows.shape[2]
    rows = synth_regulate(enc_rows, cum, out32, Tmax)
    context = rows_as_context(rows, B, C)
    out_lens = SequenceLength(out32.long(), frames)

    # the frame-rate predictors on the regulated rows: one merged bi-LSTM recurrence
    from .attribute_predictors import dap_forward_many
    calls = [((None, context, f0_spk, out_lens), {"accent_emb": accent_vecs}),
             ((None, context, en_spk, out_lens), {"accent_emb": accent_vecs}),
             ((None, context, f0_spk, out_lens), {"accent_emb": accent_vecs})]
    preds = (model.f0_predictor, model.energy_predictor, model.voiced_predictor)
    outs = dap_forward_many(list(preds), calls, rows=rows)
    f0_hat = model.f0_predictor.inv_tx_data(outs[0]["x_hat"], f0_mean, f0_std)
    en_hat = model.energy_predictor.inv_tx_data(outs[1]["x_hat"])
    v_hat = model.voiced_predictor.inv_tx_data(outs[2]["x_hat"])
    shift = shift_stats and f0_mean is not None
    f0, energy, voiced = synth_f0(f0_hat, v_hat, en_hat, out32, f0_mean if shift else None, f0_std if shift else None)

    C0 = dec.n_mel_channels * g
    residual = _check_residual(residual, B, C0, Tmax // g, sigma, txt_enc)
    mel = dec.infer_context(dec_spk, context, out_lens, sigma, f0, energy,
                            accent_vecs if dec.use_accent_emb_for_decoder else None, residual)["mel"]
    mel = mel_descale(mel)
    return {"mel": mel, "out_lens": frames, "durations": dur, "f0": f0, "energy": energy, "voiced": voiced,
            "residual": residual, "audio": _vocode(model, mel, frames // g * g, vocode)}


@torch.no_grad()
@fp32_region
def reconstruct_from_batch_attributes(model, batch: Dict[str, torch.Tensor], durations=None, vocode=True,
                                      residual=None) -> Dict[str, object]:
    """TTSModel.reconstruct_from_batch_attributes (tts_lightning_modules.py:389-437): the batch's text, speaker, f0 and
    energy with the durations of its binarised alignment (attention + on-device MAS), durations = attn[:, 0].sum(1).
    A given `durations` [B, L] (integer frame counts) is used instead (the reference ignores the argument).  batch keys as
    TTSTrainingStep.training_step (+ optional *_lengths_host).  Returns {output_mel (descaled), output_audio, attn_used,
    attn_soft, out_lens (host), durations, residual}."""
    if vocode and model.synth_vocoder is None:
        raise RuntimeError("reconstruct_from_batch_attributes: attach a vocoder first or pass vocode=False")
    _require_cuda(text=batch["text"], mel=batch["mel"])
    dec = model.decoder
    g = dec.n_group_size
    in_lens = SequenceLength(batch["input_lengths"], batch.get("input_lengths_host"))
    mel_lens = SequenceLength(batch["output_lengths"], batch.get("output_lengths_host"))
    max_in = int(in_lens.lengths_host.max())
    mel = model.mel_scale(batch["mel"])
    spk_vecs = model.encode_speaker(batch["speaker_ids"])
    accent_vecs = model.encode_accent(batch["accent_ids"]) if model.use_accent else None
    txt_enc, txt_emb = model.encode_text(batch["text"], in_lens.lengths,
                                         accent_vecs if model.use_accent_emb_for_encoder else None, max_in)
    attn, attn_soft, _, _ = model.compute_attention(mel, txt_emb, spk_vecs, accent_vecs, mel_lens.lengths, in_lens.lengths,
                                                    batch["attn_prior"], True, max_in)
    if durations is None:
        durations = attn[:, 0].sum(1)
    elif not durations.is_cuda:
        raise RuntimeError("durations is a CPU tensor: synthesis runs on the GPU")
    dur, cum, out32 = synth_durations(durations.float(), in_lens.lengths, integer_mode=True)
    frames = _frames_host(out32, g, vocode)
    Tmax = int(frames.max())
    B = txt_enc.shape[0]
    enc_rows = txt_enc.transpose(1, 2)
    rows = synth_regulate(enc_rows, cum, out32, Tmax)
    context = rows_as_context(rows, B, enc_rows.shape[2])
    out_lens = SequenceLength(out32.long(), frames)

    def track(t):
        if t is None:
            return None
        t = t.float()
        return t[:, :Tmax] if t.shape[1] >= Tmax else torch.nn.functional.pad(t, (0, Tmax - t.shape[1]))
    residual = _check_residual(residual, B, dec.n_mel_channels * g, Tmax // g, 1.0, txt_enc)
    out = dec.infer_context(spk_vecs, context, out_lens, 1.0, track(batch.get("f0")), track(batch.get("energy_avg")),
                            accent_vecs if dec.use_accent_emb_for_decoder else None, residual)
    mel_out = mel_descale(out["mel"])
    return {"output_mel": mel_out, "output_audio": _vocode(model, mel_out, frames // g * g, vocode), "attn_used": attn,
            "attn_soft": attn_soft, "out_lens": frames, "durations": dur, "residual": residual}
