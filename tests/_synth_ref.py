"""CPU restatement of batched synthesis (TTSModel.sample_full, tts_lightning_modules.py:319-384) from the oracle's pieces:
encoder_forward, dap_forward (speaker and accent concatenated, as oracle.tts_joint_step feeds the joint predictors),
length_regulate and decoder_infer.  Test helper, not product code.

Two points follow rad_mmm_amd.synthesis rather than the reference, on purpose: the shift statistics
pool only frames inside each utterance's length, and f0 / energy / voiced are zero past it.  Pinned to the reference's own
components on tests/golden/synth_small.npz (tests/golden/make_golden_synth.py; tests/test_synthesis_cpu.py), whose padded
frames are unvoiced so that the two rules agree there."""
import torch

from oracle import radmmm_oracle as O


def _inv_tx(x, spec):
    """AttributePredictor.inv_tx_data without target normalisation (attribute_predictors.py:120-133)"""
    if spec.get("log_target", False):
        x = torch.exp(x) - 1
    return (x - spec.get("target_offset", 0.0)) / spec.get("target_scale", 1.0)


def durations_ref(d, text_lens):
    """tts_lightning_modules.py:345-346: clamp(round(d), min=1) * mask, d [B, L] -> long [B, L]"""
    mask = O.lengths_to_mask(text_lens.long(), d.shape[1])
    return (torch.clamp(torch.round(d), min=1) * mask).long()


def f0_ref(f0, voiced, lens, f0_mean=None, f0_std=None):
    """f0 * voiced and the shift stats of tts_lightning_modules.py:355-376 over the frames inside each length;
    f0 [B, T] fp32, voiced [B, T] bool"""
    T = f0.shape[1]
    valid = O.lengths_to_mask(lens.long(), T)
    voiced = voiced & valid
    f0 = f0 * voiced
    if f0_mean is not None and int(voiced.sum()) >= 2:
        mu, sigma = f0[voiced].mean(), f0[voiced].std()
        f0 = f0.clone()
        f0[voiced] = (f0[voiced] - mu) / sigma
        f0[voiced] = f0[voiced] * f0_std[:, None].expand(-1, T)[voiced] + f0_mean[:, None].expand(-1, T)[voiced]
    return f0, voiced


def synth_ref(p, cfg, specs, text, text_lens, spk_ids, acc_ids, residual, f0_mean=None, f0_std=None, dur=None,
              voiced=None, n_enc_conv=3, role_ids=None):
    """p: the TTSTrainingStep's state_dict on the CPU; specs {name: dict(n_layers, target_offset, log_target, ...)}.
    dur / voiced: decisions to impose (the HIP run's), else the restatement's own.  role_ids: speaker ids per role
    {"decoder" | "f0" | "energy" | "duration": ids} (tts_lightning_modules.py:309-326: the voiced predictor reads the f0
    speaker), default spk_ids.  Returns the intermediate and final tensors of the synthesis (mel descaled)."""
    role_ids = role_ids or {}
    acc = p["accent_embeddings.weight"][acc_ids]

    def spk_of(role):
        return p["speaker_embeddings.weight"][role_ids.get(role, spk_ids)]
    emb = p["text_embeddings.weight"][text].transpose(1, 2)
    txt_enc = O.encoder_forward(p, "text_encoder.", emb, text_lens, n_enc_conv).transpose(1, 2)       # [B, C, L]

    def pred(name, src, lens):
        role = "f0" if name == "voiced" else name
        x = O.dap_forward(p, f"{name}_predictor.", src, torch.cat((spk_of(role), acc), 1), lens, specs[name]["n_layers"])
        return _inv_tx(x, specs[name])[:, 0]
    d_pred = pred("duration", txt_enc, text_lens)
    dur_own = durations_ref(d_pred, text_lens)
    dur = dur_own if dur is None else dur.long()
    out_lens = dur.sum(1)
    context = O.length_regulate(txt_enc.transpose(1, 2), dur).transpose(1, 2)                         # :349-350
    v_logit = pred("voiced", context, out_lens)
    f0 = pred("f0", context, out_lens)
    energy = pred("energy", context, out_lens)
    voiced_own = torch.sigmoid(v_logit) > 0.5                                                          # :354
    f0, voiced = f0_ref(f0, voiced_own if voiced is None else voiced.bool(), out_lens, f0_mean, f0_std)
    energy = energy * O.lengths_to_mask(out_lens, energy.shape[1])
    dp = {k[len("decoder."):]: v for k, v in p.items() if k.startswith("decoder.")}
    mel = O.decoder_infer(dp, cfg, spk_of("decoder"), txt_enc, residual, dur, out_lens, f0, energy,
                          acc if cfg.use_accent_emb_for_decoder else None)
    return {"mel": mel * 2 - 5, "durations": dur, "durations_own": dur_own, "d_pred": d_pred, "out_lens": out_lens,
            "f0": f0, "energy": energy, "voiced": voiced, "voiced_own": voiced_own, "v_logit": v_logit, "txt_enc": txt_enc}
