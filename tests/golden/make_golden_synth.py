#!/usr/bin/env python3
"""Generate tests/golden/synth_small.npz by RUNNING THE REFERENCE's components in the order of TTSModel.sample_full.

Run in the build container only (needs the reference checkout):

    python tests/golden/make_golden_synth.py [--ref /root/reference]

tts_lightning_modules imports pytorch_lightning (absent), so TTSModel cannot be imported: the step is composed here from
the reference's own modules -- common.Encoder, attribute_predictors.ConvLSTMLinearDAP (infer) for all four predictors,
common.LengthRegulator and decoders.RADMMMFlow.infer -- and the few inline glue lines of sample_full are restated below
with their line citations.  Same stand-ins as make_golden.py (numba.jit, librosa helpers) and the same CPU noise stream
for decoders.py:221.  Nothing of the reference's source is written into this repo: the fixture holds inputs, the weights
of the small modules (the decoder's are procedural: oracle.procedural_decoder_state, end_scale 0.002, rebuilt by the
tests) and the outputs the reference computed.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

# fixture dimensions (read back by the tests from the "cfg." / "dims." keys)
N_TEXT, N_TOKENS, N_SPK, N_ACC = 32, 40, 4, 3
DECODER = dict(n_speaker_dim=16, use_accent_emb_for_decoder=False, n_accent_dim=8, n_text_dim=N_TEXT, n_f0_dims=1,
               n_energy_avg_dims=1, n_mel_channels=80, n_early_size=2, n_early_every=2, n_group_size=2,
               scaling_fn="tanh", affine_activation="softplus", use_partial_padding=True, n_conv_layers_per_step=4,
               n_flows=2)
# the joint config's predictor targets (bench.JOINT_PREDICTORS) at small widths
PREDICTORS = {"f0": dict(target_offset=-5.0), "energy": dict(target_offset=-0.75), "voiced": dict(),
              "duration": dict(log_target=True)}
DAP = dict(n_speaker_dim=16, n_accent_dim=8, use_accent_embedding=True, in_dim=N_TEXT, out_dim=1, reduction_factor=4,
           n_backbone_layers=2, n_hidden=16, kernel_size=3, p_dropout=0.25, lstm_type="bilstm")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    from make_golden import install_stubs, save, t2n
    install_stubs()
    sys.path[:0] = [args.ref, os.path.join(args.ref, "vocoders")]
    cwd = os.getcwd()
    os.chdir("/tmp")
    import torch
    torch.set_num_threads(8)
    import common
    import decoders
    import attribute_predictors as ref_ap
    from oracle import radmmm_oracle as O
    os.chdir(cwd)

    torch.manual_seed(77)
    mods = torch.nn.ModuleDict(dict(
        text_embeddings=torch.nn.Embedding(N_TOKENS, N_TEXT), text_encoder=common.Encoder(3, N_TEXT, 5, lstm_norm_fn=None),
        speaker_embeddings=torch.nn.Embedding(N_SPK, 16), accent_embeddings=torch.nn.Embedding(N_ACC, 8),
        **{f"{n}_predictor": ref_ap.ConvLSTMLinearDAP(**DAP, **PREDICTORS[n]) for n in PREDICTORS}))
    dec = decoders.RADMMMFlow(use_accent=True, **DECODER)
    cfg = O.DecoderConfig(**DECODER)
    proc = O.procedural_decoder_state({n: tuple(p.shape) for n, p in dec.state_dict().items()}, end_scale=0.002)
    dec.load_state_dict({n: torch.from_numpy(np.asarray(v)) for n, v in proc.items()})
    with torch.no_grad():
        for n in PREDICTORS:                 # converge the spectral norms' power iteration (as bench.build_step_model)
            lstm = mods[f"{n}_predictor"].feat_pred_fn.bilstm
            lstm.train()
            for _ in range(20):
                for hook in lstm._forward_pre_hooks.values():
                    hook(lstm, ())
        # tokens of ~2-6 frames (log target: exp(x) - 1), a mix of voiced and unvoiced frames with padded frames unvoiced
        mods["duration_predictor"].feat_pred_fn.dense.bias.fill_(float(np.log(3.2)))
        mods["duration_predictor"].feat_pred_fn.dense.weight.mul_(4.0)
        mods["voiced_predictor"].feat_pred_fn.dense.bias.fill_(-0.93)
        mods["voiced_predictor"].feat_pred_fn.dense.weight.mul_(6.0)
    mods.eval()
    dec.eval()

    g = torch.Generator().manual_seed(5)
    B, L = 3, 11
    text_lens = torch.tensor([11, 8, 5])
    text = torch.randint(1, N_TOKENS, (B, L), generator=g) * (torch.arange(L)[None] < text_lens[:, None])
    speaker_ids, accent_ids = torch.tensor([0, 3, 1]), torch.tensor([2, 0, 1])
    f0_mean, f0_std = torch.tensor([5.2, 4.6, 5.9]), torch.tensor([0.35, 0.5, 0.25])
    sigma, seed = 0.8, 4242
    # decoders.py:221 allocates the noise with torch.cuda.FloatTensor: the CPU type stands in (seeded normal_() stream)
    torch.cuda.FloatTensor = torch.FloatTensor

    with torch.no_grad():
        # tts_lightning_modules.py:299-303: lengths as a SequenceLength (token ids given: the text processor is skipped)
        txt_lens = common.SequenceLength(text_lens)
        # :319-326 speaker vectors per role (defaults: speaker_ids); :328-330 accent vectors
        spk_vecs = mods["speaker_embeddings"](speaker_ids)
        accent_vecs = mods["accent_embeddings"](accent_ids)
        # :345-351 encode_text (:246-268, accent not fed to the encoder): embeddings -> Encoder -> [B, C, L]
        emb = mods["text_embeddings"](text).transpose(1, 2)
        txt_enc = mods["text_encoder"](emb, txt_lens.lengths).transpose(1, 2)
        # :354-357 durations
        durations = mods["duration_predictor"].infer(txt_enc, spk_vecs, txt_lens, accent_emb=accent_vecs)
        durations_int = (torch.clamp(torch.round(durations), min=1) * txt_lens.mask.unsqueeze(1)).long()
        # :360-361 LengthRegulator
        context = common.LengthRegulator()(txt_enc.transpose(1, 2), durations_int[:, 0]).transpose(1, 2)
        # :364-366 attributes
        out_lens = common.SequenceLength(durations_int[:, 0].sum(1))
        v_logit = mods["voiced_predictor"].infer(context, spk_vecs, out_lens, accent_emb=accent_vecs)
        voiced_pred = torch.sigmoid(v_logit) > 0.5
        f0_pred = mods["f0_predictor"].infer(context, spk_vecs, out_lens, x_mean=f0_mean, x_std=f0_std,
                                             accent_emb=accent_vecs) * voiced_pred
        # :371-382 shift stats
        f0_mu, f0_sigma = f0_pred[voiced_pred].mean(), f0_pred[voiced_pred].std()
        f0_pred[voiced_pred] = (f0_pred[voiced_pred] - f0_mu) / f0_sigma
        f0_mean_exp = f0_mean[:, None, None].expand(-1, 1, f0_pred.shape[2])
        f0_std_exp = f0_std[:, None, None].expand(-1, 1, f0_pred.shape[2])
        f0_pred = f0_pred.float()
        f0_pred[voiced_pred] = f0_pred[voiced_pred].float() * f0_std_exp[voiced_pred].float() + \
            f0_mean_exp[voiced_pred].float()
        # :384
        energy_pred = mods["energy_predictor"].infer(context, spk_vecs, out_lens, accent_emb=accent_vecs)
        # :387-388 sample_decoder -> RADMMMFlow.infer (:423-425), then mel_descale (:547-549)
        torch.manual_seed(seed)
        out = dec.infer(spk_vecs, txt_enc, sigma, dur=durations_int.squeeze(1), f0=f0_pred[:, 0],
                        energy_avg=energy_pred[:, 0], out_lens=out_lens.lengths, accent_vecs=accent_vecs)
        mel = out["mel"] * 2 - 5
        torch.manual_seed(seed)
        Tmax = int(out_lens.lengths.max())
        residual = torch.FloatTensor(B, cfg.n_mel_channels * cfg.n_group_size, Tmax // cfg.n_group_size).normal_() * sigma

    n = out_lens.lengths
    valid = torch.arange(Tmax)[None] < n[:, None]
    assert not (voiced_pred[:, 0] & ~valid).any(), "a padded frame is voiced: the shift stats would differ (DESIGN §4.17)"
    nv = int(voiced_pred[:, 0][valid].sum())
    # decision margins: how far the values the HIP / oracle runs must agree on lie from their thresholds
    dv = durations[:, 0][txt_lens.mask]
    print(f"min |v_logit| {float(v_logit[:, 0][valid].abs().min()):.2e}, "
          f"min |frac(d) - 0.5| {float((dv - torch.floor(dv) - 0.5).abs().min()):.2e}")
    assert 2 <= nv < int(n.sum()), nv
    d = durations_int[:, 0][durations_int[:, 0] > 0]
    print(f"frames {n.tolist()}, durations {int(d.min())}..{int(d.max())}, voiced {nv} of {int(n.sum())}")
    arrs = {"text": text, "text_lens": text_lens, "speaker_ids": speaker_ids, "accent_ids": accent_ids, "f0_mean": f0_mean,
            "f0_std": f0_std, "sigma": sigma, "seed": seed, "end_scale": 0.002, "residual": residual,
            "d_pred": durations[:, 0], "durations": durations_int[:, 0], "out_lens": n, "v_logit": v_logit[:, 0],
            "voiced": voiced_pred[:, 0], "f0": f0_pred[:, 0], "energy": energy_pred[:, 0], "mel": mel}
    for k, v in mods.state_dict().items():
        arrs["sd." + k] = v
    for k, v in DECODER.items():
        arrs["cfg." + k] = np.asarray(v)
    for k, v in {"n_text": N_TEXT, "n_tokens": N_TOKENS, "n_spk": N_SPK, "n_acc": N_ACC}.items():
        arrs["dims." + k] = np.asarray(v)
    save("synth_small.npz", **t2n(arrs))


if __name__ == "__main__":
    main()
