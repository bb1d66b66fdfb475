#!/usr/bin/env python3
"""Batched synthesis benchmark (rad_mmm_amd/synthesis.py, csrc/synth.hip): one JSON line.

    python tools/synth_bench.py [--iters 10] [--warmup 3]

At the joint config (bench.CONFIGS["joint"]: the RADMMM decoder + the four ConvLSTMLinearDAP predictors, random weights
from a seed, durations of ~4 frames per token), 150 tokens, B = 1 and 32: ms per phase of sample_full (encoder;
duration predictor + quantisation + the host read + regulation; frame-rate predictors; f0; decoder; vocoder with HiFi-GAN
V1) and of the whole call; and each new kernel against the torch expressions it replaces on the same inputs (the torch length regulator this package used before,
attribute_predictors._rows' permute + pad, the reference's boolean-index f0 code), with achieved bandwidth against the
HBM roofline: 8 TB/s on paper, ~6.3 TB/s for a measured float4 copy (MI355X microarchitecture guide).  Device events
around each timed call, after warm-up."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HBM_PAPER, HBM_COPY = 8.0e12, 6.3e12


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


# ---- the torch expressions the kernels replace (inlined: they are no longer in the package) -----------------------------
def torch_regulator(x, dur):
    """the torch RADMMMFlow.length_regulator this change deletes: x [B, T_txt, C], dur [B, T_txt]"""
    B, Tt, C = x.shape
    dur = dur.long().clamp_min(0)
    cum = torch.cumsum(dur, 1)
    total = cum[:, -1]
    Tmax = int(total.max())
    t = torch.arange(Tmax, device=x.device)[None, :].expand(B, -1).contiguous()
    idx = torch.searchsorted(cum, t, right=True).clamp_max(Tt - 1)
    out = torch.gather(x, 1, idx[:, :, None].expand(-1, -1, C))
    return out * (t < total[:, None])[:, :, None].to(x.dtype)


def torch_rows(x):
    """attribute_predictors._rows: [B, C, T] -> [B*T, round_up(C, 32)]"""
    B, C, T = x.shape
    y = x.float().permute(0, 2, 1)
    if C % 32:
        y = F.pad(y, (0, (-C) % 32))
    return y.reshape(B * T, -1).contiguous()


def torch_durations(d, mask):
    """tts_lightning_modules.py:345-346"""
    return (torch.clamp(torch.round(d), min=1) * mask).long()


def torch_f0(f0_pred, v_logit, f0_mean, f0_std):
    """tts_lightning_modules.py:354-376 (boolean indexing: host synchronisations)"""
    voiced = torch.sigmoid(v_logit) > 0.5
    f0_pred = f0_pred * voiced
    f0_mu, f0_sigma = f0_pred[voiced].mean(), f0_pred[voiced].std()
    f0_pred[voiced] = (f0_pred[voiced] - f0_mu) / f0_sigma
    m = f0_mean[:, None, None].expand(-1, 1, f0_pred.shape[2])
    s = f0_std[:, None, None].expand(-1, 1, f0_pred.shape[2])
    f0_pred[voiced] = f0_pred[voiced] * s[voiced] + m[voiced]
    return f0_pred, voiced


def build(dev):
    import bench
    import radmmm_synth as S
    from _vocoder_ref import V1, random_state
    from rad_mmm_amd.decoders import RADMMMFlow
    from rad_mmm_amd.vocoder import Denoiser, HiFiGANGenerator
    CFG = bench.CONFIGS["joint"]
    cfg = S.DecoderConfig(**CFG)
    dec = RADMMMFlow(use_accent=True, **CFG)
    dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in
                         S.procedural_decoder_state(S.decoder_state_shapes(cfg), end_scale=0.002).items()})
    model = bench.build_step_model(dec.to(dev), CFG, dev, joint=True)
    with torch.no_grad():
        model.duration_predictor.feat_pred_fn.dense.bias.fill_(float(np.log(5.0)))
        model.voiced_predictor.feat_pred_fn.dense.bias.fill_(0.0)
    model.eval()
    model.decoder.enable_inverse_cache()
    gen = HiFiGANGenerator(V1)
    gen.load_state_dict(random_state(gen, 5, 0.2, 0.6))
    gen = gen.to(dev).eval()
    model.synth_vocoder = (gen, Denoiser(gen).to(dev))
    return model


@torch.no_grad()
def phases(model, B, L, iters, warmup, dev):
    from rad_mmm_amd.attribute_predictors import dap_forward_many
    from rad_mmm_amd.common import SequenceLength
    from rad_mmm_amd import synthesis as Y
    g = torch.Generator().manual_seed(B)
    text = torch.randint(0, 185, (B, L), generator=g).to(dev)
    lens_h = torch.full((B,), L)
    spk, acc = torch.randint(0, 8, (B,), generator=g).to(dev), torch.randint(0, 4, (B,), generator=g).to(dev)
    fm, fs = torch.full((B,), 150.0, device=dev), torch.full((B,), 25.0, device=dev)
    in_lens = SequenceLength(lens_h.to(dev), lens_h)
    sv, av = model.encode_speaker(spk), model.encode_accent(acc)
    r = {}
    st = {}

    def enc():
        st["txt"] = model.encode_text(text, in_lens.lengths, None, L)[0]
    r["encoder"] = timed(enc, iters, warmup)
    txt = st["txt"]

    def durs():
        d = model.duration_predictor.infer(txt, sv, in_lens, accent_emb=av)
        dur, cum, o32 = Y.synth_durations(d, in_lens.lengths)
        fr = o32.cpu()
        st.update(dur=dur, cum=cum, o32=o32, fr=fr, rows=Y.synth_regulate(txt.transpose(1, 2), cum, o32, int(fr.max())))
    r["duration_predictor_quantisation_read_regulation"] = timed(durs, iters, warmup)
    o32, fr, rows = st["o32"], st["fr"], st["rows"]
    Tmax = int(fr.max())
    ctx = Y.rows_as_context(rows, B, txt.shape[1])
    ol = SequenceLength(o32.long(), fr.long())

    def preds():
        calls = [((None, ctx, sv, ol), {"accent_emb": av})] * 3
        st["p"] = dap_forward_many([model.f0_predictor, model.energy_predictor, model.voiced_predictor], calls, rows=rows)
    r["predictors"] = timed(preds, iters, warmup)
    f0h, enh, vh = (o["x_hat"] for o in st["p"])

    def f0k():
        st["f"] = Y.synth_f0(f0h, vh, enh, o32, fm, fs)
    r["f0"] = timed(f0k, iters, warmup)
    f0, en, _ = st["f"]
    res = torch.randn(B, 160, Tmax // 2, device=dev)

    def decode():
        st["mel"] = model.decoder.infer_context(sv, ctx, ol, 1.0, f0, en, None, res)["mel"]
    r["decoder"] = timed(decode, iters, warmup)
    mel = Y.mel_descale(st["mel"])
    r["vocoder"] = timed(lambda: model.vocode_mels(mel, fr // 2 * 2), max(2, iters // 3), 1)
    r["sample_full"] = timed(lambda: model.sample_full(text, lens_h, spk, accent_ids=acc, f0_mean=fm, f0_std=fs),
                             max(2, iters // 3), 1)
    r["frames"] = int(fr.sum())
    r["audio_seconds"] = float((fr // 2 * 2).sum()) * 256 / 22050

    # ---- kernels against the torch expressions, same inputs
    k = {}
    d_pred = model.duration_predictor.infer(txt, sv, in_lens, accent_emb=av)
    mask = in_lens.mask.unsqueeze(1)
    k["durations"] = {"hip_us": 1e3 * timed(lambda: Y.synth_durations(d_pred, in_lens.lengths), iters, warmup),
                      "torch_us": 1e3 * timed(lambda: torch_durations(d_pred, mask), iters, warmup)}
    x = txt.transpose(1, 2)
    C = x.shape[2]
    ldc = (C + 31) // 32 * 32
    cum = st["cum"]
    hip_reg = 1e3 * timed(lambda: Y.synth_regulate(x, cum, o32, Tmax), iters, warmup)
    tor_reg = 1e3 * timed(lambda: torch_rows(torch_regulator(x, st["dur"]).transpose(1, 2)), iters, warmup)
    byts = B * Tmax * ldc * 4 + int(fr.sum()) * C * 4          # rows written + the text rows read (one per frame)
    k["regulate"] = {"hip_us": hip_reg, "torch_us": tor_reg, "bytes": byts, "hip_TBs": byts / hip_reg / 1e6,
                     "frac_of_8TBs": byts / hip_reg / 1e-6 / HBM_PAPER, "frac_of_6p3TBs": byts / hip_reg / 1e-6 / HBM_COPY}
    hip_f0 = 1e3 * timed(lambda: Y.synth_f0(f0h, vh, enh, o32, fm, fs), iters, warmup)
    tor_f0 = 1e3 * timed(lambda: torch_f0(f0h.clone(), vh, fm, fs), iters, warmup)
    fb = B * Tmax * 4 * (3 + 3) + B * Tmax * 4 * 2             # stats read f0 + v; apply reads 3, writes 3
    k["f0"] = {"hip_us": hip_f0, "torch_us": tor_f0, "bytes": fb, "hip_TBs": fb / hip_f0 / 1e6,
               "frac_of_8TBs": fb / hip_f0 / 1e-6 / HBM_PAPER}
    r["kernels"] = k
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("synth_bench needs an MI355X")
    dev = torch.device("cuda:0")
    model = build(dev)
    out = {"metric": "synthesis_ms", "tokens": 150, "by_batch": {}}
    for B in (1, 32):
        out["by_batch"][str(B)] = phases(model, B, 150, args.iters, args.warmup, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
