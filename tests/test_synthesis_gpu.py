"""GPU checks of batched synthesis (rad_mmm_amd/synthesis.py, csrc/synth.hip): each glue kernel against the torch / oracle
expression it replaces, RADMMMFlow.infer_context against infer, sample_full at the shipped joint dims against the CPU
restatement (tests/_synth_ref.py), the reconstruction round trip, the synchronisation budget, audio and the error paths."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = torch.device("cuda:0")


def _rel(a, b):
    return float((a.float().cpu() - b.float().cpu()).abs().max() / b.float().abs().max().clamp_min(1e-30))


# ---------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("Tt", [1, 63, 64, 65, 300, 2048])
def test_durations_match_torch(Tt):
    from rad_mmm_amd.synthesis import synth_durations
    g = torch.Generator().manual_seed(Tt)
    B = 5
    x = torch.rand(B, 1, Tt, generator=g) * 8 - 1.5
    ties = torch.tensor([0.5, -0.5, 1.5, 2.5, -1.5, 3.5, 0.49999997, -2.0])
    x[0, 0, : min(Tt, len(ties))] = ties[: min(Tt, len(ties))]
    lens = torch.tensor([Tt, max(Tt - 1, 0), Tt // 2, 1, 0])
    dur, cum, out_lens = synth_durations(x.to(DEV), lens.to(DEV))
    ref = (torch.clamp(torch.round(x[:, 0]), min=1) * (torch.arange(Tt)[None] < lens[:, None])).long()
    assert torch.equal(dur.cpu().long(), ref)
    assert torch.equal(cum.cpu().long(), torch.cumsum(ref, 1))
    assert torch.equal(out_lens.cpu().long(), ref.sum(1))
    # integer mode: unchanged, no clamp to 1, still masked
    xi = torch.randint(0, 5, (B, Tt), generator=g).float()
    dur, cum, out_lens = synth_durations(xi.to(DEV), lens.to(DEV), integer_mode=True)
    ref = (xi * (torch.arange(Tt)[None] < lens[:, None])).long()
    assert torch.equal(dur.cpu().long(), ref) and torch.equal(out_lens.cpu().long(), ref.sum(1))


def test_durations_cap_non_finite():
    from rad_mmm_amd.synthesis import synth_durations
    x = torch.tensor([[float("nan"), float("inf"), -float("inf"), 1e9, 2.0]], device=DEV)
    dur, _, out_lens = synth_durations(x, None)
    assert dur.cpu().tolist() == [[1, 65536, 1, 65536, 2]] and int(out_lens) == 2 * 65536 + 4


@pytest.mark.parametrize("C", [512, 520, 18])          # 18: a width the float4 copy takes zero-padded
@pytest.mark.parametrize("ragged", [False, True])
def test_regulate_bit_equal_to_oracle(C, ragged):
    from oracle import radmmm_oracle as O
    from rad_mmm_amd.synthesis import synth_durations, synth_regulate, rows_as_context
    g = torch.Generator().manual_seed(C)
    B = 3 if ragged else 1
    L = 37
    enc = torch.randn(B, L + 5, C, generator=g)                   # the encoder's [B, L', C], sliced to L as encode_text does
    txt = enc.to(DEV)[:, :L]
    lens = torch.tensor([L, 20, 9][:B])
    d = torch.randint(0, 7, (B, L), generator=g).float()
    dur, cum, out32 = synth_durations(d.to(DEV), lens.to(DEV), integer_mode=True)
    Tmax = int(out32.max())
    rows = synth_regulate(txt, cum, out32, Tmax)
    ldc = (C + 31) // 32 * 32
    assert rows.shape == (B * Tmax, ldc)
    ref = O.length_regulate(enc[:, :L], dur.cpu().long())                  # [B, Tmax, C]
    r = rows.view(B, Tmax, ldc).cpu()
    assert torch.equal(r[:, :, :C].view(torch.int32), ref.contiguous().view(torch.int32))
    assert not r[:, :, C:].any()
    for b in range(B):
        assert not r[b, int(out32[b]):].any()
    assert torch.equal(rows_as_context(rows, B, C).cpu(), ref.transpose(1, 2))


def test_f0_stats_match_torch_and_repeat():
    from rad_mmm_amd.synthesis import synth_f0
    from _synth_ref import f0_ref
    g = torch.Generator().manual_seed(3)
    B, T = 6, 700
    f0 = torch.rand(B, 1, T, generator=g) * 200 + 80
    v = torch.randn(B, 1, T, generator=g)
    v[0, 0, :4] = torch.tensor([1e-8, -1e-8, 0.0, 3e-7])
    en = torch.randn(B, 1, T, generator=g)
    lens = torch.tensor([700, 650, 300, 1, 2, 512], dtype=torch.int32)
    fm, fs = torch.rand(B, generator=g) * 100 + 100, torch.rand(B, generator=g) * 30 + 10
    a = synth_f0(f0.to(DEV), v.to(DEV), en.to(DEV), lens.to(DEV), fm.to(DEV), fs.to(DEV))
    b = synth_f0(f0.to(DEV), v.to(DEV), en.to(DEV), lens.to(DEV), fm.to(DEV), fs.to(DEV))
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    rf, rv = f0_ref(f0[:, 0], 1 / (1 + torch.exp(-v[:, 0])) > 0.5, lens, fm, fs)
    assert torch.equal(a[2].cpu().bool(), rv)
    assert _rel(a[0], rf) < 1e-6
    assert torch.equal(a[1].cpu(), en[:, 0] * (torch.arange(T)[None] < lens[:, None].long()))
    # fewer than 2 voiced frames: f0 * voiced, unshifted
    v1 = torch.full((B, 1, T), -5.0)
    v1[2, 0, 10] = 5.0
    f, _, vo = synth_f0(f0.to(DEV), v1.to(DEV), en.to(DEV), lens.to(DEV), fm.to(DEV), fs.to(DEV))
    assert int(vo.sum()) == 1 and float(f[2, 10]) == float(f0[2, 0, 10]) and int((f != 0).sum()) == 1


# ---------------------------------------------------------------------------------------------------- models
def _joint():
    import bench
    import radmmm_synth as S
    from rad_mmm_amd.decoders import RADMMMFlow
    CFG = bench.CONFIGS["joint"]
    cfg = S.DecoderConfig(**CFG)
    dec = RADMMMFlow(use_accent=True, **CFG)
    # the inverse flows of random weights amplify last-bit differences unless the coupling outputs are small (as
    # tests/test_infer.py: end_scale 0.002)
    dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in
                         S.procedural_decoder_state(S.decoder_state_shapes(cfg), end_scale=0.002).items()})
    model = bench.build_step_model(dec.to(DEV), CFG, DEV, joint=True)
    with torch.no_grad():       # durations of ~2-6 frames, a mix of voiced and unvoiced frames
        model.duration_predictor.feat_pred_fn.dense.bias.fill_(float(np.log(4.0)))
        model.voiced_predictor.feat_pred_fn.dense.bias.fill_(0.0)
    model.eval()
    model.decoder.enable_inverse_cache()
    specs = {name: dict(n_layers=3, **spec) for name, spec in bench.JOINT_PREDICTORS.items()}
    return model, cfg, specs


def _text(B, L, seed, ragged=True):
    g = torch.Generator().manual_seed(seed)
    lens = torch.tensor([L - (7 * (b % 8) if ragged else 0) for b in range(B)])
    text = torch.randint(0, 185, (B, L), generator=g) * (torch.arange(L)[None] < lens[:, None])
    spk, acc = torch.randint(0, 8, (B,), generator=g), torch.randint(0, 4, (B,), generator=g)
    return text, lens, spk, acc


def test_sample_full_matches_restatement_at_joint_dims():
    from _synth_ref import synth_ref
    model, cfg, specs = _joint()
    B, L = 4, 150
    text, lens, spk, acc = _text(B, L, 11)
    fm, fs = torch.tensor([120.0, 200.0, 150.0, 90.0]), torch.tensor([20.0, 35.0, 25.0, 15.0])
    # a different speaker per role (tts_lightning_modules.py:309-326), so that a mix-up of the roles shows
    roles = {"decoder": (spk + 1) % 8, "f0": (spk + 3) % 8, "energy": (spk + 5) % 8, "duration": (spk + 6) % 8}
    out = model.sample_full(text.to(DEV), lens, spk.to(DEV), accent_ids=acc.to(DEV), f0_mean=fm.to(DEV),
                            f0_std=fs.to(DEV), vocode=False,
                            **{f"{r}_speaker_ids": ids.to(DEV) for r, ids in roles.items()})
    torch.cuda.synchronize()
    p = {n: v.detach().float().cpu() if v.is_floating_point() else v.detach().cpu() for n, v in model.state_dict().items()}
    dur_h = out["durations"].cpu().long()
    with torch.no_grad():
        ref = synth_ref(p, cfg, specs, text, lens, spk, acc, out["residual"].cpu(), fm, fs, dur=dur_h,
                        voiced=out["voiced"].cpu().bool(), role_ids=roles)
    # every differing decision must come from a value within 1e-4 of its threshold
    dflip = dur_h != ref["durations_own"]
    frac = ref["d_pred"] - torch.floor(ref["d_pred"])
    print(f"duration flips: {int(dflip.sum())} of {int((ref['durations_own'] > 0).sum())}")
    assert bool(((frac[dflip] - 0.5).abs() < 1e-4).all())
    vflip = out["voiced"].cpu().bool() != (ref["voiced_own"] & (torch.arange(ref["v_logit"].shape[1])[None] <
                                                                ref["out_lens"][:, None]))
    print(f"voiced flips: {int(vflip.sum())} of {int(ref['out_lens'].sum())} frames; "
          f"voiced {int(out['voiced'].sum())}")
    assert bool((ref["v_logit"][vflip].abs() < 1e-4).all())
    assert torch.equal(out["out_lens"], ref["out_lens"])
    assert 0 < int(out["voiced"].sum()) < int(out["out_lens"].sum())
    e_f0, e_en, e_mel = _rel(out["f0"], ref["f0"]), _rel(out["energy"], ref["energy"]), 0.0
    for b in range(B):
        n = int(out["out_lens"][b]) // 2 * 2
        e_mel = max(e_mel, _rel(out["mel"][b, :, :n], ref["mel"][b, :, :n]))
    print(f"f0 {e_f0:.2e} energy {e_en:.2e} mel {e_mel:.2e}")
    assert e_f0 < 1e-4 and e_en < 1e-4 and e_mel < 1e-4


def test_infer_context_on_rows_bit_equal_to_infer():
    from rad_mmm_amd.synthesis import synth_durations, synth_regulate, rows_as_context
    model, cfg, _ = _joint()
    dec = model.decoder
    g = torch.Generator().manual_seed(5)
    B, L, C = 3, 40, 520
    enc = torch.randn(B, L, C, generator=g).to(DEV)
    dur = torch.randint(1, 6, (B, L), generator=g).to(DEV)
    _, cum, out32 = synth_durations(dur.float(), None, integer_mode=True)
    Tmax = int(out32.max())
    f0, en = torch.rand(B, Tmax, device=DEV), torch.rand(B, Tmax, device=DEV)
    spk = torch.randn(B, 16, device=DEV)
    res = torch.randn(B, 160, Tmax // 2, generator=g).to(DEV)
    a = dec.infer(spk, enc.transpose(1, 2), 1.0, dur=dur, f0=f0, energy_avg=en, residual=res)["mel"]
    ctx = rows_as_context(synth_regulate(enc, cum, out32, Tmax), B, C)
    b = dec.infer_context(spk, ctx, out32.long(), 1.0, f0, en, None, res)["mel"]
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_reconstruct_round_trip():
    import bench
    import radmmm_synth as S
    from rad_mmm_amd.common import SequenceLength
    model, cfg, _ = _joint()
    B, T = 3, 160
    gb = {k: torch.from_numpy(v).to(DEV) for k, v in S.synthetic_batch(B, T, cfg, seed=21, ragged=True).items()}
    batch = bench.build_step_batch(gb, B, T, DEV, t_txt=40)
    with torch.no_grad():
        in_lens = SequenceLength(batch["input_lengths"], batch["input_lengths_host"])
        out_lens = SequenceLength(batch["output_lengths"], batch["output_lengths_host"])
        mel = model.mel_scale(batch["mel"])
        spk = model.encode_speaker(batch["speaker_ids"])
        acc = model.encode_accent(batch["accent_ids"])
        txt_enc, txt_emb = model.encode_text(batch["text"], in_lens.lengths, None, 40)
        attn, *_ = model.compute_attention(mel, txt_emb, spk, acc, out_lens.lengths, in_lens.lengths, batch["attn_prior"],
                                           True, 40)
        context = torch.bmm(txt_enc, attn.squeeze(1).transpose(1, 2))
        z = model.decoder(mel, spk, context, out_lens, f0=batch["f0"], energy_avg=batch["energy_avg"])["z_mel"]
    Tmax = int(batch["output_lengths_host"].max())
    out = model.reconstruct_from_batch_attributes(batch, vocode=False, residual=z[:, :, : Tmax // 2])
    assert torch.equal(out["out_lens"], batch["output_lengths_host"].long())
    for b in range(B):
        n = int(out["out_lens"][b]) // 2 * 2
        e = _rel(out["output_mel"][b, :, :n], batch["mel"][b, :, :n])
        print(f"item {b}: {n} frames, rel {e:.2e}")
        assert e < 1e-4


def test_sample_full_sync_budget():
    model, _, _ = _joint()
    B, L = 32, 150
    text, lens, spk, acc = _text(B, L, 3)
    args = (text.to(DEV), lens, spk.to(DEV))
    kw = dict(accent_ids=acc.to(DEV), vocode=False)
    model.sample_full(*args, **kw)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            model.sample_full(*args, **kw)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    syncs = [f"{x.filename}:{x.lineno}" for x in w if "synchroniz" in str(x.message)]
    print(f"synchronising calls: {len(syncs)}")
    assert len(syncs) <= 1, syncs


def test_sample_full_audio(golden):
    from _vocoder_ref import load_fixture
    from rad_mmm_amd.vocoder import Denoiser, HiFiGANGenerator, vocode
    model, _, _ = _joint()
    vcfg, vsd = load_fixture(golden("vocoder_gen_r2.npz"))
    gen = HiFiGANGenerator(vcfg)
    gen.load_state_dict(vsd)
    gen = gen.to(DEV).eval()
    den = Denoiser(gen).to(DEV)
    model.synth_vocoder = (gen, den)
    text, lens, spk, acc = _text(3, 30, 8)
    out = model.sample_full(text.to(DEV), lens, spk.to(DEV), accent_ids=acc.to(DEV))
    frames = out["out_lens"] // 2 * 2
    assert len(set(frames.tolist())) > 1
    for b, a in enumerate(out["audio"]):
        # each utterance alone, cut to the frames the decoder produced (the batched vocoder is bit-identical per item)
        n = int(frames[b])
        one, s_len = vocode(gen, den, out["mel"][b: b + 1, :, :n].contiguous(), [n], strength=0.001, normalize=True)
        assert a.shape[0] == n * gen.hop == int(s_len[0])
        assert np.array_equal(a, one[0, :n * gen.hop].cpu().numpy())


def test_sample_full_errors():
    model, _, _ = _joint()
    text, lens, spk, acc = _text(2, 12, 4)
    t, s, a = text.to(DEV), spk.to(DEV), acc.to(DEV)
    with pytest.raises(ValueError, match="accent_ids"):
        model.sample_full(t, lens, s, vocode=False)
    with pytest.raises(RuntimeError, match="CPU"):
        model.sample_full(text, lens, s, accent_ids=a, vocode=False)
    with pytest.raises(RuntimeError, match="vocoder"):
        model.sample_full(t, lens, s, accent_ids=a)
    with pytest.raises(ValueError, match="residual"):
        model.sample_full(t, lens, s, accent_ids=a, vocode=False, residual=torch.zeros(2, 160, 1, device=DEV))
    with torch.no_grad():
        model.duration_predictor.feat_pred_fn.dense.bias.fill_(-20.0)          # every token 1 frame
    one = torch.tensor([1, 12])
    with pytest.raises(ValueError, match="utterance 0"):
        model.sample_full(t, one, s, accent_ids=a, vocode=False)
    model.synth_vocoder = (None, None)
    with pytest.raises(ValueError, match="utterance 0 has 2 frames"):
        model.sample_full(t, torch.tensor([2, 12]), s, accent_ids=a)
    model.synth_vocoder = None
    pred = model.energy_predictor
    model.energy_predictor = None
    with pytest.raises(ValueError, match="energy predictor"):
        model.sample_full(t, lens, s, accent_ids=a, vocode=False)
    model.energy_predictor = pred


def test_reconstruct_errors():
    import bench
    import radmmm_synth as S
    model, cfg, _ = _joint()
    B, T = 2, 64
    gb = {k: torch.from_numpy(v).to(DEV) for k, v in S.synthetic_batch(B, T, cfg, seed=2, ragged=True).items()}
    batch = bench.build_step_batch(gb, B, T, DEV, t_txt=12)
    with pytest.raises(RuntimeError, match="vocoder"):
        model.reconstruct_from_batch_attributes(batch)
    with pytest.raises(RuntimeError, match="CPU"):
        model.reconstruct_from_batch_attributes(batch, durations=torch.full((B, 12), 4.0), vocode=False)
    with pytest.raises(ValueError, match="residual"):
        model.reconstruct_from_batch_attributes(batch, vocode=False, residual=torch.zeros(B, 160, 3, device=DEV))
    # a given durations is honoured (the reference ignores the argument)
    out = model.reconstruct_from_batch_attributes(batch, durations=torch.full((B, 12), 3.0, device=DEV), vocode=False)
    assert out["out_lens"].tolist() == [36, 36] and out["output_mel"].shape[2] == 36


# ---------------------------------------------------------------------------------------------------- reference fixture
def test_sample_full_matches_reference_fixture():
    """sample_full against tests/golden/synth_small.npz: the reference's Encoder, ConvLSTMLinearDAP.infer,
    LengthRegulator and RADMMMFlow.infer composed in the order of TTSModel.sample_full (tests/golden/make_golden_synth.py);
    the tolerances of tests/test_infer.py."""
    from test_synthesis_cpu import load_synth_fixture, valid_rel
    from rad_mmm_amd.attribute_predictors import ConvLSTMLinearDAP
    from rad_mmm_amd.decoders import RADMMMFlow
    from rad_mmm_amd.encoder import Encoder
    from rad_mmm_amd.loss import RADMMMLoss
    from rad_mmm_amd.tts_step import TTSTrainingStep
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_synth as G
    t, cfg_kwargs, sd = load_synth_fixture()
    preds = {f"{n}_predictor": ConvLSTMLinearDAP(**G.DAP, **G.PREDICTORS[n]) for n in G.PREDICTORS}
    model = TTSTrainingStep(Encoder(3, G.N_TEXT, 5), RADMMMFlow(use_accent=True, **cfg_kwargs), RADMMMLoss(),
                            n_speakers=G.N_SPK, n_accents=G.N_ACC, n_text_tokens=G.N_TOKENS, n_text_dim=G.N_TEXT,
                            n_speaker_dim=16, n_accent_dim=8, use_accent=True, use_accent_emb_for_decoder=False, **preds)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("attention.") for k in missing), (missing, unexpected)
    model = model.to(DEV).eval()
    d = {k: v.to(DEV) for k, v in t.items()}
    out = model.sample_full(d["text"], t["text_lens"], d["speaker_ids"], accent_ids=d["accent_ids"], f0_mean=d["f0_mean"],
                            f0_std=d["f0_std"], sigma=float(t["sigma"]), residual=d["residual"], vocode=False)
    n = t["out_lens"]
    assert torch.equal(out["out_lens"], n.long())
    assert torch.equal(out["durations"].cpu().long(), t["durations"].long())
    valid = torch.arange(int(n.max()))[None] < n[:, None]
    assert torch.equal(out["voiced"].cpu().bool(), t["voiced"] & valid)
    e_f0, e_en = valid_rel(out["f0"].cpu(), t["f0"], n), valid_rel(out["energy"].cpu(), t["energy"], n)
    e_mel = valid_rel(out["mel"].cpu(), t["mel"], n // 2 * 2)
    print(f"fixture: f0 {e_f0:.2e} energy {e_en:.2e} mel {e_mel:.2e}")
    assert e_f0 < 1e-4 and e_en < 1e-4 and e_mel < 1e-4
