"""CPU checks of the multi-period discriminator's precision "h3" (no GPU): the names, the host-only precision plan, the
automatic gradient scale, the descriptors an "h3" step builds against the host plan queries, the new entry points' binding,
and the inputs tests/test_mpd_h3_gpu.py uses: clear of the kinks, with the conditioning the choice promises (the float32
restatement passes that file's bars on them by construction; this one check needs no "h3" code and would pass without it)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import _mpd_h3_cases as K
import _mpd_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 97), (16, 8192), (32, 8192)]
CONVS = [f"convs.{l}" for l in range(5)] + ["conv_post"]


def _mpd(**kw):
    from rad_mmm_amd.discriminators import MultiPeriodDiscriminator
    return MultiPeriodDiscriminator(**kw)


@pytest.mark.parametrize("name", ["f16", "H3", "", None, 3])
def test_an_unknown_precision_raises_before_anything_else(name, tmp_path):
    from rad_mmm_amd.discriminators import load_mpd
    mpd = _mpd(channels=(4, 8, 16, 16, 16))
    assert mpd.precision == "fp32"
    y = torch.zeros(2, 1, 64)
    with pytest.raises(ValueError, match="precision"):            # before the file is looked at: it does not exist
        load_mpd(str(tmp_path / "no_such_file"), "cpu", precision=name)
    if name is not None:                                          # (None as a per-call argument means the attribute)
        for call in (lambda: mpd(y, y, precision=name), lambda: mpd.discriminator_loss(y, y, precision=name),
                     lambda: mpd.generator_losses(y, y, None, precision=name), lambda: mpd.precision_plan(name)):
            with pytest.raises(ValueError, match="precision"):
                call()
        mpd.precision = name                                      # the attribute: at the next call
        for call in (lambda: mpd(y, y), lambda: mpd.discriminator_loss(y, y), lambda: mpd.generator_losses(y, y), mpd.precision_plan):
            with pytest.raises(ValueError, match="precision"):
                call()
        mpd.precision = "fp32"
        assert mpd.precision_plan()[0]["convs.1"][0] == "fp32"


@pytest.mark.parametrize("name", ["fp32", "h3"])
def test_a_valid_precision_on_cpu_tensors_is_refused_as_before(name):
    from rad_mmm_amd._lib import RadmmmError
    mpd = _mpd(channels=K.CHANNELS)
    y = torch.zeros(2, 1, 64)
    for call in (lambda: mpd(y, y, precision=name), lambda: mpd.discriminator_loss(y, y, precision=name),
                 lambda: mpd.generator_losses(y, y, precision=name)):
        with pytest.raises(RadmmmError, match="GPU tensors"):
            call()
    mpd.precision = name
    with pytest.raises(RadmmmError, match="GPU tensors"):
        mpd(y, y)


def test_the_multi_scale_discriminator_and_the_checkpoint_have_no_mode(tmp_path):
    from rad_mmm_amd.discriminators import MultiScaleDiscriminator, load_mpd
    assert not hasattr(MultiScaleDiscriminator((8, 8, 16, 16, 32, 32, 16), (1, 2, 2, 4, 4, 4, 1)), "precision")
    src = _mpd(channels=K.CHANNELS)
    src.precision = "h3"
    assert not any("precision" in k or "sat" in k or "h3" in k for k in src.state_dict())
    path = tmp_path / "do_00000001"
    torch.save({"mpd": src.state_dict()}, path)
    assert load_mpd(str(path), "cpu", channels=K.CHANNELS).precision == "fp32"
    got = load_mpd(str(path), "cpu", precision="h3", channels=K.CHANNELS)
    assert got.precision == "h3" and all(torch.equal(a, b) for a, b in zip(src.state_dict().values(), got.state_dict().values()))
    assert src.grad_scale is None and src.grad_saturated() is False            # no "h3" call yet: nothing to read


@pytest.mark.parametrize("B,T", SHAPES)
def test_the_plan_at_the_reference_widths(B, T):
    mpd = _mpd()
    plan = mpd.precision_plan("h3", B, T)
    assert len(plan) == 5 and all(list(p) == CONVS for p in plan)
    for p in plan:
        assert all(p[f"convs.{l}"] == ("h3", "") for l in range(1, 5)), p
        assert p["convs.0"][0] == "fp32" and p["convs.0"][1] and p["conv_post"][0] == "fp32" and p["conv_post"][1]
    assert all(m == "fp32" and why for p in mpd.precision_plan(None, B, T) for m, why in p.values())     # the attribute: "fp32"
    mpd.precision = "h3"
    assert mpd.precision_plan(B=B, T=T) == plan and mpd.precision_plan("fp32", B, T) != plan


def test_the_plan_of_narrow_and_odd_widths_is_fp32_with_a_reason():
    for p in _mpd(channels=(4, 8, 16, 16, 16)).precision_plan("h3", 2, 97):
        assert all(m == "fp32" and why for m, why in p.values()), p
    # K = 5 * C_in % 32 (C_in = 48), the data gradient's K = C_out % 32 (C_out = 48): those convs alone fall back
    p = _mpd(channels=(32, 48, 64, 32, 32)).precision_plan("h3", 2, 97)[0]
    assert [p[c][0] for c in CONVS] == ["fp32", "fp32", "fp32", "h3", "h3", "fp32"]
    assert "multiple of 32" in p["convs.1"][1] and "multiple of 32" in p["convs.2"][1]


def test_the_automatic_gradient_scale_is_a_power_of_two_of_host_sizes():
    from rad_mmm_amd.discriminators import _Geometry, auto_grad_scale
    for B, T in SHAPES:
        for p in R.PERIODS:
            s = auto_grad_scale(B, T, p)
            g = _Geometry(p, K.WIDE, B, T, {})
            assert math.frexp(s)[0] == 0.5 and s == g.g_scale
            n_out = B * g.H[4] * p                                 # the adversarial means' normaliser at full lengths
            assert 16 * n_out <= s < 32 * n_out
    assert _Geometry(3, K.WIDE, 2, 97, {"grad_scale": 2.0 ** 20}).g_scale == 2.0 ** 20
    mpd = _mpd(channels=K.CHANNELS)
    mpd.precision, mpd.grad_scale = "h3", 3.0
    with pytest.raises(ValueError, match="power of two"):
        mpd._h3(None)
    mpd.grad_scale = 0.25
    assert mpd._h3(None)["grad_scale"] == 0.25 and mpd._h3("fp32") is None


@pytest.mark.parametrize("B,T", SHAPES)
def test_every_h3_descriptor_is_accepted_by_the_host_plans(B, T):
    """the framed forward GEMMs and the data-gradient GEMMs of a whole walk (all S sequences) and of the generated half (S / 2)
    pass radmmm_rowgemm_h3_plan as three-product launches; the weight gradient's operands meet radmmm_wgrad_rm's conditions;
    the last window of every framed read stays inside its padded sequence"""
    from rad_mmm_amd._lib import lib, rowgemm_h3_plan
    from rad_mmm_amd.discriminators import _WGRAD_RM_ROWS, _Geometry
    for p in R.PERIODS:
        g = _Geometry(p, K.WIDE, B, T, {})
        assert g.mode == ["fp32", "h3", "h3", "h3", "h3", "fp32"]
        for n in (g.S, g.S // 2):
            descs = g.h3_descriptors(n)
            assert len(descs) == 8
            for kw in descs:
                code = rowgemm_h3_plan(nprod=3, **kw)
                assert code > 0 and code // 100 % 10 == 3, (kw, code)
            for l in range(1, 5):
                fwd = descs[2 * (l - 1)]
                C, H, Cin, Hin, st = g.C[l], g.H[l], g.C[l - 1], g.H[l - 1], g.stride[l]
                assert fwd["a_item_stride"] == (Hin + 4) * Cin and fwd["lda_h"] == st * Cin and fwd["K"] == 5 * Cin
                assert st * (H - 1) + 5 <= Hin + 4
                R_ = max(n * H, _WGRAD_RM_ROWS)
                assert C % 8 == 0 and (5 * Cin) % 8 == 0 and R_ >= 32 and R_ * max(C, 5 * Cin) * 2 < 2 ** 31
                assert int(lib.radmmm_wgrad_rm_tiles(C, 5 * Cin, 1)) > 0
                assert int(lib.radmmm_mpdh3_plan(n, Hin, Cin, H, C, st)) == 1


def test_the_framed_descriptor_is_validated_on_the_host():
    from rad_mmm_amd._lib import RadmmmError, rowgemm_h3_plan
    a = 256
    ok = dict(Ah=a, Al=a, Bh=a, Bl=a, C=a, lda_h=96, a_item_stride=37 * 32, ldb_h=160, ldc=64, M=3 * 11, N=64, K=160, T=11, nprod=3)
    assert rowgemm_h3_plan(**ok) > 0
    for bad in (dict(a_item_stride=37 * 32 + 4), dict(taps=3), dict(nprod=2), dict(a_mask_mode=1, lens=a), dict(a_item_stride=-8)):
        with pytest.raises(RadmmmError, match="a_item_stride"):
            rowgemm_h3_plan(**dict(ok, **bad))
    with pytest.raises(RadmmmError, match="ld >= K"):             # without a_item_stride a row must hold K halves
        rowgemm_h3_plan(**dict(ok, a_item_stride=0))


def test_new_entry_points_are_declared_exported_and_bound():
    import rad_mmm_amd._lib as L
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "radmmm_hip.h")).read(), flags=re.S)
    protos = dict(re.findall(r"\b(radmmm_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S))
    raw = ctypes.CDLL(L.LIB_PATH)
    names = {"radmmm_mpdh3_repad": 12, "radmmm_mpdh3_frame": 13, "radmmm_mpdh3_unframe": 17, "radmmm_mpdh3_conv_post_dgrad": 17,
             "radmmm_mpdh3_plan": 6}
    assert {n for n in protos if n.startswith("radmmm_mpdh3_")} == set(names)
    for name, n_args in names.items():
        assert protos[name].count(",") + 1 == n_args, name
        assert hasattr(raw, name) and len(getattr(L.lib, name).argtypes) == n_args, name
    assert L.lib.radmmm_mpdh3_plan(0, 5, 32, 2, 32, 3) == -1 and L.lib.radmmm_mpdh3_plan(4, 5, 32, 4, 32, 3) == -1     # bad dims, windows
    assert L.lib.radmmm_mpdh3_plan(4, 5, 32, 2, 36, 3) == 0 and b"% 8" in L.lib.radmmm_last_error()
    assert L.lib.radmmm_mpdh3_plan(4, 5, 32, 2, 40, 3) == 0 and b"multiple of 32" in L.lib.radmmm_last_error()
    assert L.lib.radmmm_mpdh3_plan(4, 5, 32, 2, 64, 3) == 1


@pytest.mark.parametrize("T,ragged,plain", [(97, True, False), (97, False, False), (64, True, False), (64, True, True)])
def test_the_gpu_tests_inputs_are_clear_of_kinks_and_the_float32_restatement_passes_their_bars(T, ragged, plain):
    c = K.case(T, ragged, plain)
    print(f"T {T} ragged {ragged} plain {plain}: audio seed {c['seed']}, kink ratios {c['kink'][0]:.1f} / {c['kink'][1]:.1f}")
    assert min(c["kink"]) > R.KINK_FACTOR and c["seed"] < K.N_SEEDS
    conds = [R.weight_g_condition(c["sd"], K.case(T, ragged)["w64"]["grad"], f"discriminators.{i}.conv_post.") for i in range(5)]
    print(f"condition numbers of the conv_post.weight_g gradients {[round(v, 1) for v in conds]}")
    assert max(conds) == c["cond"] and (c["cond"] < K.COND_MAX or T == 64)
    w32, w64 = c["w32"], c["w64"]
    lb, gb = K.loss_bars(w32, w64), K.grad_bars(w32, w64)
    assert all(float(np.abs(np.asarray(w32[k]) - np.asarray(w64[k])).max()) <= lb[k] for k in K.LOSSES)
    assert all(R.relative_l2(w32["grad"][k], w64["grad"][k]) <= gb[k] for k in w64["grad"])
    assert R.relative_l2(w32["grad_y"], w64["grad_y"]) <= gb["y"]
    assert all(np.abs(v).max() > 0 for v in w64["grad"].values())
    assert len(w64["grad"]) == (5 * 6 * (2 if plain else 3) + 1)
