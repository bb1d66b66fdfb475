"""CPU checks of the grouped strided convolution's entry points (csrc/msd.hip): every refusal returns -1 with its text
before any HIP call (there is no GPU here, so a call that reached the runtime would fail differently), and the split count
of the weight gradient is the documented function of the shape."""
import pytest

D = 0x1000            # a non-null, 16-byte aligned address that a refused call never dereferences
REF = [(4, 32, 32, 2), (16, 8, 16, 2), (16, 16, 32, 4), (16, 32, 64, 4), (16, 64, 64, 1)]


def _lib():
    from rad_mmm_amd._lib import lib
    return lib


def _fwd(lib, X=D, W=D, b=D, Y=D, S=2, Hin=9, Hout=None, G=2, ci=8, co=8, k=41, st=2, po=20):
    Hout = (Hin - 1) // st + 1 if Hout is None and st > 0 else Hout
    return lib.radmmm_msd_gconv_fwd(X, W, b, Y, S, Hin, Hout, G, ci, co, k, st, po, 0.1, None)


def _dgrad(lib, dY=D, W=D, add=None, X=D, dX=D, S=2, Hin=9, Hout=None, G=2, ci=8, co=8, k=41, st=2):
    Hout = (Hin - 1) // st + 1 if Hout is None and st > 0 else Hout
    return lib.radmmm_msd_gconv_dgrad(dY, W, add, X, dX, S, Hin, Hout, G, ci, co, k, st, 0.1, None)


def _wgrad(lib, dZ=D, X=D, P=D, S=2, Hin=9, Hout=None, G=2, ci=8, co=8, k=41, st=2):
    Hout = (Hin - 1) // st + 1 if Hout is None and st > 0 else Hout
    return lib.radmmm_msd_gconv_wgrad(dZ, X, P, S, Hin, Hout, G, ci, co, k, st, None)


@pytest.mark.parametrize("call,name,ptrs", [(_fwd, "msd_gconv_fwd", ("X", "W", "b", "Y")),
                                            (_dgrad, "msd_gconv_dgrad", ("dY", "W", "X", "dX")),
                                            (_wgrad, "msd_gconv_wgrad", ("dZ", "X", "P"))])
def test_refusals_come_before_any_hip_call(call, name, ptrs):
    lib = _lib()

    def refused(text, **kw):
        assert call(lib, **kw) == -1, kw
        msg = lib.radmmm_last_error().decode()
        assert msg.startswith(name + ": ") and text in msg, (kw, msg)

    for p in ptrs:
        refused("null pointer", **{p: None})
    refused("Cin_g and Cout_g must be multiples of 4", ci=6)
    refused("Cin_g and Cout_g must be multiples of 4", co=6)
    refused("Cin_g and Cout_g must be multiples of 4", ci=68)
    refused("Cin_g and Cout_g must be multiples of 4", co=0)
    refused("stride must be 1, 2 or 4", st=3)
    refused("stride must be 1, 2 or 4", st=0, Hout=5)
    refused("k must be odd and at most 41", k=42)
    refused("k must be odd and at most 41", k=43)
    refused("k must be odd and at most 41", k=0)
    refused("bad dims", S=0)
    refused("bad dims", G=0)
    refused("bad dims", Hin=0, Hout=1)
    refused("does not belong to", Hout=4)
    refused("exceeds 2 GiB", S=64, Hin=1 << 20, G=16, ci=64, co=64, st=1)
    if call is _fwd:
        refused("pad_out must lie in [0, 20]", po=21)
        refused("pad_out must lie in [0, 20]", po=-1)
        refused("16B alignment", X=D + 4)
    if call is _dgrad:
        refused("16B alignment", dY=D + 8)
    if call is _wgrad:
        refused("16B alignment", X=D + 4)


def test_weight_gradient_split_count():
    """n = min(units, 64, max(1, 1024 // (G * ceil(k / 4)))), units = S * ceil(Hout / 32); 0 for a shape that is none"""
    lib = _lib()
    for S, Hout in ((3, 1), (3, 66), (4, 49), (64, 4096), (1, 33)):
        for G, _, _, _ in REF + [(1, 4, 4, 1), (2, 4, 4, 2)]:
            for k in (1, 5, 41):
                units = S * -(-Hout // 32)
                want = max(1, min(units, 64, 1024 // (G * -(-k // 4))))
                assert lib.radmmm_msd_gconv_wgrad_splits(S, Hout, G, k) == want
    assert lib.radmmm_msd_gconv_wgrad_splits(0, 5, 1, 5) == 0


# ---- the float64 restatement (tests/_msd_ref.py) against the reference's own figures (tests/golden/msd_*.npz) --------------
import numpy as np
import torch

import _msd_ref as R

FIXTURES = ("t97", "t64")
KEYS = ("fm", "gen", "disc", "r_losses", "g_losses")


def _sd(d):
    return {k[3:]: d[k] for k in d if k.startswith("sd/")}


@pytest.fixture(scope="module", params=FIXTURES)
def fx(request, golden):
    d = golden(f"msd_{request.param}.npz")
    sd = _sd(d)
    return dict(name=request.param, d=d, sd=sd, w64=R.run(sd, d["y"], d["y_hat"], torch.from_numpy(d["len_ratios"])))


def test_fixture_shapes_and_kink_condition(fx):
    d = fx["d"]
    B, T = {"t97": (2, 97), "t64": (3, 64)}[fx["name"]]
    assert d["y"].shape == d["y_hat"].shape == (B, 1, T) and d["len_ratios"].dtype == np.float32
    assert float(d["kink_min_abs"]) > R.KINK_FACTOR * float(d["kink_max_dev"])
    assert float(d["diff_min_abs"]) > R.KINK_FACTOR * float(d["diff_max_dev"])
    lens = [T, T // 2 + 1, (T // 2 + 1) // 2 + 1]
    for i, t in enumerate(lens):
        h = t
        for st in R.STRIDES[:7]:
            h = (h - 1) // st + 1
        assert d[f"out_r/{i}"].shape == (B, h)
    assert sum(k.startswith("sd_after/") for k in d) == 16


def test_restatement_reproduces_the_reference(fx):
    """float64 figures to 1e-12 relative, those stored as float32 to half a float32 ulp, the power-iteration vectors after the
    call to float64 rounding"""
    d, w = fx["d"], fx["w64"]
    for k in KEYS:
        err = float(np.abs(np.asarray(w[k]) - d[k + "64"]).max() / np.abs(d[k + "64"]).max())
        print(f"{fx['name']} {k}: {err:.2e}")
        assert err <= 1e-12, k
    half_ulp = 2.0 ** -24 * (1 + 1e-6)
    for i in range(3):
        for got, key in ((w["out_r"][i], f"out_r/{i}"), (w["out_g"][i], f"out_g/{i}")):
            assert (np.abs(got - d[key]) <= half_ulp * np.abs(got) + 1e-45).all(), key
    names = [k[5:] for k in d if k.startswith("grad/")]
    assert set(names) == set(w["grad"])
    for k in names:
        got = w["grad"][k]
        tol = half_ulp * np.abs(got) + 1e-12 * np.abs(got).max() + 2.0 ** -150
        assert (np.abs(got - d["grad/" + k]) <= tol).all(), k
    for k in (k for k in d if k.startswith("sd_after/")):
        got = w["after"][k[9:]]
        assert np.abs(got - d[k]).max() <= 1e-14, k
        assert got.size == 1 or np.abs(got - fx["sd"][k[9:]]).max() > 1e-4, k      # the call moved it (a 1-vector stays 1)


def test_float32_restatement_deviates_as_the_reference_does(fx):
    """the restatement's float32 run stays within 10 x the reference's own float32 deviation (the bar of the GPU tests): the
    bars measured from it elsewhere are of the right size"""
    d = fx["d"]
    w32 = R.run(fx["sd"], d["y"], d["y_hat"], torch.from_numpy(d["len_ratios"]), torch.float32)
    for k in w32["grad"]:
        dev = R.relative_l2(w32["grad"][k], fx["w64"]["grad"][k])
        assert dev <= max(10 * float(d["f32_vs_f64/" + k]), 1e-6), (k, dev)


FLAWS = ("same_weight", "pool_divisor", "pool_length", "groups_transposed", "stride_1", "pad_2", "slope_001", "floor",
         "no_channels", "factor_2")


@pytest.mark.parametrize("flaw", FLAWS)
def test_planted_errors_miss_the_bars(fx, flaw):
    """each planted error moves some loss or some gradient by far more than the GPU tests' bar on it; printed: the factor"""
    d, w = fx["d"], fx["w64"]
    bad = R.run(fx["sd"], d["y"], d["y_hat"], torch.from_numpy(d["len_ratios"]), flaw=flaw)
    worst = 0.0
    for k in KEYS:
        bar = max(10 * float(np.abs(d[k + "32"] - d[k + "64"]).max()), 1e-6 * float(np.abs(d[k + "64"]).max()))
        worst = max(worst, float(np.abs(np.asarray(bad[k]) - np.asarray(w[k])).max()) / bar)
    for k in w["grad"]:
        if bad["grad"][k].shape == w["grad"][k].shape:
            worst = max(worst, R.relative_l2(bad["grad"][k], w["grad"][k]) / max(10 * float(d["f32_vs_f64/" + k]), 1e-6))
    print(f"{fx['name']} {flaw}: misses a bar by a factor of {worst:.3g}")
    assert worst > 100, (flaw, worst)


def test_one_power_iteration_and_early_sigma_are_told_apart(fx):
    """one power iteration instead of two leaves other vectors behind than sd_after; sigma taken from the vectors before the
    update gives other losses"""
    d, w = fx["d"], fx["w64"]
    lr = torch.from_numpy(d["len_ratios"])
    one = R.run(fx["sd"], d["y"], d["y_hat"], lr, flaw="one_iteration")
    dev = max(float(np.abs(one["after"][k[9:]] - d[k]).max()) for k in d if k.startswith("sd_after/"))
    print(f"{fx['name']} one_iteration: vectors off by {dev:.3e}")
    assert dev > 1e-3
    early = R.run(fx["sd"], d["y"], d["y_hat"], lr, flaw="sigma_before_update")
    bar = max(10 * abs(float(d["disc32"]) - float(d["disc64"])), 1e-6 * float(d["disc64"]))
    print(f"{fx['name']} sigma_before_update: disc off by {abs(early['disc'] - w['disc']) / bar:.3g} bars")
    assert abs(early["disc"] - w["disc"]) > 100 * bar


def test_state_dict_keys_are_the_references(golden, tmp_path):
    from rad_mmm_amd.discriminators import DiscriminatorP, MultiScaleDiscriminator, load_msd
    d = golden("msd_t97.npz")
    msd = MultiScaleDiscriminator()
    sd = msd.state_dict()
    assert list(sd.keys()) == [str(k) for k in d["default_keys"]]
    assert [",".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in d["default_shapes"]]
    path = tmp_path / "do_1"
    torch.save({"msd": sd, "mpd": {}}, path)
    back = load_msd(str(path), device="cpu")
    for k, v in back.state_dict().items():
        assert torch.equal(v, sd[k]), k
    with pytest.raises(KeyError):
        torch.save({"mpd": {}}, path)
        load_msd(str(path), device="cpu")
    narrow = MultiScaleDiscriminator(tuple(int(c) for c in d["widths"]), tuple(int(g) for g in d["groups"]))
    narrow.load_state_dict({k: torch.as_tensor(v) for k, v in _sd(d).items()})
    narrow.remove_weight_norm()
    keys = list(narrow.state_dict().keys())
    assert "discriminators.0.convs.1.weight_orig" in keys and "discriminators.1.convs.1.weight" in keys
    narrow.apply_weight_norm()
    assert list(narrow.state_dict().keys()) == list(_sd(d).keys())
    with pytest.raises(NotImplementedError):
        DiscriminatorP(2, use_spectral_norm=True)
    with pytest.raises(ValueError):
        MultiScaleDiscriminator((8, 8, 16, 16, 32, 32, 16), (1, 2, 4, 4, 4, 4, 1))        # convs.2 would have 2 channels per group


def test_fold_spectral_norm_is_torchs(golden):
    """fold_spectral_norm against torch.nn.utils.spectral_norm's own module call, training (two calls) and eval, CPU float32:
    same weights to the bit, same buffers"""
    from rad_mmm_amd.discriminators import fold_spectral_norm
    torch.manual_seed(3)
    conv = torch.nn.utils.spectral_norm(torch.nn.Conv1d(8, 16, 41, 2, groups=2, padding=20))
    w0, u, v = conv.weight_orig.detach().clone(), conv.weight_u.clone(), conv.weight_v.clone()
    x = torch.randn(2, 8, 30)
    for training in (True, True, False):
        conv.train(training)
        conv(x)
        w = fold_spectral_norm(w0, u, v, training)
        assert torch.equal(w, conv.weight.detach()) and torch.equal(u, conv.weight_u) and torch.equal(v, conv.weight_v)
    w0.requires_grad_(True)
    fold_spectral_norm(w0, u, v, True).square().sum().backward()
    conv.train()
    conv(x)
    conv.weight.square().sum().backward()
    assert torch.allclose(w0.grad, conv.weight_orig.grad, rtol=1e-6, atol=1e-9)


def test_support_entry_points_refuse_before_any_hip_call():
    lib = _lib()

    def refused(rc, text):
        assert rc == -1
        assert text in lib.radmmm_last_error().decode(), lib.radmmm_last_error()

    refused(lib.radmmm_msd_avgpool(None, D, 8, D, 2, 8, None), "msd_avgpool: null pointer")
    refused(lib.radmmm_msd_avgpool(D, D, 7, D, 2, 8, None), "msd_avgpool: bad dims")
    refused(lib.radmmm_msd_avgpool_bwd(D, None, 8, 2, 8, None), "msd_avgpool_bwd: null pointer")
    refused(lib.radmmm_msd_avgpool_bwd(D, D, 8, 0, 8, None), "msd_avgpool_bwd: bad dims")
    refused(lib.radmmm_msd_frame15(D, None, 8, D, 2, 8, None), "msd_frame15: null pointer")
    refused(lib.radmmm_msd_frame15(D, D, 1 << 26, D, 4, 1 << 26, None), "msd_frame15: the frame matrix exceeds 2 GiB")
    refused(lib.radmmm_msd_unframe15(None, D, 8, 2, 8, None), "msd_unframe15: null pointer")
    refused(lib.radmmm_msd_unframe15(D, D, 7, 2, 8, None), "msd_unframe15: bad dims")
    refused(lib.radmmm_msd_repad(D, 8, None, 2, 8, 8, 20, 0.1, None), "msd_repad: null pointer")
    refused(lib.radmmm_msd_repad(D, 8, D, 2, 8, 6, 20, 0.1, None), "msd_repad: bad dims")
    refused(lib.radmmm_msd_repad(D, 8, D, 2, 8, 8, 21, 0.1, None), "msd_repad: bad dims")
    refused(lib.radmmm_msd_repad(D, 6, D, 2, 8, 8, 2, 0.1, None), "msd_repad: 16B alignment")
    refused(lib.radmmm_msd_fm_terms(None, None, D, 2, 8, 8, 20, None), "msd_fm_terms: null pointer")
    refused(lib.radmmm_msd_fm_terms(D, None, D, 2, 8, 6, 20, None), "msd_fm_terms: a padded map needs C % 4 == 0")
    refused(lib.radmmm_msd_fm_terms(D, None, D, 2, 8, 8, 21, None), "msd_fm_terms: pad must lie in [0, 20]")
    refused(lib.radmmm_msd_fm_terms(D, None, D, 2, 8, 4, -1, None), "the dense output C == 1")
    refused(lib.radmmm_msd_fm_grad(D, None, None, D, D, 2, 8, 8, 20, None), "msd_fm_grad: null pointer")
    refused(lib.radmmm_msd_finish(D, None, None, None, D, None, D, D, 2, None), "msd_finish: null pointer")
    refused(lib.radmmm_msd_out_grad(D, None, D, D, None, 2, 8, None), "msd_out_grad: null pointer")
    refused(lib.radmmm_msd_out_grad(D, None, D, D, D, 2, 0, None), "msd_out_grad: bad dims")
    # the multi-period entry points keep their texts
    refused(lib.radmmm_mpd_fm_terms(None, None, D, 2, 2, 8, 8, 1, None), "mpd_fm_terms: null pointer")
    refused(lib.radmmm_mpd_finish(D, None, None, None, D, None, D, D, 2, 2, None), "mpd_finish: null pointer")


def test_dense_descriptors_have_a_plan_at_the_reference_widths():
    """every row GEMM and dense weight gradient the module builds at the reference's widths is one the fp32 family accepts:
    the first conv (K = 16), the framed 5-tap conv, both data gradients, the two weight gradients"""
    from rad_mmm_amd._lib import rowgemm_plan, wgrad_plan
    A = 0x10000
    C0, C5, C6 = 128, 1024, 1024
    for B, T in ((2, 97), (16, 8192), (32, 8192)):
        for t in (T, T // 2 + 1, (T // 2 + 1) // 2 + 1):
            Sq = 2 * B
            h = t
            for st in R.STRIDES[:6]:
                h = (h - 1) // st + 1
            R0, R6 = Sq * t, Sq * h
            assert rowgemm_plan(A=A, lda=16, B=A, ldb=16, C=A, ldc=C0, M=R0, N=C0, K=16, T=t, bias=A) > 0
            assert rowgemm_plan(A=A, lda=C5, a_item_stride=(h + 4) * C5, B=A, ldb=5 * C5, C=A, ldc=C6, M=R6, N=C6, K=5 * C5, T=h,
                                bias=A) > 0
            assert rowgemm_plan(A=A, lda=C6, B=A, ldb=5 * C5, b_layout=1, C=A, ldc=5 * C5, M=R6, N=5 * C5, K=C6, T=h) > 0
            assert rowgemm_plan(A=A, lda=C0, B=A, ldb=16, b_layout=1, C=A, ldc=16, M=R0, N=16, K=C0, T=t) > 0
            assert wgrad_plan(GY=A, ldgy=C6, X=A, ldx=5 * C5, P=A, ldp=5 * C5, split_stride=C6 * 5 * C5, R=R6, Mc=C6, Nc=5 * C5,
                              taps=1, dil=1, T=R6, splits=1) > 0
            assert wgrad_plan(GY=A, ldgy=C0, X=A, ldx=16, P=A, ldp=16, split_stride=C0 * 16, R=R0, Mc=C0, Nc=16, taps=1, dil=1,
                              T=R0, splits=1) > 0
