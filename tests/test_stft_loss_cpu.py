"""CPU checks of the multi-resolution STFT loss (rad_mmm_amd/stft_loss.py, csrc/stft_loss.hip) without a GPU: the float64
oracle tests/_stft_loss_ref.py against the fixtures made by the reference's own MultiResolutionSTFTLoss
(tests/golden/make_golden_stft_loss.py), its framing and unframing, the package's basis builder, the entry points'
refusals, and the planted-bug controls: the bars of the GPU comparisons reject every wrong variant of BUGS."""
import os

import numpy as np
import pytest

import _stft_loss_ref as K
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixtures():
    out = {}
    for name in K.FIXTURES:
        d = load_golden(f"stft_loss_{name}.npz")
        want = K.multi_resolution(d["x"], d["y"], d.get("len_ratios"), *K.FIXTURE_RES, a_weighting=name.endswith("log1p"))
        out[name] = (d, want)
    return out


@pytest.fixture(scope="module")
def probe():
    """the default-resolution case of the GPU test, with its seed search"""
    return K.probe_case(2, 4096, [4096, 2500], K.DEFAULT_RES)


def test_fixtures_hold_what_the_generator_promises(fixtures):
    for name, (d, want) in fixtures.items():
        assert d["x"].dtype == d["y"].dtype == np.float32 and d["x"].shape == (len(d["lengths"]), 600)
        for b, n in enumerate(d["lengths"]):
            assert not d["x"][b, n:].any() and not d["y"][b, n:].any()
        assert float(d["clamp_margin"]) > 1e-3 and float(d["dlog_min"]) > 8 * float(d["dlog_dev"])
        cm, dm = K.kink_margins(want["res"])
        assert cm == pytest.approx(float(d["clamp_margin"]), rel=1e-6) and dm == pytest.approx(float(d["dlog_min"]), rel=1e-6)
        assert ("len_ratios" in d) == name.startswith("ragged")
        assert list(d["state_dict_keys"]) == [f"stft_losses.{i}.window" for i in range(3)]


def test_oracle_reproduces_the_reference(fixtures):
    """losses and the four gradients of every fixture to 1e-10 relative"""
    for name, (d, want) in fixtures.items():
        for k in K.LOSS_KEYS:
            assert abs(want[k] - float(d[k + "64"])) <= 1e-10 * abs(float(d[k + "64"])), (name, k)
        for k in K.GRAD_KEYS:
            assert K.rel_l2(want[k], d["grad/" + k]) <= 1e-10, (name, k)


@pytest.mark.parametrize("T,n_fft,hop,win", [(600, 64, 12, 40), (33, 64, 5, 39), (100, 32, 1, 32), (17, 32, 50, 7)])
def test_framing_is_numpy_reflect_pad_plus_strided_frames(T, n_fft, hop, win):
    x = np.random.RandomState(0).randn(2, T)
    left = (n_fft - win) // 2
    pad = np.pad(x, ((0, 0), (n_fft // 2, n_fft // 2)), mode="reflect")
    F = 1 + T // hop
    want = np.stack([pad[:, f * hop + left:f * hop + left + win] for f in range(F)], 1).reshape(2 * F, win)
    assert np.array_equal(K.frame(x, None, n_fft, hop, win), want)
    frames = np.array([F, 1])
    got = K.frame(x, frames, n_fft, hop, win, ldk=win + 3).reshape(2, F, win + 3)
    assert np.array_equal(got[0, :, :win], want.reshape(2, F, win)[0]) and not got[1, 1:].any() and not got[:, :, win:].any()


@pytest.mark.parametrize("T,n_fft,hop,win", [(33, 64, 5, 39), (17, 32, 1, 32), (40, 32, 12, 16), (600, 64, 12, 40)])
def test_unframe_is_the_exact_adjoint_of_frame(T, n_fft, hop, win):
    """<frame(x), A> == <x, unframe(A)> exactly on integer data; T = n_fft/2 + 1 gives sample 1 .. T-2 both mirrors"""
    rng = np.random.RandomState(1)
    F = 1 + T // hop
    x = rng.randint(-8, 9, size=(3, T)).astype(np.float64)
    A = rng.randint(-8, 9, size=(3 * F, win)).astype(np.float64)
    for frames in (None, np.array([F, 1, 0]), np.array([F // 2 + 1, F, 2])):
        lhs = float((K.frame(x, frames, n_fft, hop, win) * A).sum())
        for un in (K.unframe, K.unframe_fast):
            assert lhs == float((x * un(A, frames, T, n_fft, hop, win)).sum())
        assert np.array_equal(K.unframe(A, frames, T, n_fft, hop, win), K.unframe_fast(A, frames, T, n_fft, hop, win))
    if T == n_fft // 2 + 1:
        h = n_fft // 2
        assert all(1 <= s <= h and T - 1 - h <= s <= T - 2 for s in range(1, T - 1))
    assert not np.array_equal(K.unframe(A, None, T, n_fft, hop, win), K.unframe(A, None, T, n_fft, hop, win, bug="drop_mirror"))


@pytest.mark.parametrize("n_fft,win", [(64, 40), (128, 100), (32, 16), (64, 39), (1024, 600), (512, 240)])
def test_basis_builder_is_the_float64_windowed_dft_on_the_support(n_fft, win):
    from rad_mmm_amd.audio_processing import windowed_dft_basis
    from rad_mmm_amd.stft_loss import stft_loss_basis
    got = stft_loss_basis(n_fft, win)
    cutoff, left = n_fft // 2 + 1, (n_fft - win) // 2
    assert got.dtype == np.float32 and got.shape == (2 * cutoff, (win + 3) // 4 * 4) and not got[:, win:].any()
    bre, bim = K.basis64(n_fft, win)
    want = np.vstack([bre, bim])
    assert np.array_equal(got[:, :win], want.astype(np.float32))          # float64, rounded once
    eye = np.eye(n_fft)[left:left + win]                                    # the DFT of unit impulses on the support
    full = np.fft.fft(eye * K.reference_window(win)[:, None], axis=1)[:, :cutoff].T
    assert np.abs(want - np.vstack([full.real, full.imag])).max() < 1e-12
    # and the package's full-width fp32 basis restricted to the support, to its own rounding (two fp32 products)
    assert np.abs(got[:, :win] - windowed_dft_basis(n_fft, win)[:, left:left + win]).max() < 4e-7


def test_identical_arguments_give_exact_zeros(fixtures):
    d, _ = fixtures["ragged_log"]
    for lr in (d["len_ratios"], None):
        for a_w in (False, True):
            o = K.multi_resolution(d["x"], d["x"], lr, *K.FIXTURE_RES, a_weighting=a_w)
            assert o["sc"] == 0.0 and o["mag"] == 0.0
            for k in K.GRAD_KEYS:
                assert np.isfinite(o[k]).all() and not o[k].any(), k


def test_module_refuses_what_it_cannot_run():
    import torch
    from rad_mmm_amd._lib import RadmmmError
    from rad_mmm_amd.stft_loss import MultiResolutionSTFTLoss, STFTLoss
    with pytest.raises(ValueError, match="hann_window"):
        MultiResolutionSTFTLoss(window="hamming_window")
    with pytest.raises(ValueError):
        STFTLoss(fft_size=64, win_length=65)
    m = MultiResolutionSTFTLoss()
    assert list(m.state_dict().keys()) == [f"stft_losses.{i}.window" for i in range(3)]
    assert torch.equal(m.stft_losses[2].window, torch.hann_window(240))
    with pytest.raises(RadmmmError, match="GPU"):
        m(torch.zeros(2, 4096), torch.zeros(2, 4096))


def test_entry_points_refuse_before_any_hip_call():
    import rad_mmm_amd._lib as L
    lib = L.lib
    d = 0x10000                                                   # never dereferenced
    err = lib.radmmm_last_error

    def frame(x=d, A=d, ldk=40, T=600, F=51, n_fft=64, hop=12, win=40):
        return lib.radmmm_stftloss_frame(x, T, None, A, ldk, 2, T, F, n_fft, hop, win, None)

    def unframe(dA=d, dx=d, ldk=40, T=600, F=51, n_fft=64, hop=12, win=40):
        return lib.radmmm_stftloss_unframe(dA, ldk, None, dx, T, 2, T, F, n_fft, hop, win, 0, None)

    for fn, who in ((frame, b"stftloss_frame"), (unframe, b"stftloss_unframe")):
        first, second = ("x", "A") if fn is frame else ("dA", "dx")
        for kw in ({first: None}, {second: None}):
            assert fn(**kw) == -1 and err() == who + b": null pointer"
        assert fn(T=32, F=3) == -1 and err().startswith(who + b": T=32 cannot be reflect-padded")
        assert fn(win=65, ldk=68) == -1 and err().startswith(who + b": win=65 exceeds n_fft=64")
        assert fn(ldk=42) == -1 and err().startswith(who + b": ldk=42 must be a multiple of 4")
        assert fn(ldk=36) == -1 and err().startswith(who + b": ldk=36")
        assert fn(F=52) == -1 and b"at most 1 + T / hop" in err()
        assert fn(hop=0) == -1 and b"bad dims" in err()
    assert lib.radmmm_stftloss_terms(None, d, 68, None, d, 2, 51, 33, 0, None) == -1 and err() == b"stftloss_terms: null pointer"
    assert lib.radmmm_stftloss_terms(d, d, 68, None, None, 2, 51, 33, 0, None) == -1 and err() == b"stftloss_terms: null pointer"
    assert lib.radmmm_stftloss_terms(d, d, 66, None, d, 2, 51, 33, 0, None) == -1 and err().startswith(b"stftloss_terms: lds=66")
    assert lib.radmmm_stftloss_terms(d, d, 64, None, d, 2, 51, 33, 0, None) == -1 and err().startswith(b"stftloss_terms: lds=64")
    assert lib.radmmm_stftloss_finish(d, None, None, d, 2, 51, 33, None) == -1 and err() == b"stftloss_finish: null pointer"
    assert lib.radmmm_stftloss_finish(d, None, d, d, 0, 51, 33, None) == -1 and err().startswith(b"stftloss_finish: bad dims")
    bwd = lambda **k: lib.radmmm_stftloss_bwd(k.get("sx", d), d, k.get("lds", 68), d, d, None, k.get("g", d), d, 1.0,  # noqa: E731
                                              k.get("dx", d), k.get("dy", d), 2, 51, 33, 0, None)
    for kw in (dict(sx=None), dict(g=None), dict(dx=None, dy=None)):
        assert bwd(**kw) == -1 and err() == b"stftloss_bwd: null pointer"
    assert bwd(lds=70) == -1 and err().startswith(b"stftloss_bwd: lds=70")
    assert lib.radmmm_stftloss_frame(d, 1 << 20, None, d, 2048, 64, 1 << 20, (1 << 20) + 1, 2048, 1, 2048, None) == -1
    assert b"exceeds 2 GiB" in err()


def _worst(got, want, bars):
    return max(K.measured_over_bar(got, want, bars).values())


INVISIBLE_IN_FIXTURES = ("sqrt_clamp", "clamp_grad")


@pytest.mark.parametrize("bug", K.BUGS)
def test_fixture_bars_reject_the_planted_bug(fixtures, bug):
    """The fixture comparison of the GPU test, with its own bars, fails for the wrong variant on at least one fixture.
    The two clamp variants are the exception, and the reason is pinned here: the fixtures' signals are zero past each
    length in x AND y, so no valid frame holds a bin that is below the clamp in one signal and live in the other, and
    both variants then compute what the right code computes; the oracle comparison below covers them."""
    worst = {}
    for name, (d, want) in fixtures.items():
        got = K.multi_resolution(d["x"], d["y"], d.get("len_ratios"), *K.FIXTURE_RES, a_weighting=name.endswith("log1p"), bug=bug)
        ref = {k: float(d[k + "64"]) for k in K.LOSS_KEYS}
        ref.update({k: d["grad/" + k] for k in K.GRAD_KEYS})
        worst[name] = _worst(got, ref, K.fixture_bars(d))
    if bug in INVISIBLE_IN_FIXTURES:
        for name, (d, want) in fixtures.items():
            for r in want["res"]:
                ok = r["valid"] > 0
                assert not ((r["p_x"][ok] < K.CLAMP) ^ (r["p_y"][ok] < K.CLAMP)).any()
        assert max(worst.values()) < 1e-3
    else:
        assert max(worst.values()) > 10, worst


def test_right_variant_passes_its_own_bars(fixtures, probe):
    for name, (d, want) in fixtures.items():
        ref = {k: float(d[k + "64"]) for k in K.LOSS_KEYS}
        ref.update({k: d["grad/" + k] for k in K.GRAD_KEYS})
        assert _worst(want, ref, K.fixture_bars(d)) < 1e-3
    x, y, ratios, want, seed, (cm, dm) = probe
    assert cm > K.DIRECT_KINK_FACTOR and dm > K.DIRECT_KINK_FACTOR
    sub = sum(int(((r["p_x"][r["valid"] > 0] < K.CLAMP) & (r["p_y"][r["valid"] > 0] >= K.CLAMP)).sum()) for r in want["res"])
    assert sub > 100                                              # the quiet stretch: bins below the clamp in x only


# which figures a wrong variant moves at all in the default-resolution case (the others it leaves bit-equal or within 1e-6 of
# a bar): each of these must be rejected on that very figure, by its own bar, in both forms
MOVES = {"left0": K.LOSS_KEYS + K.GRAD_KEYS, "reflectT": K.LOSS_KEYS + K.GRAD_KEYS, "floor": K.LOSS_KEYS + K.GRAD_KEYS,
         "denomBF": K.LOSS_KEYS + K.GRAD_KEYS, "sqrt_clamp": ("sc", "mag", "sc_x", "mag_x"),
         "global_norm": ("sc", "sc_x", "sc_y"), "drop_mirror": K.GRAD_KEYS, "clamp_grad": ("sc_x", "mag_x")}


@pytest.mark.parametrize("a_w", [False, True])
@pytest.mark.parametrize("bug", K.BUGS)
def test_oracle_bars_reject_the_planted_bug(probe, bug, a_w):
    """the default-resolution comparisons of the GPU test fail for every wrong variant ON EVERY FIGURE the variant moves:
    1e-6 losses and 1e-5 gradients against this oracle, and in the log form the derived bars of log_gradient_fp32_bars for
    the two log-magnitude gradients; the generator-step comparison uses the same oracle at the fixture resolutions"""
    x, y, ratios, want, seed, _ = probe
    bars = dict(K.ORACLE_BARS_LOG, **K.log_gradient_fp32_bars(want))
    if a_w:
        want, bars = K.multi_resolution(x, y, ratios, *K.DEFAULT_RES, a_weighting=True), K.ORACLE_BARS
    got = K.multi_resolution(x, y, ratios, *K.DEFAULT_RES, a_weighting=a_w, bug=bug)
    mob = K.measured_over_bar(got, want, bars)
    assert set(mob) == set(K.LOSS_KEYS + K.GRAD_KEYS)
    for k, v in mob.items():
        assert (v > 2.0) == (k in MOVES[bug]), (k, v)


def test_derived_log_gradient_bars_of_the_probe(probe):
    x, y, ratios, want, seed, (cm, dm) = probe
    bars = K.log_gradient_fp32_bars(want)
    print(seed, cm, dm, bars)
    assert cm > K.DIRECT_KINK_FACTOR and dm > K.DIRECT_KINK_FACTOR
    assert all(1e-5 <= v < K.PROBE_BAR_CAP for v in bars.values())


def test_log_form_gradients_are_beyond_fp32_at_the_default_resolutions(probe):
    """why the log form's two log-magnitude gradients take a derived bar there: stock float32 arithmetic on the CPU
    deviates from float64 by more than 1e-5 on the very signals, and by less than 1e-5 in the log(1 + m) form"""
    x, y, ratios, want, seed, _ = probe
    log = K.stock_fp32_deviation(x, y, ratios, K.DEFAULT_RES)
    log1p = K.stock_fp32_deviation(x, y, ratios, K.DEFAULT_RES, a_weighting=True)
    print(log, log1p)
    assert min(log.values()) > 1e-5 and max(log1p.values()) < 5e-6
