"""CPU checks of the mel L1 loss (rad_mmm_amd/mel_loss.py, csrc/mel_loss.hip) without a GPU: the float64 model
tests/_mel_loss_ref.py against the fixtures made by the reference's own TacotronSTFT under torch autograd
(tests/golden/make_golden_mel_loss.py), its framing and unframing, the planted-bug controls (the bars of the GPU comparisons
reject every wrong variant of BUGS in every figure it moves), the silent-stretch case, and the entry points' refusals."""
import numpy as np
import pytest

import _mel_loss_ref as K
from conftest import load_golden


@pytest.fixture(scope="module")
def fixtures():
    out = {}
    for name in K.FIXTURES:
        d = load_golden(f"mel_loss_{name}.npz")
        g = K.fixture_geometry(d)
        out[name] = (d, g, K.mel_loss(*K.fixture_inputs(d), g, d["mel_basis"]))
    return out


def test_fixtures_hold_what_the_generator_promises(fixtures):
    for name, (d, g, got) in fixtures.items():
        assert d["x"].dtype == d["target"].dtype == np.float32 and d["mel_basis"].shape == (g.n_mel, g.cutoff)
        assert float(d["clamp_margin"]) > 100 and float(d["kink_margin"]) > 100, name
        for b, n in enumerate(d.get("lens", [])):
            assert g.h < n <= g.S and not d["x"][b, n:].any()
        assert np.array_equal(got["n"], d["n"]), name
    d, g, _ = fixtures["small"]
    assert (g.n_fft, g.hop, g.win, g.n_mel, g.B, g.S) == (64, 16, 64, 12, 3, 400) and list(d["lens"]) == [400, 333, 33]
    assert d["lens"][2] == g.h + 1 and d["target"].shape == (3, 12, g.F - 1) and list(d["frames"]) == [25, 20, 2]
    assert float(d["melp_min"]) < K.CLIP                         # both sides of the clamp take part
    d, g, _ = fixtures["small_win"]
    assert g.win == 48 < g.n_fft and d["target"].shape == d["x"].shape and "lens" not in d and "grad/t" in d
    d, g, _ = fixtures["shipped"]
    assert (g.n_fft, g.hop, g.win, g.n_mel, g.B, g.S, g.rows) == (1024, 256, 1024, 80, 2, 8192, 66) and g.cutoff % 4 == 1


def test_model_reproduces_the_reference(fixtures):
    """the loss and every gradient of every fixture to 1e-12 relative (L2 for the gradients)"""
    for name, (d, g, got) in fixtures.items():
        want = K.fixture_want(d)
        for k, v in want.items():
            err = abs(got[k] - v) / abs(v) if k == "loss" else K.rel_l2(got[k], v)
            print(f"{name} {k}: model against the reference's float64 {err:.3e}")
            assert err <= 1e-12, (name, k, err)


def test_shipped_mel_basis_is_the_module_s(fixtures):
    from rad_mmm_amd.audio_processing import mel_filterbank
    d, g, _ = fixtures["shipped"]
    assert np.abs(mel_filterbank(22050, 1024, 80, 0.0, 8000.0) - d["mel_basis"]).max() <= 1e-7
    d, g, _ = fixtures["small"]
    assert np.array_equal(mel_filterbank(22050, 64, 12, 0.0, None), d["mel_basis"])


@pytest.mark.parametrize("S,n_fft,hop,lens", [(400, 64, 16, [400, 333, 33]), (100, 32, 1, [100, 17, 64]), (70, 32, 50, [70, 50, 49])])
def test_framing_is_numpy_reflect_pad_plus_strided_frames_per_item(S, n_fft, hop, lens):
    g = K.Geometry(n_fft, hop, n_fft, 4, len(lens), S)
    x = np.random.RandomState(0).randn(g.B, S)
    A = K.frame(x, lens, g).reshape(g.B, g.F, n_fft)
    for b, n in enumerate(lens):
        pad = np.pad(x[b, :n], (g.h, g.h), mode="reflect")
        nf = 1 + n // hop
        assert np.array_equal(A[b, :nf], np.stack([pad[f * hop:f * hop + n_fft] for f in range(nf)])) and not A[b, nf:].any()
    assert np.array_equal(K.frame(x, None, g), K.frame(x, [S] * g.B, g))
    short = K.frame(x, [g.h, 1, 0], g)                          # lens <= h: clamped into the item, finite
    assert np.isfinite(short).all()


@pytest.mark.parametrize("S,n_fft,hop,lens", [(400, 64, 16, [400, 333, 33]), (100, 32, 1, [100, 17, 64]), (70, 32, 12, [70, 50, 17])])
def test_unframe_is_the_exact_adjoint_of_frame(S, n_fft, hop, lens):
    """<frame(x), A> == <x, unframe(A)> exactly on integer data; lens = h + 1 gives samples 1 .. lens-2 both mirrors"""
    g = K.Geometry(n_fft, hop, n_fft, 4, len(lens), S)
    rng = np.random.RandomState(1)
    x = rng.randint(-8, 9, size=(g.B, S)).astype(np.float64)
    A = rng.randint(-8, 9, size=(g.rows, n_fft)).astype(np.float64)
    for ln in (lens, None):
        lhs = float((K.frame(x, ln, g) * A).sum())
        L = K.item_lens(ln, g.B, S)
        xm = x * (np.arange(S)[None, :] < L[:, None])
        assert lhs == float((K.frame(xm, ln, g) * A).sum())      # samples past lens[b] are never read
        for un in (K.unframe, K.unframe_fast):
            u = un(A, ln, g)
            assert lhs == float((x * u).sum()) and not u[np.arange(S)[None, :] >= L[:, None]].any()
        assert np.array_equal(K.unframe(A, ln, g), K.unframe_fast(A, ln, g))
    assert any(n == g.h + 1 for n in lens)
    assert not np.array_equal(K.unframe(A, lens, g), K.unframe(A, lens, g, bug="drop_mirror"))
    assert np.array_equal(K.unframe(A, lens, g, bug="drop_mirror"), K.unframe_fast(A, lens, g, bug="drop_mirror"))


def test_every_gpu_bar_rejects_every_planted_variant_in_every_figure_it_moves(fixtures):
    """A variant `moves` a figure of a fixture when the model with the bug differs from the model without it by more than
    1e-12 relative.  Every such figure must then miss the GPU test's bar for it, and every variant must move something."""
    for bug in K.BUGS:
        moved = []
        for name, (d, g, clean) in fixtures.items():
            bars, want = K.fixture_bars(d), K.fixture_want(d)
            assert set(bars) == set(want)
            bad = K.mel_loss(*K.fixture_inputs(d), g, d["mel_basis"], bug=bug)
            mob = K.measured_over_bar(bad, want, bars)
            for k in bars:
                change = K.measured_over_bar(bad, clean, {k: 1.0})[k]
                if change > 1e-12:
                    moved.append((name, k))
                    print(f"{bug} {name} {k}: moves the figure by {change:.3e}, {mob[k]:.3g} of its bar {bars[k]:.3e}")
                    assert mob[k] > 1.0, (bug, name, k, mob[k])
        assert moved, bug
    for name, (d, g, clean) in fixtures.items():                 # and the model itself passes them
        mob = K.measured_over_bar(clean, K.fixture_want(d), K.fixture_bars(d))
        assert max(mob.values()) < 1e-3, (name, mob)


def test_silent_stretch_gives_a_finite_loss_and_exact_zero_gradient_there():
    """four frames of exact zeros inside a valid item: re = im = 0 in every bin, where the gradient of sqrt is pinned to 0
    (torch gives NaN): the loss is finite, no NaN anywhere, and the samples only those frames hold get exactly 0"""
    g, mb, x, target, lens, frames, (f_lo, f_hi), (s_lo, s_hi) = K.silent_case()
    out = K.mel_loss(x, target, lens, frames, g, mb, exact_order=True)
    rows = slice(0 * g.F + f_lo, 0 * g.F + f_hi)
    assert not out["fx"]["spec"][rows].any() and not out["fx"]["mag"][rows].any()
    assert np.array_equal(out["mel_x"][0, :, f_lo:f_hi], np.full((g.n_mel, f_hi - f_lo), np.log(K.CLIP)))
    assert np.isfinite(out["loss"]) and out["loss"] > 0 and np.isfinite(out["grad_x"]).all()
    assert not out["grad_x"][0, s_lo:s_hi].any() and out["grad_x"][0, :128].any() and out["grad_x"][0, 240:].any()
    assert not out["grad_x"][1, 333:].any()
    fast = K.mel_loss(x, target, lens, frames, g, mb)
    assert K.rel_l2(fast["grad_x"], out["grad_x"]) < 1e-13


def test_empty_loss_is_zero_not_nan():
    g, mb, x, target, lens, _, _, _ = K.silent_case()
    out = K.mel_loss(x, target, lens, np.array([0, -3]), g, mb)
    assert out["loss"] == 0.0 and out["norm"] == 0.0 and not out["grad_x"].any()


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """null pointers, n_fft % 4 != 0, B = 0 and hop = 0 give -1 with a text, before any HIP call: testable without a GPU.
    The stand-in addresses are never dereferenced."""
    from rad_mmm_amd._lib import lib
    err = lib.radmmm_last_error
    d = 0x10000
    B, S, n_fft, hop, n_mel = 2, 400, 64, 16, 12
    F, cutoff, lds, ldm, ldn = 1 + S // hop, 33, 68, 36, 12

    def frame(**k):
        return lib.radmmm_melloss_frame(k.get("x", d), S, None, k.get("A", d), k.get("B", B), S, k.get("F", F), k.get("n_fft", n_fft),
                                        k.get("hop", hop), None)

    def unframe(**k):
        return lib.radmmm_melloss_unframe(k.get("x", d), None, k.get("A", d), S, k.get("B", B), S, k.get("F", F),
                                          k.get("n_fft", n_fft), k.get("hop", hop), 0, None)

    def mag(**k):
        return lib.radmmm_melloss_mag(k.get("x", d), k.get("lds", lds), None, k.get("A", d), k.get("ldm", ldm), k.get("B", B), S,
                                      k.get("F", F), k.get("hop", hop), cutoff, None)

    def dspec(**k):
        return lib.radmmm_melloss_dspec(k.get("x", d), k.get("ldm", ldm), d, k.get("lds", lds), None, k.get("A", d), k.get("B", B),
                                        S, k.get("F", F), k.get("hop", hop), cutoff, None)

    def terms(**k):
        return lib.radmmm_melloss_terms(k.get("x", d), k.get("ldn", ldn), None, None, k.get("t", d), F, None, k.get("A", d),
                                        k.get("B", B), S, k.get("F", F), k.get("hop", hop), n_mel, 1e-5, None)

    def finish(**k):
        return lib.radmmm_melloss_finish(k.get("x", d), None, None, k.get("A", d), d, k.get("B", B), S, k.get("F", F), F,
                                         k.get("hop", hop), n_mel, None)

    def bwd(**k):
        return lib.radmmm_melloss_bwd(k.get("x", d), k.get("ldn", ldn), None, None, k.get("t", d), F, d, k.get("g", d),
                                      k.get("dmel"), k.get("A", d), k.get("B", B), S, k.get("F", F), k.get("hop", hop), n_mel, 1e-5,
                                      None)

    for fn, who in ((frame, b"melloss_frame"), (unframe, b"melloss_unframe"), (mag, b"melloss_mag"), (dspec, b"melloss_dspec"),
                    (terms, b"melloss_terms"), (finish, b"melloss_finish"), (bwd, b"melloss_bwd")):
        for kw in (dict(x=None), dict(A=None)):
            assert fn(**kw) == -1 and err() == who + b": null pointer", (who, kw, err())
        for kw in (dict(B=0), dict(hop=0), dict(B=-1)):
            assert fn(**kw) == -1 and err().startswith(who + b": bad dims"), (who, kw, err())
        assert fn(F=F + 1) == -1 and err().startswith(who + b": F="), (who, err())
    for fn, who in ((frame, b"melloss_frame"), (unframe, b"melloss_unframe")):
        for bad in (66, 62, 0, -64):
            assert fn(n_fft=bad) == -1 and err().startswith(who + b": n_fft="), (who, bad, err())
        assert fn(n_fft=1024) == -1 and b"cannot be reflect-padded" in err()
    for fn, who in ((mag, b"melloss_mag"), (dspec, b"melloss_dspec")):
        assert fn(lds=66) == -1 and err().startswith(who + b": lds=66")
        assert fn(lds=64) == -1 and err().startswith(who + b": lds=64")
        assert fn(ldm=34) == -1 and err().startswith(who + b": ldm=34")
        assert fn(ldm=32) == -1 and err().startswith(who + b": ldm=32")
    for fn, who in ((terms, b"melloss_terms"), (bwd, b"melloss_bwd")):
        assert fn(ldn=14) == -1 and err().startswith(who + b": ldn=14")
        assert fn(ldn=8) == -1 and err().startswith(who + b": ldn=8")
    assert terms(t=None) == -1 and err() == b"melloss_terms: target and part come together"
    assert bwd(dmel=d) == -1 and err() == b"melloss_bwd: exactly one of target and dmel"
    assert bwd(t=None) == -1 and err() == b"melloss_bwd: exactly one of target and dmel"
    assert bwd(g=None) == -1 and err() == b"melloss_bwd: null pointer"
    assert lib.radmmm_melloss_frame(d, S - 1, None, d, B, S, F, n_fft, hop, None) == -1 and err().startswith(b"melloss_frame: ldx=")
    assert lib.radmmm_melloss_frame(d, S, None, d + 4, B, S, F, n_fft, hop, None) == -1 and b"16B aligned" in err()


def test_module_refuses_cpu_tensors_and_carries_the_shipped_default():
    import torch
    from rad_mmm_amd._lib import RadmmmError
    from rad_mmm_amd.audio_processing import TacotronSTFT
    from rad_mmm_amd.mel_loss import MelSpectrogramLoss, mel_spectrogram
    m = MelSpectrogramLoss()
    s = m.stft.stft_fn
    assert (s.filter_length, s.hop_length, s.win_length, m.stft.n_mel_channels, m.stft.sampling_rate) == (1024, 256, 1024, 80, 22050)
    assert sorted(m.state_dict().keys()) == ["stft.mel_basis", "stft.stft_fn.forward_basis"]
    d = load_golden("mel_loss_shipped.npz")
    assert np.abs(m.stft.mel_basis.numpy() - d["mel_basis"]).max() <= 1e-7          # fmax 8000
    small = MelSpectrogramLoss(filter_length=64, hop_length=16, win_length=48, n_mel_channels=12)
    assert small.stft.stft_fn.win_length == 48 and small.stft.mel_basis.shape == (12, 33)
    own = TacotronSTFT(64, 16, 64, 12)
    assert MelSpectrogramLoss(own).stft is own
    with pytest.raises(ValueError, match="not both"):
        MelSpectrogramLoss(own, hop_length=8)
    with pytest.raises(RadmmmError, match="GPU tensors"):
        m(torch.zeros(2, 8192), torch.zeros(2, 80, 33))
    with pytest.raises(RadmmmError, match="GPU tensors"):
        mel_spectrogram(torch.zeros(2, 8192), m.stft)
