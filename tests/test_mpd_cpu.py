"""CPU checks of the multi-period discriminator (no GPU): the float64 restatement tests/_mpd_ref.py reproduces what the
reference's own code computed (tests/golden/mpd_t97.npz / mpd_t64.npz, written by tests/golden/make_golden_mpd.py), the
module carries the reference's state_dict, the new entry points are declared, exported and bound, and ten planted errors
each exceed the bars of tests/test_mpd_gpu.py on at least one compared figure."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _mpd_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSSES = ("fm", "gen", "disc", "r_losses", "g_losses")


def _sd(d):
    return {k[3:]: d[k] for k in d if k.startswith("sd/")}


@pytest.fixture(scope="module", params=["t97", "t64"])
def fx(request, golden):
    d = golden(f"mpd_{request.param}.npz")
    return request.param, d, R.run(_sd(d), d["y"], d["y_hat"], torch.from_numpy(d["len_ratios"]))


def _as_stored(want64, stored32):
    """a float64 figure against its copy stored as float32: within half a float32 ulp (plus 1e-12 relative)"""
    want64, stored = np.asarray(want64, np.float64), np.asarray(stored32)
    assert stored.dtype == np.float32 and want64.shape == stored.shape
    slack = 0.5 * np.spacing(np.abs(stored)).astype(np.float64) * (1 + 1e-6) + 1e-12 * np.abs(want64)
    return bool((np.abs(stored.astype(np.float64) - want64) <= slack).all())


def test_restatement_reproduces_the_reference_fixture(fx):
    name, d, got = fx
    for k in LOSSES:
        want = np.asarray(d[k + "64"], np.float64)
        err = float((np.abs(np.asarray(got[k]) - want) / np.abs(want)).max())
        print(f"{name} {k}: {err:.2e} relative")
        assert err <= 1e-12, k
    for i in range(5):
        assert _as_stored(got["out_r"][i], d[f"out_r/{i}"]) and _as_stored(got["out_g"][i], d[f"out_g/{i}"])
    names = [k[5:] for k in d if k.startswith("grad/")]
    assert set(names) == set(got["grad"]) and len(names) == 5 * 6 * 3 + 1
    for k in names:
        assert _as_stored(got["grad"][k], d["grad/" + k]), k
    assert float(d["kink_min_abs"]) > R.KINK_FACTOR * float(d["kink_max_dev"])
    assert float(d["diff_min_abs"]) > R.KINK_FACTOR * float(d["diff_max_dev"])
    assert all(np.abs(d["grad/" + k]).max() > 0 for k in names)


def test_fixture_geometry(golden):
    """T = 97 pads at every period, T = 64 does not at period 2; the ragged counts are not all trivial"""
    for name, T in (("t97", 97), ("t64", 64)):
        d = golden(f"mpd_{name}.npz")
        assert d["y"].shape == d["y_hat"].shape == (3, 1, T) and d["len_ratios"].tolist() == pytest.approx([1.0, 0.7, 0.5])
        assert [T % p != 0 for p in R.PERIODS] == ([True] * 5 if T == 97 else [False] + [True] * 4)
        for i, p in enumerate(R.PERIODS):
            assert d[f"out_r/{i}"].shape[1] % p == 0


def test_module_has_the_reference_state_dict(golden):
    from rad_mmm_amd.discriminators import DiscriminatorP, MultiPeriodDiscriminator
    d = golden("mpd_t97.npz")
    mpd = MultiPeriodDiscriminator()
    sd = mpd.state_dict()
    assert list(sd.keys()) == [str(k) for k in d["default_keys"]]
    assert [",".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in d["default_shapes"]]
    narrow = MultiPeriodDiscriminator(channels=tuple(int(c) for c in d["widths"]))
    narrow.load_state_dict({k: torch.from_numpy(v) for k, v in _sd(d).items()})
    # weight norm comes off and goes back on with the same folded weights
    before = R.fold_weight({k: v.detach() for k, v in narrow.state_dict().items()}, "discriminators.2.convs.3.")
    narrow.remove_weight_norm()
    assert "discriminators.2.convs.3.weight" in narrow.state_dict() and not any(k.endswith("weight_g") for k in narrow.state_dict())
    assert torch.allclose(narrow.state_dict()["discriminators.2.convs.3.weight"], before, rtol=1e-6, atol=0)
    narrow.apply_weight_norm()
    assert list(narrow.state_dict().keys()) == list(_sd(d).keys())
    with pytest.raises(NotImplementedError):
        DiscriminatorP(3, use_spectral_norm=True)
    with pytest.raises(ValueError):
        DiscriminatorP(3, channels=(4, 8, 18, 16, 16))
    with pytest.raises(Exception):                                # no CPU path
        narrow(torch.zeros(1, 1, 64), torch.zeros(1, 1, 64))


def test_load_mpd_reads_the_checkpoint_entry(tmp_path):
    from rad_mmm_amd.discriminators import MultiPeriodDiscriminator, load_mpd
    src = MultiPeriodDiscriminator()
    path = tmp_path / "do_00000001"
    torch.save({"mpd": src.state_dict(), "steps": 1}, path)
    got = load_mpd(str(path), "cpu")
    assert all(torch.equal(a, b) for a, b in zip(src.state_dict().values(), got.state_dict().values()))
    torch.save({"generator": {}}, path)
    with pytest.raises(KeyError):
        load_mpd(str(path), "cpu")


def test_new_entry_points_are_declared_exported_and_bound():
    import rad_mmm_amd._lib as L
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "radmmm_hip.h")).read(), flags=re.S)
    protos = dict(re.findall(r"\b(radmmm_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S))
    raw = ctypes.CDLL(L.LIB_PATH)
    names = {"radmmm_mpd_fold_frame": 10, "radmmm_mpd_repad": 8, "radmmm_mpd_frame": 8, "radmmm_mpd_unframe": 11,
             "radmmm_mpd_conv_post": 9, "radmmm_mpd_conv_post_dgrad": 11, "radmmm_mpd_conv_post_wgrad_parts": 3,
             "radmmm_mpd_conv_post_wgrad": 8, "radmmm_mpd_unfold_audio": 10, "radmmm_mpd_fm_terms_parts": 4,
             "radmmm_mpd_fm_terms": 9, "radmmm_mpd_finish": 11, "radmmm_mpd_fm_grad": 10, "radmmm_mpd_out_grad": 9}
    assert {n for n in protos if n.startswith("radmmm_mpd_")} == set(names)
    for name, n_args in names.items():
        assert protos[name].count(",") + 1 == n_args, name
        assert hasattr(raw, name) and len(getattr(L.lib, name).argtypes) == n_args, name
    assert "#define RADMMM_ABI_VERSION 4" in open(os.path.join(ROOT, "include", "radmmm_hip.h")).read()
    # argument validation happens before any HIP call
    L.lib.radmmm_last_error.restype = ctypes.c_char_p
    a = 0x10000                                                   # never dereferenced
    assert L.lib.radmmm_mpd_fold_frame(None, None, 97, None, 3, 97, 11, 9, 3, None) == -1
    assert b"mpd_fold_frame: null pointer" in L.lib.radmmm_last_error()
    assert L.lib.radmmm_mpd_fold_frame(a, a, 5, a, 2, 5, 11, 1, 1, None) == -1
    assert b"cannot be reflect-padded" in L.lib.radmmm_last_error()
    assert L.lib.radmmm_mpd_fold_frame(a, a, 97, a, 3, 97, 11, 8, 3, None) == -1 and b"do not belong" in L.lib.radmmm_last_error()
    assert L.lib.radmmm_mpd_repad(a, 6, a, 4, 3, 6, 0.1, None) == -1 and b"multiple of 4" in L.lib.radmmm_last_error()
    assert L.lib.radmmm_mpd_frame(a, a, 4, 7, 8, 4, 3, None) == -1 and b"leave the" in L.lib.radmmm_last_error()
    assert L.lib.radmmm_mpd_unframe(a, None, a, a, 4, 7, 8, 4, 3, 0.1, None) == -1 and b"leave the" in L.lib.radmmm_last_error()
    assert L.lib.radmmm_mpd_fm_terms(a, None, a, 2, 3, 4, 1, 1, None) == -1 and b"padded map" in L.lib.radmmm_last_error()
    assert L.lib.radmmm_mpd_conv_post_wgrad_parts(4, 3, 43) == (4 * 3 * 43 + 63) // 64
    assert L.lib.radmmm_mpd_fm_terms_parts(2, 3, 4, 8) == 1 and L.lib.radmmm_mpd_fm_terms_parts(64, 11, 4096, 32) == 1024


@pytest.mark.parametrize("B,T", [(2, 97), (16, 8192), (32, 8192)])
def test_every_layers_gemm_descriptor_is_accepted_at_the_reference_widths(B, T):
    """host only: the descriptors the module builds at the default widths (the first conv's K = 8, the framed convs up to
    N = 1024, K = 5120, lda = 3 * 512 and 1 * 1024, their data gradients with b_layout 1 and the audio gradient's N = 8)
    reach a kernel radmmm_rowgemm_f32_plan accepts, and so do the weight gradients' radmmm_wgrad_f32_plan"""
    from rad_mmm_amd._lib import rowgemm_plan, wgrad_plan
    from rad_mmm_amd.discriminators import _framed, _Geometry
    a = 0x10000                                                   # never dereferenced
    for p in R.PERIODS:
        g = _Geometry(p, (32, 128, 512, 1024, 1024), B, T)
        S = g.S
        assert rowgemm_plan(A=a, lda=8, B=a, ldb=8, C=a, ldc=g.C[0], M=S * g.H[0], N=g.C[0], K=8, T=g.H[0], bias=a) > 0
        assert rowgemm_plan(A=a, lda=g.C[0], B=a, ldb=8, b_layout=1, C=a, ldc=8, M=S * g.H[0], N=8, K=g.C[0], T=g.H[0]) > 0
        assert wgrad_plan(GY=a, ldgy=g.C[0], X=a, ldx=8, P=a, ldp=8, R=S * g.H[0], Mc=g.C[0], Nc=8, T=S * g.H[0]) > 0
        for l in range(1, 5):
            C, H, Cin, Hin, st = g.C[l], g.H[l], g.C[l - 1], g.H[l - 1], g.stride[l]
            kw = _framed(a, S, Hin, Cin, st, a, a, H, C, a)
            assert kw["lda"] == st * Cin and kw["K"] == 5 * Cin and kw["a_item_stride"] == (Hin + 4) * Cin
            assert st * (H - 1) + 5 <= Hin + 4                    # the last window stays inside the sequence's padded rows
            assert rowgemm_plan(**kw) > 0
            assert rowgemm_plan(A=a, lda=C, B=a, ldb=5 * Cin, b_layout=1, C=a, ldc=5 * Cin, M=S * H, N=5 * Cin, K=C, T=H) > 0
            assert wgrad_plan(GY=a, ldgy=C, X=a, ldx=5 * Cin, P=a, ldp=5 * Cin, R=S * H, Mc=C, Nc=5 * Cin, T=S * H) > 0


def _bars(d):
    bars = {k: max(10 * float(np.abs(d[k + "32"] - d[k + "64"]).max()), 1e-6 * float(np.abs(d[k + "64"]).max())) for k in LOSSES}
    gbars = {k[5:]: max(10 * float(d["f32_vs_f64/" + k[5:]]), 1e-6) for k in d if k.startswith("grad/")}
    return bars, gbars


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_planted_errors_exceed_the_gpu_bars(golden, variant):
    """each wrong variant of the restatement, compared as tests/test_mpd_gpu.py compares the module, misses a bar on at least
    one figure of at least one fixture; the largest measured / bar is printed (the margin by which it is seen)"""
    best = 0.0
    for name in ("t97", "t64"):
        d = golden(f"mpd_{name}.npz")
        bars, gbars = _bars(d)
        got = R.run(_sd(d), d["y"], d["y_hat"], torch.from_numpy(d["len_ratios"]), variant=variant)
        over = [float(np.abs(np.asarray(got[k]) - d[k + "64"]).max()) / bars[k] for k in LOSSES]
        over += [R.relative_l2(got["grad"][k], d["grad/" + k]) / gbars[k] for k in gbars]
        print(f"{variant} on {name}: largest measured / bar {max(over):.3g} ({sum(o > 1 for o in over)} of {len(over)} figures miss)")
        best = max(best, max(over))
    assert best > 1.0, variant


def test_a_correct_restatement_passes_those_bars(golden):
    for name in ("t97", "t64"):
        d = golden(f"mpd_{name}.npz")
        bars, gbars = _bars(d)
        got = R.run(_sd(d), d["y"], d["y_hat"], torch.from_numpy(d["len_ratios"]))
        assert all(float(np.abs(np.asarray(got[k]) - d[k + "64"]).max()) <= bars[k] for k in LOSSES)
        assert all(R.relative_l2(got["grad"][k], d["grad/" + k]) <= gbars[k] for k in gbars)
