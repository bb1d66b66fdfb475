"""CPU checks of HiFi-GAN's precision "f16": the host models of tests/_vocoder_f16_ref.py, the kernel family's plan query,
the per-stage precision plan of a config, and the switch's name handling.  No GPU."""
import ctypes
import os
import subprocess
import threading

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _vocoder_f16_ref import (LRELU_SLOPE, R1_WIDE, V1_STAGE, W_SCALE, case, conv_f16_ref, generator_f16_ref, h16, rel_l2)
from _vocoder_ref import V1, V3, generator_ref, load_fixture, random_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "radmmm_hip.h")


def _gen(cfg):
    from rad_mmm_amd.vocoder import HiFiGANGenerator
    return HiFiGANGenerator(cfg)


# ---- the host models ------------------------------------------------------------------------------------------------
def test_operand_rounding_model():
    x = np.array([0.0, 1.0, -1.0, 3.14159, -2.71828, 70000.0, -700000.0, 1e-9, 2049.0, 2051.0, -20490.0], dtype=np.float32)
    got = h16(x, 1.0, 0.1)
    assert got.dtype == np.float16
    for xi, gi in zip(x, got):                                     # element by element, in float32 scalars
        v = np.float32(xi) * np.float32(1.0)
        v = v if v >= 0 else np.float32(0.1) * v
        v = min(max(v, np.float32(-60000.0)), np.float32(60000.0))
        assert gi == np.float16(v), (xi, gi)
    assert got[5] == 60000.0 and got[6] == -60000.0                # the clamp (fp16 holds 60000 exactly)
    assert got[8] == 2048.0 and got[9] == 2052.0                   # ties go to even
    assert h16(np.float32([-3.0]), 2.0, 1.0)[0] == -6.0            # in_slope = 1: no leaky-relu
    assert h16(np.float32([-3.0]), 2.0, 0.5)[0] == -3.0


@pytest.mark.parametrize("C,taps,dil", [(16, 3, 1), (48, 7, 5), (32, 11, 5), (16, 7, 12)])
def test_conv_model_is_conv1d_on_fp16_exact_inputs(C, taps, dil):
    g = torch.Generator().manual_seed(C + taps)
    B, T, ldx, ldw = 2, 50, C + 4, C + 8
    X = torch.randn(B * T, ldx, generator=g).half().float()        # fp16-exact: h() changes nothing (no slope, scale 1)
    Wh = torch.randn(taps, C, ldw, generator=g).half()
    bias, add = torch.randn(C, generator=g), torch.randn(B * T, C, generator=g)
    got = conv_f16_ref(X.numpy(), Wh.numpy(), bias.numpy(), B, T, C, taps, dil, add=add.numpy(), acc_scale=0.5)
    x = X.view(B, T, ldx)[:, :, :C].transpose(1, 2).double()
    w = Wh[:, :, :C].permute(1, 2, 0).double() * 0.5
    ref = F.conv1d(x, w, bias.double(), dilation=dil, padding=(taps // 2) * dil).transpose(1, 2).reshape(B * T, C) + add.double()
    err = np.abs(got["y"] - ref.numpy()).max()
    print(f"C {C} taps {taps} dil {dil}: max-abs against conv1d {err:.3e} (|ref| max {ref.abs().max():.2f})")
    assert err <= 1e-12 * ref.abs().max()
    assert np.array_equal(got["y"], got["y2"])


def test_conv_model_masks_and_accumulates():
    g = torch.Generator().manual_seed(3)
    B, T, C, taps, dil = 3, 20, 16, 3, 2
    lens = [20, 1, 7]
    X = torch.randn(B * T, C, generator=g).numpy().copy()
    add = torch.randn(B * T, C, generator=g).numpy().copy()
    Wh = torch.randn(taps, C, C, generator=g).half().numpy()
    bias = np.zeros(C, dtype=np.float32)
    y2_before = torch.randn(B * T, C, generator=g).numpy()
    clean = conv_f16_ref(X, Wh, bias, B, T, C, taps, dil, lens=lens, add=add, Y2=y2_before, y2_accum=True, in_slope=0.1)
    for b, n in enumerate(lens):
        X[b * T + n:(b + 1) * T] = np.nan
        add[b * T + n:(b + 1) * T] = np.nan
    got = conv_f16_ref(X, Wh, bias, B, T, C, taps, dil, lens=lens, add=add, Y2=y2_before, y2_accum=True, in_slope=0.1)
    assert np.array_equal(got["y"], clean["y"]) and np.isfinite(got["y"]).all()
    for b, n in enumerate(lens):
        assert not got["y"][b * T + n:(b + 1) * T].any()
    assert np.array_equal(got["y2"], got["y"] + y2_before.astype(np.float64))
    # item 2 alone, cut at its length, is the same: the rows past a length are zeros to the taps
    alone = conv_f16_ref(X[2 * T:2 * T + 7], Wh, bias, 1, 7, C, taps, dil, add=add[2 * T:2 * T + 7], in_slope=0.1)
    assert np.array_equal(alone["y"], got["y"][2 * T:2 * T + 7])


def test_all_fp32_plan_is_the_exact_restatement(golden):
    cfg, sd = load_fixture(golden("vocoder_gen_r2.npz"))
    mel = torch.from_numpy(golden("vocoder_gen_r2.npz")["mel"])[:1, :, :6]
    assert torch.equal(generator_f16_ref(sd, cfg, mel, ["fp32"] * 3), generator_ref(sd, cfg, mel))
    c = case("r1")
    mel = c["mel"][:1, :, :c["lens"][0]]
    assert torch.equal(generator_f16_ref(c["sd"], c["cfg"], mel, [("fp32", "x"), ("fp32", "y")]), generator_ref(c["sd"], c["cfg"], mel))


@pytest.mark.parametrize("name", ["r1", "r1_wide", "v1_stage"])
def test_the_emulation_is_far_from_fp32_on_the_gpu_tests_inputs(name):
    """tests/test_vocoder_f16_gpu.py holds the HIP error within a factor 3 of the emulation's, both ways.  The lower side
    separates the mode from the fp32 path (near 5e-7) only if the emulation's own error is well above that."""
    c = case(name)
    assert "f16" in c["plan"]
    for b, n in enumerate(c["lens"]):
        e = rel_l2(c["refs"][b]["f16"], c["refs"][b]["exact"])
        print(f"{name} item {b} ({n} frames): emulation rel-L2 against exact {e:.3e}")
        assert e >= 1e-5
        assert c["refs"][b]["exact"].abs().max() < 0.999          # not saturated in tanh: the error is visible


# ---- the kernel family's plan query -----------------------------------------------------------------------------------
def _plan(**kw):
    import rad_mmm_amd._lib as L
    a = 0x10000                                                  # never dereferenced
    C = kw.get("C", 32)
    base = dict(X=a, ldx=(C + 7) // 4 * 4, Wh=a, ldw=(C + 15) // 8 * 8, Y=2 * a, ldy=C + 1, B=3, T=700, C=C, taps=3, dil=1, bias=a)
    base.update(kw)
    return L.voc_conv_f16_plan(**base), L.lib.radmmm_last_error().decode()


def test_plan_over_a_table_of_shapes():
    import rad_mmm_amd._lib as L
    code = L.voc_f16_kernel_code
    taken = {16: code(1, 4), 32: code(1, 4), 48: code(2, 2), 64: code(2, 2), 128: code(4, 1), 256: code(8, 1)}
    for C, want in taken.items():
        for taps, dil in ((3, 1), (11, 5), (7, 12), (7, 5), (1, 1), (11, 8)):
            assert _plan(C=C, taps=taps, dil=dil)[0] == want, (C, taps, dil)
    for C in (8, 272, 24, 4):
        rc, why = _plan(C=C)
        assert rc == 0 and why.startswith(f"voc_conv_f16: C={C} not taken"), why
    for taps in (13, 2, 4):
        rc, why = _plan(taps=taps)
        assert rc == 0 and why.startswith(f"voc_conv_f16: taps={taps} not taken"), why
    for taps, dil in ((11, 9), (3, 41), (7, 14)):                 # a reach over the limit of 40
        rc, why = _plan(taps=taps, dil=dil)
        assert rc == 0 and "reach" in why and "not taken" in why, why
    assert _plan(taps=3, dil=40)[0] == code(1, 4) and _plan(taps=11, dil=8)[0] == code(1, 4)
    hdr = open(HDR).read()
    assert "#define RADMMM_VOC_F16_KERNEL_CODE(ntc, mi) ((ntc) * 100 + (mi))" in hdr and code(8, 1) == 801


def test_bad_arguments_are_refused_before_any_hip_call():
    import rad_mmm_amd._lib as L
    lib = L.lib
    assert lib.radmmm_voc_conv_f16_plan(None) == -1 and lib.radmmm_last_error() == b"voc_conv_f16: null descriptor"
    assert lib.radmmm_voc_conv_f16(None, None) == -1 and lib.radmmm_last_error() == b"voc_conv_f16: null descriptor"
    a = 0x10000
    ok = dict(X=a, ldx=32, Wh=a, ldw=32, Y=2 * a, ldy=32, B=2, T=9, C=32, taps=3, dil=1, bias=a)
    refused = [(dict(ok, bias=None), "null pointer"), (dict(ok, T=0), "bad dims"), (dict(ok, dil=0), "bad dims"),
               (dict(ok, B=1 << 20, T=1 << 12), "bad dims"), (dict(ok, ldx=30), "bad pitches"), (dict(ok, ldw=36), "bad pitches"),
               (dict(ok, ldy=31), "bad pitches"), (dict(ok, add=a, ldadd=8), "bad pitches"), (dict(ok, X=a + 4), "16B aligned"),
               (dict(ok, Y=a), "alias"), (dict(ok, add=2 * a, ldadd=32), "alias"), (dict(ok, Y2=2 * a, ldy2=32), "alias")]
    for kw, text in refused:
        d = L._voc_f16_desc(kw, L._addr)
        assert lib.radmmm_voc_conv_f16_plan(ctypes.byref(d)) == -1 and text in lib.radmmm_last_error().decode(), (kw, text)
        mine = lib.radmmm_last_error()
        assert lib.radmmm_voc_conv_f16(ctypes.byref(d), None) == -1 and lib.radmmm_last_error() == mine
        with pytest.raises(L.RadmmmError, match=text):
            L.voc_conv_f16_plan(**kw)
    seen = []

    def fresh_thread():                                          # a shape the plan does not take: the entry point runs nothing
        seen.append(lib.radmmm_voc_conv_f16_last_kernel())
        d = L._voc_f16_desc(dict(ok, C=8, ldx=8, ldw=8, ldy=8), L._addr)
        seen.append(lib.radmmm_voc_conv_f16_plan(ctypes.byref(d)))
        seen.append(lib.radmmm_voc_conv_f16(ctypes.byref(d), None))
        seen.append(lib.radmmm_last_error())
        seen.append(lib.radmmm_voc_conv_f16_last_kernel())

    t = threading.Thread(target=fresh_thread)
    t.start()
    t.join()
    assert seen[0] == 0 and seen[1] == 0 and seen[2] == -1 and b"C=8 not taken" in seen[3] and seen[4] == 0


def test_descriptor_mirror_matches_the_c_layout(tmp_path):
    import rad_mmm_amd._lib as L
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HDR}"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(radmmm_voc_conv_f16_desc));']
    for fname, _ in L.VocConvF16Desc._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(radmmm_voc_conv_f16_desc, {fname}));')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines))
    r = subprocess.run(["gcc", "-std=c99", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(L.VocConvF16Desc)
    for fname, _ in L.VocConvF16Desc._fields_:
        assert int(got[fname]) == getattr(L.VocConvF16Desc, fname).offset, fname


# ---- the switch ---------------------------------------------------------------------------------------------------------
def test_precision_plan_per_config(golden):
    from rad_mmm_amd.vocoder import PRECISIONS
    assert PRECISIONS == ("fp32", "f16")
    g = _gen(V1)
    assert g.precision == "fp32"
    assert [m for m, _ in g.precision_plan()] == ["fp32"] * 4                 # the attribute's mode
    assert g.precision_plan("f16") == [("f16", "")] * 4                        # 256 / 128 / 64 / 32, reach up to 25
    assert _gen(V3).precision_plan("f16") == [("f16", "")] * 3                 # 128 / 64 / 32, k = 7 with d = 12: reach 36
    for name, want in (("r1", ["f16", "fp32"]), ("r2", ["f16", "fp32", "fp32"])):   # widths 16 / 8 (/ 4): mixed plans
        cfg, _ = load_fixture(golden(f"vocoder_gen_{name}.npz"))
        plan = _gen(cfg).precision_plan("f16")
        assert [m for m, _ in plan] == want
        assert plan[0][1] == "" and "C=8 not taken" in plan[1][1]
    assert "C=4 not taken" in plan[2][1]
    narrow = _gen(dict(R1_WIDE, upsample_initial_channel=16)).precision_plan("f16")          # widths 8 / 4: all fp32
    assert [m for m, _ in narrow] == ["fp32", "fp32"] and all(why for _, why in narrow)
    assert [m for m, _ in _gen(R1_WIDE).precision_plan("f16")] == ["f16", "f16"]
    assert [m for m, _ in _gen(V1_STAGE).precision_plan("f16")] == ["f16"]
    far = dict(R1_WIDE, resblock_kernel_sizes=[3, 5, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 9]])
    plan = _gen(far).precision_plan("f16")                                      # k = 11, d = 9: reach 45
    assert [m for m, _ in plan] == ["fp32", "fp32"] and "reach" in plan[0][1]
    g.precision = "f16"
    assert g.precision_plan() == [("f16", "")] * 4 and [m for m, _ in g.precision_plan("fp32")] == ["fp32"] * 4


def test_unknown_names_raise_before_any_device_work(tmp_path):
    from rad_mmm_amd.vocoder import HiFiGANGenerator, load_hifigan_vocoder, vocode
    g = _gen(R1_WIDE).eval()
    mel = torch.zeros(1, 80, 4)                                   # a CPU tensor: a valid name would raise RadmmmError
    for bad in ("h3", "fp16", "", "F16"):
        with pytest.raises(ValueError, match="precision"):
            g(mel, precision=bad)
        with pytest.raises(ValueError, match="precision"):
            g.precision_plan(bad)
        with pytest.raises(ValueError, match="precision"):
            vocode(g, None, mel, [4], precision=bad)
        with pytest.raises(ValueError, match="precision"):        # before the files are looked at
            load_hifigan_vocoder(str(tmp_path / "none.pt"), str(tmp_path / "none.json"), precision=bad)
        g.precision = bad
        try:
            with pytest.raises(ValueError, match="precision"):
                g(mel)
            with pytest.raises(ValueError, match="precision"):
                vocode(g, None, mel, [4])
        finally:
            g.precision = "fp32"
    from rad_mmm_amd._lib import RadmmmError
    with pytest.raises(RadmmmError):
        g(mel, precision="f16")


def test_f16_in_training_mode_is_the_fp32_step():
    g = _gen(R1_WIDE)
    g.precision = "f16"
    g.train()
    assert g._mode() == "fp32" and g._mode("f16") == "fp32"       # grad enabled: the training step, whatever the name
    with torch.no_grad():
        assert g._mode() == "f16"
    g.eval()
    assert g._mode() == "f16" and g._mode("fp32") == "fp32"
    g.train()
    with pytest.raises(ValueError, match="precision"):            # a name is still checked
        g._mode("half")


def test_f16_weights_live_inside_the_fold():
    import inspect
    from rad_mmm_amd.vocoder import HiFiGANGenerator
    src = inspect.getsource(HiFiGANGenerator._f16_weights)
    assert 'f.setdefault("f16"' in src and "nprod=1" in src and "ops.W_SCALE" in src
    assert W_SCALE == __import__("rad_mmm_amd.ops", fromlist=["W_SCALE"]).W_SCALE
    assert LRELU_SLOPE == __import__("rad_mmm_amd.vocoder", fromlist=["LRELU_SLOPE"]).LRELU_SLOPE
