"""CPU checks for the HiFi-GAN generator's backward pass (no GPU):
  * autograd through the float64 restatement tests/_vocoder_ref.generator_ref reproduces every gradient the reference
    left in tests/golden/vocoder_gen_bwd_r1.npz / _r2.npz (make_golden_vocoder_bwd.py) to 1e-9 relative L2: this ties
    the restatement, which the GPU tests use for other shapes and for the plain-weight form, to the reference;
  * the host models of the two new kernels (tests/_vocoder_bwd_ref.py) agree with torch autograd of leaky_relu and of
    conv1d + tanh in float64 on every case of tests/test_hip_vocoder_bwd_direct.py, and every planted bug is rejected;
  * a training-mode forward on a CPU tensor still raises RadmmmError, the argument checks are unchanged, and a shape
    whose operands exceed the row GEMM's limit raises ValueError."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _vocoder_bwd_ref as K
from _vocoder_ref import V1, load_fixture

TOL = 1e-9


rel_l2, restatement_step = K.rel_l2, K.restatement_step


@pytest.mark.parametrize("name", ["r1", "r2"])
def test_restatement_autograd_reproduces_the_reference_gradients(golden, name):
    cfg, sd = load_fixture(golden(f"vocoder_gen_{name}.npz"))
    d = golden(f"vocoder_gen_bwd_{name}.npz")
    assert float(d["kink_min_abs"]) > 8.0 * float(d["kink_max_dev"])
    loss, g = restatement_step(cfg, sd, torch.from_numpy(d["mel"]), d["lens"].tolist(),
                               torch.from_numpy(d["target"]))
    assert abs(float(loss) - float(d["loss64"])) <= TOL * abs(float(d["loss64"]))
    keys = [k[5:] for k in d if k.startswith("grad/")]
    assert set(keys) == set(g)
    worst = 0.0
    for k in keys:
        # the fixture holds the float64 gradient rounded to float32: compare at that rounding
        err = rel_l2(g[k].numpy().astype(np.float32), d["grad/" + k])
        err64 = rel_l2(g[k].numpy(), d["grad/" + k])
        worst = max(worst, err)
        assert err <= TOL and err64 < 1e-7, (k, err, err64)
    print(f"{name}: {len(keys)} gradients, worst relative L2 {worst:.3e}")


# ---- the host models of the kernels against torch autograd ------------------------------------------------------------

def _items(c, use_lens):
    return [(b, n if use_lens else c["T"]) for b, n in enumerate(c["lens"])]


def _lrelu_autograd(c, inp, use_lens):
    """gx from torch: d/dx sum(gy * leaky_relu(x / div, slope)), x recovered from the saved output a"""
    C, T = c["C"], c["T"]
    div, slope = K._f32(c["div"]), K._f32(c["slope"])
    want = inp["gx0"].astype(np.float64).copy()
    if c["inplace"]:
        want = inp["gy"].astype(np.float64).copy()
    base = want[:, :C].copy()
    want[:, :C] = 0.0
    for b, n in _items(c, use_lens):
        if n == 0:
            continue
        r = slice(b * T, b * T + n)
        a = torch.from_numpy(inp["a"][r, :C].astype(np.float64))
        x = (torch.where(a > 0, a, a / slope) * div).requires_grad_(True)       # any x with this output: same derivative
        y = F.leaky_relu(x / div, slope)
        y.backward(torch.from_numpy(inp["gy"][r, :C].astype(np.float64)))
        want[r, :C] = x.grad.numpy() + (base[r] if c["accum"] else 0.0)
    return want


SMALL_LRELU = [c for c in K.LRELU_BWD_CASES if c["T"] < 1000]


@pytest.mark.parametrize("use_lens", [True, False], ids=["lens", "null"])
@pytest.mark.parametrize("c", SMALL_LRELU, ids=[K.case_id(c) for c in SMALL_LRELU])
def test_lrelu_bwd_model_against_autograd(c, use_lens):
    inp = K.lrelu_bwd_inputs(c, use_lens)
    want = _lrelu_autograd(c, inp, use_lens)
    got = K.lrelu_bwd_expect(c, inp, np.float64)
    C = c["C"]
    assert np.abs(got[:, :C] - want[:, :C]).max() <= 1e-12
    assert K.bit_equal(got[:, C:].astype(np.float32), want[:, C:].astype(np.float32)).all()
    # the float32 model is the same operations in the kernel's precision: within a few roundings of the float64 one
    got32 = K.lrelu_bwd_expect(c, inp, np.float32)
    assert np.abs(got32[:, :C] - want[:, :C]).max() <= 4 * K.U * (np.abs(want[:, :C]).max() + 4.0)
    for bug in K.BUGS:
        if bug == "row_leaks" and not use_lens:
            continue
        if bug == "div_missing" and c["div"] == 1.0:
            continue
        bad = K.lrelu_bwd_expect(c, inp, np.float64, bug)
        with np.errstate(invalid="ignore"):
            ok = np.abs(bad[:, :C] - want[:, :C]) <= 1e-12
        assert not ok.all(), f"planted bug {bug} passes"


def _post_autograd(c, inp, use_lens):
    C, T, taps = c["C"], c["T"], c["taps"]
    div, slope = K._f32(c["div"]), K._f32(c["slope"])
    rows = inp["x"].shape[0]
    w = torch.from_numpy(inp["w"][:, :C].astype(np.float64)).t()[None].contiguous().requires_grad_(True)   # [1, C, taps]
    bias = torch.zeros(1, dtype=torch.float64, requires_grad=True)
    dx = np.zeros((rows, C))
    for b, n in _items(c, use_lens):
        if n == 0:
            continue
        r = slice(b * T, b * T + n)
        x = torch.from_numpy(inp["x"][r, :C].astype(np.float64)).requires_grad_(True)
        pre = F.conv1d(F.leaky_relu(x.t()[None] / div, slope), w, bias, padding=taps // 2)[0, 0]
        # the kernel is handed audio = tanh(pre) and g: choose the upstream gradient that gives the same dpre
        dpre = inp["g"][r].astype(np.float64) * (1.0 - inp["audio"][r].astype(np.float64) ** 2)
        pre.backward(torch.from_numpy(dpre))
        dx[r] = x.grad.numpy()
    return dx, w.grad[0].t().numpy(), float(bias.grad)


SMALL_POST = [c for c in K.POST_BWD_CASES if c["T"] < 1000]


@pytest.mark.parametrize("use_lens", [True, False], ids=["lens", "null"])
@pytest.mark.parametrize("c", SMALL_POST, ids=[K.case_id(c) for c in SMALL_POST])
def test_conv_post_bwd_model_against_autograd(c, use_lens):
    inp = K.post_bwd_inputs(c, use_lens)
    dx, dw, db = _post_autograd(c, inp, use_lens)

    def agrees(e):
        s = max(1.0, np.abs(dw).max())
        return (np.abs(e["dx"] - dx).max() <= 1e-11 and np.abs(e["dw"] - dw).max() <= 1e-11 * s
                and abs(e["dbias"] - db) <= 1e-11 * s)
    assert agrees(K.post_bwd_expect(c, inp))
    for bug in K.POST_BUGS:
        if bug == "row_leaks" and not use_lens:
            continue
        if bug == "div_missing" and c["div"] == 1.0:
            continue
        if bug == "tap_not_flipped" and c["taps"] == 1:
            continue
        with np.errstate(invalid="ignore"):
            assert not agrees(K.post_bwd_expect(c, inp, bug)), f"planted bug {bug} passes"


def test_tanh_derivative_is_part_of_the_model():
    """dpre = g (1 - audio^2): tanh's derivative from its output, against autograd through tanh itself"""
    g = np.random.default_rng(5)
    pre = torch.from_numpy(g.standard_normal(50)).requires_grad_(True)
    up = g.standard_normal(50)
    a = torch.tanh(pre)
    a.backward(torch.from_numpy(up))
    e = K.conv_post_bwd_ref(np.ones((50, 4), np.float32), np.ones((1, 4), np.float32), a.detach().numpy(), up, 4, 1, 50,
                            None, 1.0, 0.01)
    assert np.abs(e["dx"][:, 0] - pre.grad.numpy()).max() < 1e-14


# ---- the module on the CPU ----------------------------------------------------------------------------------------

def test_training_mode_forward_on_the_cpu_still_raises():
    from rad_mmm_amd._lib import RadmmmError
    from rad_mmm_amd.vocoder import HiFiGANGenerator
    cfg = dict(V1, upsample_initial_channel=64)
    gen = HiFiGANGenerator(cfg)
    for mode in (gen.train, gen.eval):
        mode()
        with pytest.raises(RadmmmError, match="no CPU path"):
            gen(torch.zeros(1, 80, 4))
    gen.train()
    assert gen._train_active()
    with torch.no_grad():
        assert not gen._train_active()
    with pytest.raises(ValueError, match="p_blurring"):
        HiFiGANGenerator(dict(cfg, gaussian_blur={"p_blurring": 0.5}))
    names = gen._conv_names()
    assert names[0] == "conv_pre" and names[-1] == "conv_post" and names[1] == "ups.0"
    assert sorted(names) == sorted({k.rsplit(".", 1)[0] for k in gen.state_dict()})
    w = gen._train_weights()
    assert len(w) == 2 * len(names) and all(t.requires_grad for t in w)
    assert w[0].grad_fn is not None                  # folded from weight_g / weight_v under autograd
    assert tuple(w[2].shape) == tuple(gen.ups[0].weight_v.shape)
    gen.remove_weight_norm()
    assert gen._train_weights()[0] is gen.conv_pre.weight


def test_oversized_training_shape_raises_before_any_launch():
    from rad_mmm_amd.vocoder import HiFiGANGenerator
    gen = HiFiGANGenerator(V1)
    gen._check_train_shape(32, 32)                   # the largest training shape of tools/vocoder_bench.py
    with pytest.raises(ValueError, match="row GEMM's limit"):
        gen._check_train_shape(64, 1100)             # 64 * 1100 * 256 rows of 32 channels: above 2 GiB
