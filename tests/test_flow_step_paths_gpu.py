"""One case per path of AffineFlowStepH3Fn that the decoder-level tests do not reach (or reach only at one shape): one flow step
at WN width 64, B = 2, a ragged T of 24 or 40, outputs and ALL gradients against AffineFlowStepFn (fp32 MFMA) on the same inputs.

Paths (ops.flow_plan): transposed copies under h3 / f8x with T < 32; the wide-tap fp32 fallback (5 layers without row-major
pairs: dilation 16 reaches past the copies' zero gap); n_layers outside 2 .. 4 (no c2_src skip sum, no one-pass gQ, no grouped
launch) with pairs and with transposed copies; T % 16 != 0 (the channel mix's weight gradient from split pairs; T = 40 in every
pairs case); frozen parameters; pair-only with two products.

Bars: those of tests/test_hip_parity.py for the precision -- test_decoder_golden for h3 / f8x (outputs 1e-4 of the maximum;
every gradient tensor 5e-4 / f8x 2e-3 of its maximum elementwise and 5e-4 in L2), test_decoder_f16_throughput_mode_is_close
for f16 (outputs 5e-3, gradient norms 2e-2).

The upstream gradients are zero at frames >= length, as under every length-masked loss of this package.  The transposed-copy
strategy depends on that: its res_skip weight gradient of layer j < n-1 reuses the LENGTH-MASKED transposed copy of H[j+1] that
layer j+1's in_layer gradient made, while H[j+1] = softplus(masked conv) is ln 2, not 0, at the padded frames -- with an
upstream gradient that is not zero there, these cases miss res_skip_layers.{0..n-2}.weight_v / weight_g by tens of percent, on this code and on the
commit before the plan alike (known defect).
"""
import numpy as np
import pytest
import torch

from conftest import rel_err

DEV = torch.device("cuda:0")
B, CZ, D, WC = 2, 8, 12, 64

# id: (precision, T, n_layers, frozen, environment)
CASES = {
    "h3-T24-transposed": ("h3", 24, 4, False, {}),
    "f8x-T24-transposed": ("f8x", 24, 4, False, {}),
    "f16-wide-taps": ("f16", 40, 5, False, {}),
    "h3-T24-wide-taps": ("h3", 24, 5, False, {}),
    "f8x-one-layer": ("f8x", 40, 1, False, {}),
    "f8x-five-layers": ("f8x", 40, 5, False, {}),
    "h3-one-layer": ("h3", 40, 1, False, {}),
    "h3-five-layers": ("h3", 40, 5, False, {}),
    "f16-one-layer": ("f16", 40, 1, False, {}),
    "f8x-T40": ("f8x", 40, 4, False, {}),
    "f8x-T40-two-products": ("f8x", 40, 4, False, {"RADMMM_WGRAD_PRODUCTS": "2"}),
    "h3-T40": ("h3", 40, 4, False, {}),
    "f16-T40": ("f16", 40, 4, False, {}),
    "f8x-frozen": ("f8x", 40, 4, True, {}),
    "h3-frozen": ("h3", 40, 4, True, {}),
    "f16-frozen": ("f16", 40, 4, True, {}),
}
_REFERENCE = {}


def _run(precision, T, n_layers, frozen):
    """one AffineTransformationLayer.run, forward and backward -> {name: tensor on the host}"""
    from rad_mmm_amd.common import AffineTransformationLayer
    from rad_mmm_amd.ops import ZLD
    g = torch.Generator().manual_seed(100 * T + n_layers)
    layer = AffineTransformationLayer(CZ, D, n_layers, affine_model="wavenet", scaling_fn="tanh", affine_activation="softplus",
                                      n_channels=WC, use_partial_padding=True)
    with torch.no_grad():
        for n, p in layer.named_parameters():
            p.copy_(torch.rand(p.shape, generator=g) + 0.5 if n.endswith("weight_g") else torch.randn(p.shape, generator=g) * 0.1)
    layer = layer.to(DEV)
    for p in layer.parameters():
        p.requires_grad_(not frozen)
    z = torch.zeros(B * T, ZLD)
    z[:, :CZ] = torch.randn(B * T, CZ, generator=g)
    z = z.to(DEV).requires_grad_(True)
    cond = torch.randn(B * T, D, generator=g).to(DEV).requires_grad_(True)
    W = torch.eye(ZLD)
    W[:CZ, :CZ] += 0.1 * torch.randn(CZ, CZ, generator=g)
    W = W.to(DEV).requires_grad_(True)
    lens = torch.tensor([T, T - 14], dtype=torch.int32, device=DEV)
    mask = (torch.arange(T)[None] < lens.cpu()[:, None]).float().reshape(B * T, 1)
    gz = torch.zeros(B * T, ZLD)
    gz[:, :CZ] = torch.randn(B * T, CZ, generator=g) * mask
    gl = torch.randn(B * T, CZ // 2, generator=g) * mask
    zo, log_s = layer.run(z, cond, lens, W, torch.zeros(ZLD, device=DEV), B, T, precision, {})
    ((zo * gz.to(DEV)).sum() + (log_s * gl.to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    out = {"out.z": zo[:, :CZ], "out.log_s": log_s, "grad.z": z.grad[:, :CZ], "grad.cond": cond.grad, "grad.W_eff": W.grad[:CZ, :CZ]}
    for n, p in layer.named_parameters():
        assert (p.grad is None) == frozen, n
        if p.grad is not None:
            out["grad." + n] = p.grad
    return {k: v.detach().cpu() for k, v in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_flow_step_path_matches_the_fp32_node(case, monkeypatch):
    from rad_mmm_amd import ops
    precision, T, n_layers, frozen, env = CASES[case]
    monkeypatch.setenv("RADMMM_F8X_MIN_ROWS", "0")       # keep the FP8-cross scheme on 80 rows (default: >= 4096 rows)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    plan = ops.flow_plan(ops.NPROD[precision], B, T, n_layers, 1, True)          # the case takes the path it is named for
    assert plan.wgrad == ("pairs" if precision != "f16" and T >= 32 else "transposed") and plan.mix_split == plan.use_rm
    assert plan.multi == (plan.use_rm and n_layers == 4) and plan.res_src == (n_layers == 4), plan
    key = (T, n_layers, frozen)
    if key not in _REFERENCE:
        _REFERENCE[key] = _run("fp32", T, n_layers, frozen)
    ref, got = _REFERENCE[key], _run(precision, T, n_layers, frozen)
    assert set(got) == set(ref)
    for name in sorted(ref):
        e = rel_err(got[name], ref[name])
        l2 = float(np.linalg.norm((got[name] - ref[name]).double().numpy()) / (np.linalg.norm(ref[name].double().numpy()) + 1e-30))
        nrm = abs(float(got[name].norm()) - float(ref[name].norm())) / (float(ref[name].norm()) + 1e-30)
        print(f"{case} [{plan.wgrad}] {name}: max {e:.2e}  L2 {l2:.2e}  norm {nrm:.2e}")
        if precision == "f16":
            assert (e < 5e-3) if name.startswith("out.") else (nrm < 2e-2), (name, e, nrm)
        elif name.startswith("out."):
            assert e < 1e-4, (name, e)
        else:
            assert e < (2e-3 if precision == "f8x" else 5e-4) and l2 < 5e-4, (name, e, l2)
