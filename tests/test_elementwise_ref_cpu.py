"""The float64 host models of tests/_elementwise_ref.py, which the GPU tests of csrc/elementwise.hip and csrc/instnorm.hip
are judged against, pinned on the CPU: each equals float64 autograd through the oracle's functions (weight_norm_fold,
affine_coupling_forward, conv_norm, lengths_to_mask) where the oracle has one, and plain torch otherwise.  No GPU, no
library."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _elementwise_ref as R
from oracle import radmmm_oracle as O

TOL = 1e-12


def _close(a, b, what, tol=TOL):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b.detach() if torch.is_tensor(b) else b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b).max() if a.size else 0.0
    assert err <= tol * max(1.0, np.abs(b).max() if b.size else 0.0), (what, err)


def _rand(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


# ----------------------------------------------------------------------------------------------------------- weight norm
@pytest.mark.parametrize("Cout,Cin,taps,ldw,perm,splits,poison", [
    (3, 10, 5, 12, R.IDENTITY, 1, None), (2, 12, 3, 20, (8, 12, 0), 2, 0.0), (4, 4, 1, 12, (8, 4, 0), 5, float("nan"))])
def test_weightnorm_model_matches_weight_norm_fold(Cout, Cin, taps, ldw, perm, splits, poison):
    g = torch.Generator().manual_seed(Cin)
    v = _rand(g, Cout, Cin, taps).requires_grad_(True)
    gg = (torch.rand(Cout, 1, 1, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    w = O.weight_norm_fold(v, gg)
    cols = R.perm_col(np.arange(Cin), perm)
    assert len(set(cols.tolist())) == Cin and cols.min() >= 0 and cols.max() < ldw
    W, inv = R.weightnorm_fwd(v.detach(), gg.detach(), ldw, perm)
    _close(W[:, :, cols], w.permute(2, 0, 1), "W")
    rest = np.setdiff1d(np.arange(ldw), cols)
    assert np.isnan(W[:, :, rest]).all() and not np.isnan(W[:, :, cols]).any()
    _close(inv, 1 / v.detach().reshape(Cout, -1).norm(dim=1), "inv_norm")
    # dL/dW in W's layout, cut into `splits` slabs; the columns outside col() hold values that must not be read
    gW = _rand(g, taps, Cout, ldw)
    parts = _rand(g, splits, taps, Cout, ldw)
    parts[-1] = gW - parts[:-1].sum(0)
    (w * gW[:, :, cols].permute(1, 2, 0)).sum().backward()
    gw, gw_abs = R.weightnorm_gather(parts, Cin, perm)
    _close(gw, gW[:, :, cols].permute(1, 2, 0), "gathered gradient")
    assert (gw_abs >= np.abs(gw) - 1e-12).all()
    dv, dg, t = R.weightnorm_bwd(v.detach(), gg.detach(), inv, gw, poison)
    _close(dv, v.grad, "dv")
    if poison is not None and np.isnan(poison):
        assert np.isnan(dg).all()
    else:
        _close(dg, gg.grad.reshape(-1), "dg")
    assert (t["absdot"] >= np.abs(t["dot"])).all()


# ------------------------------------------------------------------------------------------------------ WN input scatter
@pytest.mark.parametrize("rows,D,h,ldx0,ldctx,ldz,accum", [(5, 8, 3, 12, 8, 4, 0), (4, 7, 5, 14, 9, 8, 1), (1, 4, 1, 8, 4, 1, 1)])
def test_wn_input_bwd_model_is_the_gradient_of_the_concatenation(rows, D, h, ldx0, ldctx, ldz, accum):
    g = torch.Generator().manual_seed(h)
    ctx, z = _rand(g, rows, ldctx).requires_grad_(True), _rand(g, rows, ldz).requires_grad_(True)
    gX0 = _rand(g, rows, ldx0)
    X0 = F.pad(torch.cat((ctx[:, :D], z[:, :h]), 1), (0, ldx0 - D - h))
    (X0 * gX0).sum().backward()
    gctx0, gz0 = _rand(g, rows, ldctx).numpy(), _rand(g, rows, ldz).numpy()
    gctx, gz = R.wn_input_bwd(gX0.numpy(), gctx0, gz0, D, h, accum)
    _close(gz, gz0 + z.grad.numpy(), "gz")
    _close(gctx[:, :D], (gctx0 if accum else 0 * gctx0)[:, :D] + ctx.grad.numpy()[:, :D], "gctx")
    assert (gctx[:, D:] == gctx0[:, D:]).all() and (gz[:, h:] == gz0[:, h:]).all()


# ------------------------------------------------------------------------------------------------------- affine coupling
@pytest.mark.parametrize("mode,fn", [(R.SCALE_TANH, "tanh"), (R.SCALE_EXP, "exp"), (R.SCALE_SIGMOID, "sigmoid"),
                                     (R.SCALE_TRANSLATE, "translate")])
@pytest.mark.parametrize("h,ldz,with_gl", [(1, 2, True), (3, 9, False), (5, 10, True)])
def test_coupling_model_matches_affine_coupling_forward(mode, fn, h, ldz, with_gl):
    """A WN without layers returns its end conv's bias, so that bias IS one row of O: the oracle's coupling is run row by
    row with O's row as the bias and autograd gives gO and gz of that row."""
    g = torch.Generator().manual_seed(10 * h + mode)
    rows, nch, dc = 4, 3, 2
    Om, z, gzout = _rand(g, rows, 2 * h + 1) * 2, _rand(g, rows, ldz), _rand(g, rows, ldz)
    gl = _rand(g, rows, h) if with_gl else None
    zout, ls, mag = R.coupling_fwd(Om, z, h, mode)
    gsu, gb, gz, bmag = R.coupling_bwd(Om, z, gzout, gl, h, mode)
    pre = "c."
    for r in range(rows):
        bias = Om[r, :2 * h].clone().requires_grad_(True)
        zr = z[r, :2 * h].clone().requires_grad_(True)
        p = {pre + "affine_param_predictor.start.weight": _rand(g, nch, h + dc, 1),
             pre + "affine_param_predictor.start.bias": _rand(g, nch),
             pre + "affine_param_predictor.end.weight": _rand(g, 2 * h, nch, 1),
             pre + "affine_param_predictor.end.bias": bias}
        zo, lo = O.affine_coupling_forward(p, pre, zr[None, :, None], _rand(g, 1, dc, 1), None, 0, fn)
        _close(zout[r, :2 * h], zo[0, :, 0], f"zout row {r}")
        _close(ls[r], lo[0, :, 0], f"log_s row {r}")
        loss = (zo[0, :, 0] * gzout[r, :2 * h]).sum()
        if with_gl:
            loss = loss + (lo[0, :, 0] * gl[r]).sum()
        loss.backward()
        _close(gsu[r], bias.grad[:h], f"gO[:, 0:h] row {r}")
        _close(gb[r], bias.grad[h:], f"gO[:, h:2h] row {r}")
        _close(gz[r, :2 * h], zr.grad, f"gz row {r}")
    assert (zout[:, 2 * h:] == z.numpy()[:, 2 * h:]).all() and (gz[:, 2 * h:] == gzout.numpy()[:, 2 * h:]).all()
    assert (mag["zout1"] >= np.abs(zout[:, h:2 * h]) - 1e-12).all() and (bmag["gz1"] >= np.abs(gz[:, h:2 * h]) - 1e-12).all()
    # the float32 restatement is the same function (to float32 accuracy on these well-conditioned inputs)
    z32, l32 = R.coupling_fwd_f32(Om.numpy(), z.numpy(), h, mode)
    s32, g32 = R.coupling_bwd_f32(Om.numpy(), z.numpy(), gzout.numpy(), None if gl is None else gl.numpy(), h, mode)
    for a, b, m in ((z32[:, h:2 * h], zout[:, h:2 * h], mag["zout1"]), (l32, ls, mag["log_s"]), (s32, gsu, bmag["gsu"]),
                    (g32[:, h:2 * h], gz[:, h:2 * h], bmag["gz1"])):
        assert (np.abs(a - b) <= 64 * R.U * m + 1e-30).all()


# ------------------------------------------------------------------------------------------- row weights, act' from output
@pytest.mark.parametrize("T,lens,taps,dil", [(7, [7, 0, 1, 4], 3, 1), (9, [9, 2, 0], 5, 2), (6, None, 5, 4), (5, [1, 5], 1, 1)])
def test_row_weights_match_conv_norm(T, lens, taps, dil):
    """With a one-channel kernel that is 1 at its centre tap, conv_norm(x) = x * mask * ratio * mask: its gradient is the
    dact_mul row weight.  The bias gradient of a partial conv is the weight-2 column sum of the accumulator gradient."""
    g = torch.Generator().manual_seed(T)
    B = 3 if lens is None else len(lens)
    lt = torch.full((B,), T) if lens is None else torch.tensor(lens)
    mask = O.lengths_to_mask(lt, T)[:, None, :].double()
    _close(R.length_mask(T, lens, B), mask[:, 0], "length mask")
    w = torch.zeros(1, 1, taps, dtype=torch.float64)
    w[0, 0, taps // 2] = 1
    x = _rand(g, B, 1, T).requires_grad_(True)
    O.conv_norm({"c.conv.weight": w}, "c.", x, mask, dil, True).sum().backward()
    _close(R.dact_row_weight(2, T, lens, taps, dil, B), x.grad.reshape(-1), "ratio * mask")
    _close(R.dact_row_weight(1, T, lens, B=B), mask.reshape(-1), "mask")
    assert (R.dact_row_weight(0, T, lens, B=B) == 1).all() and (R.colsum_row_weight(0, T, lens, B=B) == 1).all()
    # bias gradient
    Cin, Cout = 3, 4
    p = {"c.conv.weight": _rand(g, Cout, Cin, taps), "c.conv.bias": _rand(g, Cout).requires_grad_(True)}
    gy = _rand(g, B, Cout, T)
    (O.conv_norm(p, "c.", _rand(g, B, Cin, T), mask, dil, True) * gy).sum().backward()
    gy_rows = gy.permute(0, 2, 1).reshape(B * T, Cout).numpy()
    dacc = R.dact_mul(gy_rows, None, R.ACT_NONE, R.dact_row_weight(2, T, lens, taps, dil, B))
    s, a = R.colsum(dacc, R.colsum_row_weight(2, T, lens, taps, dil, B))
    _close(s, p["c.conv.bias"].grad, "bias gradient")
    assert (a >= np.abs(s) - 1e-12).all()
    s1, _ = R.colsum(gy_rows, R.colsum_row_weight(1, T, lens, B=B))
    _close(s1, (gy * mask).sum((0, 2)), "masked column sum")
    s2, _ = R.colsum(gy_rows, None, square=True)
    _close(s2, (gy * gy).sum((0, 2)), "column sum of squares")


def test_colsum_scratch_count():
    assert R.colsum_scratch_floats(130, 100) == 3 * 100 and R.colsum_scratch_floats(4095, 512) == 64 * 512
    assert R.colsum_scratch_floats(4096, 508) == 64 * 508 and R.colsum_scratch_floats(4096, 512) == 256 * 512


@pytest.mark.parametrize("dact,fn", [(R.ACT_SOFTPLUS, F.softplus), (R.ACT_RELU, torch.relu),
                                     (R.ACT_LEAKY, lambda t: F.leaky_relu(t, 0.01)), (R.ACT_NONE, lambda t: t * 1)])
def test_activation_derivative_from_the_output(dact, fn):
    g = torch.Generator().manual_seed(dact)
    x = torch.cat((_rand(g, 40) * 3, torch.tensor([-30.0, -14.0, 19.5, 20.5, 30.0], dtype=torch.float64))).requires_grad_(True)
    y = fn(x)
    y.sum().backward()
    _close(R.dact_from_out(y.detach().numpy(), dact), x.grad, "act'")
    if dact == R.ACT_SOFTPLUS:
        yy = y.detach().numpy()
        d32 = R.dsoftplus_from_out_f32(yy.astype(np.float32))
        assert (np.abs(d32 - R.dact_from_out(yy.astype(np.float32), dact)) <= 16 * R.U * R.dsoftplus_mag(yy) + 3e-9).all()
    gr, rows = _rand(g, 45, 1).numpy(), np.arange(45) % 2.0
    _close(R.dact_mul(gr, y.detach().numpy()[:, None], dact, rows), gr * x.grad.numpy()[:, None] * rows[:, None], "dact_mul")


# ----------------------------------------------------------------------------------------------------- masked reductions
@pytest.mark.parametrize("B,C,T,lens", [(3, 5, 9, [9, 0, 4]), (2, 3, 1, [1, 0]), (2, 4, 6, None)])
def test_masked_reduce_model(B, C, T, lens):
    g = torch.Generator().manual_seed(T)
    x = _rand(g, B, C, T).requires_grad_(True)
    lt = torch.full((B,), T) if lens is None else torch.tensor(lens)
    m = O.lengths_to_mask(lt, T)[:, None, :].double()
    for mode, coef in ((0, 0.75), (1, -1.5)):
        val = ((x * m) ** 2).sum() if mode else (x * m).sum()
        x.grad = None
        (coef * val).backward()
        assert abs(R.masked_reduce(x.detach().numpy(), lens, mode) - float(val.detach())) <= TOL * max(1.0, abs(float(val.detach())))
        gx = R.masked_reduce_bwd(x.detach().numpy(), lens, mode, coef)
        _close(gx, x.grad, f"gx mode {mode}")
        assert gx.dtype == np.float64 and (gx[m.expand(B, C, T).numpy() == 0] == 0).all()
    # a permuted view gives the same (up to the order numpy adds in)
    xp = x.detach().permute(0, 2, 1).contiguous().permute(0, 2, 1).numpy()
    assert abs(R.masked_reduce(xp, lens, 1) - R.masked_reduce(x.detach().numpy(), lens, 1)) <= TOL * (x.detach() ** 2).sum()


# --------------------------------------------------------------------------------------------------------- instance norm
@pytest.mark.parametrize("B,T,C,lens", [(4, 9, 5, [9, 0, 1, 3]), (2, 4, 3, None), (3, 6, 1, [2, 6, 0])])
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("relu", [0, 1])
def test_instnorm_model_matches_instance_norm_per_item(B, T, C, lens, affine, relu):
    g = torch.Generator().manual_seed(T + C)
    eps = 1e-5
    x = _rand(g, B, T, C).requires_grad_(True)
    w = (_rand(g, C) * 0.5 + 1).requires_grad_(True) if affine else None
    b = (_rand(g, C) * 0.3 - 0.2).requires_grad_(True) if affine else None
    gy = _rand(g, B, T, C)
    ll = [T] * B if lens is None else lens
    y_ref = torch.zeros(B, T, C, dtype=torch.float64)
    for i, n in enumerate(ll):
        if n > 1:
            yi = F.instance_norm(x[i, :n].t()[None], weight=w, bias=b, eps=eps)
            y_ref[i, :n] = (torch.relu(yi) if relu else yi)[0].t()
        elif n == 1:                      # F.instance_norm refuses a single frame: its definition, written out
            xi = x[i, :1]
            yi = (xi - xi.mean(0)) / torch.sqrt(xi.var(0, unbiased=False) + eps) * (1 if w is None else w) + (0 if b is None else b)
            y_ref[i, :1] = torch.relu(yi) if relu else yi
    (y_ref * gy).sum().backward()
    y, mean, rstd = R.instnorm_fwd(x.detach().numpy(), None if w is None else w.detach().numpy(),
                                   None if b is None else b.detach().numpy(), lens, eps, relu)
    _close(y, y_ref, "y")
    for i, n in enumerate(ll):
        xi = x.detach()[i, :n]
        if n:
            _close(mean[i], xi.mean(0), "mean")
            _close(rstd[i], 1 / torch.sqrt(xi.var(0, unbiased=False) + eps), "rstd", 1e-11)
        else:
            assert (mean[i] == 0).all() and np.allclose(rstd[i], eps ** -0.5, rtol=1e-15)
        assert (y[i, n:] == 0).all()
    gx, dw, db, t = R.instnorm_bwd(gy.numpy(), x.detach().numpy(), y, None if w is None else w.detach().numpy(), mean, rstd,
                                   lens, relu)
    _close(gx, x.grad, "gx", 1e-10)
    if affine:
        _close(dw.sum(0), w.grad, "dw", 1e-11)
        _close(db.sum(0), b.grad, "db")
    for i, n in enumerate(ll):
        assert (gx[i, n:] == 0).all()
        if n == 0:
            assert (dw[i] == 0).all() and (db[i] == 0).all()
    assert (t["absdw"] >= np.abs(dw) - 1e-12).all() and (t["absdb"] >= np.abs(db) - 1e-12).all()
