"""Host models of the flow step's memory-bound kernels (csrc/elementwise.hip, csrc/instnorm.hip): plain float64 numpy
restatements of what include/radmmm_hip.h says each entry point computes, on the same channels-last arrays and with the
same arguments.  tests/test_elementwise_ref_cpu.py holds them to float64 autograd through oracle/radmmm_oracle.py and
torch; tests/test_hip_elementwise_direct.py judges the kernels against them.

Besides the value, the reduction models return the sum of the absolute values of the added terms, which the forward error
bounds of the GPU tests are built from.  The *_f32 functions restate the transcendental pieces in float32 torch on the
CPU: they are used only to measure how far float32 arithmetic on a test's inputs is from float64 (the tolerance of those
tests is a multiple of that), never as a reference."""
import numpy as np
import torch

U = 2.0 ** -24                           # unit roundoff of float32
SCALE_TANH, SCALE_EXP, SCALE_SIGMOID, SCALE_TRANSLATE = 0, 1, 2, 3
ACT_NONE, ACT_SOFTPLUS, ACT_RELU, ACT_LEAKY = 0, 1, 2, 3
IDENTITY = (0, 0, 0)


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ----------------------------------------------------------------------------------------------------------- weight norm
def perm_col(ci, perm):
    """col(ci) = ci < perm_split ? ci + off_lo : ci - perm_split + off_hi"""
    ps, lo, hi = perm
    ci = np.asarray(ci)
    return np.where(ci < ps, ci + lo, ci - ps + hi)


def weightnorm_fwd(v, g, ldw, perm=IDENTITY):
    """v [Cout][Cin][taps], g [Cout] -> W [taps][Cout][ldw] (NaN where no col(ci) lands: those columns are not written),
    inv_norm [Cout]"""
    v, g = f64(v), f64(g).reshape(-1)
    Cout, Cin, taps = v.shape
    nrm = np.sqrt((v * v).reshape(Cout, -1).sum(1))
    W = np.full((taps, Cout, ldw), np.nan)
    W[:, :, perm_col(np.arange(Cin), perm)] = (v * (g / nrm)[:, None, None]).transpose(2, 0, 1)
    return W, 1.0 / nrm


def weightnorm_gather(slabs, Cin, perm=IDENTITY):
    """slabs [splits][taps][Cout][ldw] of dL/dW -> (gw, |gw| terms) [Cout][Cin][taps]: the slabs added up, read through the
    column permutation.  A slab array carved out of a flat buffer with a split_stride is the caller's business."""
    s = f64(slabs)[:, :, :, perm_col(np.arange(Cin), perm)]
    return s.sum(0).transpose(1, 2, 0), np.abs(s).sum(0).transpose(1, 2, 0)


def weightnorm_bwd(v, g, inv_norm, gw, poison=None):
    """dL/dv [Cout][Cin][taps] and dL/dg [Cout] of W = g v / ||v|| from gw = dL/dW in v's layout; inv_norm as the forward
    stored it.  dg carries + poison (None: nothing).  Also returns the pieces the error bounds need:
    dot = sum gw v, absdot = sum |gw v|, a = g inv, b = g dot inv^3 (dv = a gw - b v)."""
    v, g, inv, gw = f64(v), f64(g).reshape(-1), f64(inv_norm).reshape(-1), f64(gw)
    Cout = v.shape[0]
    dot = (gw * v).reshape(Cout, -1).sum(1)
    absdot = np.abs(gw * v).reshape(Cout, -1).sum(1)
    a, b = g * inv, g * dot * inv ** 3
    dv = a[:, None, None] * gw - b[:, None, None] * v
    dg = dot * inv + (0.0 if poison is None else float(poison))
    return dv, dg, dict(dot=dot, absdot=absdot, a=a, b=b)


# ------------------------------------------------------------------------------------------------------ WN input scatter
def wn_input_bwd(gX0, gctx, gz, D, h, ctx_accum):
    """gctx[r, 0:D] (+)= gX0[r, 0:D]; gz[r, 0:h] += gX0[r, D:D+h]; every other column is left as it was.  Works in the
    dtype of its inputs (float32 in: the single rounded additions of the kernel, bit for bit)."""
    gctx, gz = gctx.copy(), gz.copy()
    gctx[:, :D] = gctx[:, :D] + gX0[:, :D] if ctx_accum else gX0[:, :D]
    gz[:, :h] = gz[:, :h] + gX0[:, D:D + h]
    return gctx, gz


# ------------------------------------------------------------------------------------------------------- affine coupling
def scaling(su, mode):
    """(s, log_s, S): AffineTransformationLayer.get_scaling_and_logs; S is the sum of the magnitudes of the terms s is
    added up from (tanh(su) + 1 + 1e-6 cancels for su < 0)"""
    su = f64(su)
    if mode == SCALE_TANH:
        th = np.tanh(su)
        s = th + 1 + 1e-6
        return s, np.log(s), np.abs(th) + 1 + 1e-6
    if mode == SCALE_EXP:
        s = np.exp(su)
        return s, su.copy(), s
    if mode == SCALE_SIGMOID:
        s = 1 / (1 + np.exp(-(su + 10))) + 1e-6
        return s, np.log(s), s
    return np.ones_like(su), np.zeros_like(su), np.ones_like(su)


def coupling_fwd(O, z, h, mode):
    """O [rows][>= 2h], z [rows][ldz] -> zout [rows][ldz], log_s [rows][h], and the magnitudes the tolerances scale with"""
    O, z = f64(O), f64(z)
    su, b, z1 = O[:, :h], O[:, h:2 * h], z[:, h:2 * h]
    s, ls, S = scaling(su, mode)
    zout = z.copy()
    zout[:, h:2 * h] = s * z1 + b
    mag = dict(zout1=S * np.abs(z1) + np.abs(b), log_s=S / s + np.abs(ls))
    return zout, ls, mag


def coupling_bwd(O, z, gzout, glog_s, h, mode):
    """-> gsu = gO[:, 0:h], gb = gO[:, h:2h], gz [rows][ldz], magnitudes.  glog_s None counts as zero."""
    O, z, gzout = f64(O), f64(z), f64(gzout)
    su, z1, gv = O[:, :h], z[:, h:2 * h], gzout[:, h:2 * h]
    gl = np.zeros_like(su) if glog_s is None else f64(glog_s)
    s, _, S = scaling(su, mode)
    if mode == SCALE_TANH:
        th = np.tanh(su)
        gsu = (gv * z1 + gl / s) * (1 - th * th)
        mag = (np.abs(gv * z1) + np.abs(gl / s) * (1 + S / s)) * (1 + th * th)
    elif mode == SCALE_EXP:
        gsu = gv * z1 * s + gl
        mag = np.abs(gv * z1 * s) + np.abs(gl)
    elif mode == SCALE_SIGMOID:
        sg = 1 / (1 + np.exp(-(su + 10)))
        gsu = (gv * z1 + gl / s) * sg * (1 - sg)
        mag = (np.abs(gv * z1) + np.abs(gl / s) * (1 + S / s)) * sg * (1 + sg)
    else:
        gsu = np.zeros_like(su)
        mag = np.zeros_like(su)
    gz = gzout.copy()
    gz[:, h:2 * h] = gv * s
    return gsu, gv.copy(), gz, dict(gsu=mag, gz1=np.abs(gv) * S)


def _scaling_f32(su, mode):
    one, eps = torch.tensor(1.0), torch.tensor(1e-6)                    # float32 scalars
    if mode == SCALE_TANH:
        th = torch.tanh(su)
        s = th + one + eps
        return s, torch.log(s), th
    if mode == SCALE_EXP:
        return torch.exp(su), su.clone(), None
    if mode == SCALE_SIGMOID:
        sg = one / (one + torch.exp(-(su + 10.0)))
        s = sg + eps
        return s, torch.log(s), sg
    return torch.ones_like(su), torch.zeros_like(su), None


def coupling_fwd_f32(O, z, h, mode):
    """the forward in float32 torch on the CPU, operation for operation as the kernel states it"""
    O, z = torch.as_tensor(O, dtype=torch.float32), torch.as_tensor(z, dtype=torch.float32)
    s, ls, _ = _scaling_f32(O[:, :h], mode)
    zout = z.clone()
    zout[:, h:2 * h] = s * z[:, h:2 * h] + O[:, h:2 * h]
    return zout.numpy(), ls.numpy()


def coupling_bwd_f32(O, z, gzout, glog_s, h, mode):
    O, z, gzout = (torch.as_tensor(t, dtype=torch.float32) for t in (O, z, gzout))
    su, z1, gv = O[:, :h], z[:, h:2 * h], gzout[:, h:2 * h]
    gl = torch.zeros_like(su) if glog_s is None else torch.as_tensor(glog_s, dtype=torch.float32)
    s, _, t = _scaling_f32(su, mode)
    if mode == SCALE_TANH:
        gsu = (gv * z1 + gl / s) * (1.0 - t * t)
    elif mode == SCALE_EXP:
        gsu = gv * z1 * s + gl
    elif mode == SCALE_SIGMOID:
        gsu = (gv * z1 + gl / s) * t * (1.0 - t)
    else:
        gsu = torch.zeros_like(su)
    gz = gzout.clone()
    gz[:, h:2 * h] = gv * s
    return gsu.numpy(), gz.numpy()


# ------------------------------------------------------------------------------------------- row weights, act' from output
def pconv_ratio(T, lens, taps, dil, B=None):
    """[B][T]: taps / (cnt + 1e-6) where the (taps, dil) window centred on t holds cnt > 0 frames below len_b, else 0
    (partialconv1d.py:75-81).  lens None: every item is T long (give B)."""
    lens = np.full(B, T) if lens is None else np.asarray(lens)
    t = np.arange(T)[None, :, None] + (np.arange(taps)[None, None, :] - taps // 2) * dil
    cnt = ((t >= 0) & (t < lens[:, None, None])).sum(2).astype(np.float64)
    return np.where(cnt > 0, taps / (cnt + 1e-6), 0.0), cnt


def length_mask(T, lens, B=None):
    lens = np.full(B, T) if lens is None else np.asarray(lens)
    return (np.arange(T)[None] < lens[:, None]).astype(np.float64)


def dact_row_weight(rowscale, T, lens, taps=1, dil=1, B=None):
    """w(r) of radmmm_dact_mul, [B * T]: rowscale 0: 1; 1: [t < len]; 2: [t < len] * partial-conv ratio"""
    m = length_mask(T, lens, B)
    if rowscale == 0:
        return np.ones(m.size)
    if rowscale == 1:
        return m.reshape(-1)
    return (m * pconv_ratio(T, lens, taps, dil, B)[0]).reshape(-1)


def colsum_row_weight(row_weight, T, lens, taps=1, dil=1, B=None):
    """w(r) of radmmm_colsum, [B * T]: 0: 1; 1: [t < len]; 2: [t < len] * (cnt + 1e-6) / taps (undoes the ratio)"""
    m = length_mask(T, lens, B)
    if row_weight == 0:
        return np.ones(m.size)
    if row_weight == 1:
        return m.reshape(-1)
    return (m * (pconv_ratio(T, lens, taps, dil, B)[1] + 1e-6) / taps).reshape(-1)


def dact_from_out(y, dact):
    """act'(x) written from the activation's OUTPUT y = act(x): softplus' = sigmoid(x) = 1 - exp(-y), and 1 where y > 20
    (torch's softplus is the identity above its threshold of 20); relu' = [y > 0]; leaky' = y > 0 ? 1 : 0.01"""
    y = f64(y)
    if dact == ACT_SOFTPLUS:
        return np.where(y > 20, 1.0, -np.expm1(-y))
    if dact == ACT_RELU:
        return (y > 0).astype(np.float64)
    if dact == ACT_LEAKY:
        return np.where(y > 0, 1.0, 0.01)
    return np.ones_like(y)


def dsoftplus_mag(y):
    """magnitude of what 1 - exp(-y) is added up from; below 0.25 the kernel sums a series whose leading term is y"""
    y = f64(y)
    return np.where(y < 0.25, y, np.where(y > 20, 1.0, 1 + np.exp(-y)))


def dsoftplus_from_out_f32(y):
    """float32 restatement of the kernel's softplus derivative: 1 above 20, the series of 1 - exp(-y) below 0.25"""
    y = torch.as_tensor(y, dtype=torch.float32)
    c = [torch.tensor(k, dtype=torch.float32) for k in (0.5, 0.16666667, 0.041666668, 0.0083333338, 0.0013888889)]
    p = y * (1.0 - y * (c[0] - y * (c[1] - y * (c[2] - y * (c[3] - y * c[4])))))
    d = torch.where(y < 0.25, p, 1.0 - torch.exp(-y))
    return torch.where(y > 20.0, torch.ones_like(y), d).numpy()


def dact_mul(g, saved, dact, w):
    """y[r, c] = g[r, c] * act'(saved[r, c]) * w[r]"""
    return f64(g) * dact_from_out(saved, dact) * f64(w)[:, None]


# ------------------------------------------------------------------------------------------------------------ column sums
def colsum(X, w=None, square=False):
    """(out, abs) [cols]: out[c] = sum_r w[r] f(X[r, c]), f = identity or square; abs = sum_r |w[r] f(X[r, c])|"""
    X = f64(X)
    t = (X * X if square else X) * (1.0 if w is None else f64(w)[:, None])
    return t.sum(0), np.abs(t).sum(0)


def colsum_rows_per_block(rows, cols):
    return 16 if rows >= 4096 and cols >= 512 else 64


def colsum_scratch_floats(rows, cols):
    rpb = colsum_rows_per_block(rows, cols)
    return -(-rows // rpb) * cols


# ----------------------------------------------------------------------------------------------------- masked reductions
def masked_reduce(x, lens, mode):
    """x [B][C][T] (any strides) -> sum of x m (mode 0) or of (x m)^2 (mode 1), m = [t < lens[b]]"""
    x = f64(x)
    xm = x * length_mask(x.shape[2], lens, x.shape[0])[:, None, :]
    return float((xm * xm if mode else xm).sum())


def masked_reduce_bwd(x, lens, mode, coef):
    """gx = coef m (mode 1 ? 2 x : 1), in the dtype of x (float32 in: one rounded product, bit for bit)"""
    m = length_mask(x.shape[2], lens, x.shape[0])[:, None, :] > 0
    cf = x.dtype.type(coef)
    v = (x.dtype.type(2) * cf) * x if mode else np.full_like(x, cf)
    return np.where(m, v, x.dtype.type(0)).astype(x.dtype)


# --------------------------------------------------------------------------------------------------------- instance norm
def instnorm_fwd(x, w, b, lens, eps, relu):
    """x [B][T][C]; statistics over t < len_b (biased variance, eps inside the rsqrt), zeros at t >= len_b; an empty item
    has mean 0 and rstd 1 / sqrt(eps).  -> y [B][T][C], mean [B][C], rstd [B][C]"""
    x = f64(x)
    B, T, C = x.shape
    m = length_mask(T, lens, B)[:, :, None]
    n = np.maximum(m.sum(1), 1.0)
    mean = (x * m).sum(1) / n
    d = (x - mean[:, None]) * m
    rstd = 1 / np.sqrt((d * d).sum(1) / n + eps)
    y = d * rstd[:, None] * (1.0 if w is None else f64(w)) + (0.0 if b is None else f64(b))
    if relu:
        y = np.maximum(y, 0.0)
    return y * m, mean, rstd


def instnorm_bwd(gy, x, y, w, mean, rstd, lens, relu):
    """gradient of instnorm_fwd from the SAVED y, mean and rstd (relu: the gate is y > 0) -> gx [B][T][C] (zeros at
    t >= len_b) and the per-item partials dw_part = sum_t g xhat, db_part = sum_t g [B][C], plus the sums of the absolute
    values of their terms"""
    gy, x, mean, rstd = f64(gy), f64(x), f64(mean), f64(rstd)
    B, T, C = x.shape
    m = length_mask(T, lens, B)[:, :, None]
    n = np.maximum(m.sum(1), 1.0)[:, None]
    g = gy * m
    if relu:
        g = g * (np.asarray(y) > 0)
    ww = np.ones(C) if w is None else f64(w)
    xh = (x - mean[:, None]) * rstd[:, None] * m
    db, dw = g.sum(1), (g * xh).sum(1)
    m1, m2 = db[:, None] * ww / n, dw[:, None] * ww / n
    gx = rstd[:, None] * (g * ww - m1 - xh * m2) * m
    return gx, dw, db, dict(absdb=np.abs(g).sum(1), absdw=np.abs(g * xh).sum(1), g=g, xh=xh, m1=m1, m2=m2, n=n, ww=ww)
