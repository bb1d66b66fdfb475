"""The memory-bound kernels of the flow step (csrc/elementwise.hip) and the masked instance norm (csrc/instnorm.hip), called
through the C ABI with leading dimensions, offsets and split strides chosen by the test, against the float64 host models of
tests/_elementwise_ref.py (themselves pinned by tests/test_elementwise_ref_cpu.py).

Rules every test follows:
  * outputs start as the bit pattern SENT_BITS; whatever the header does not say is written must still hold it;
  * a copy or a single rounded float32 operation is compared bit for bit with a float32 numpy restatement;
  * plain sums get inputs that float32 adds exactly in any order (small integers / 8), and must be the exact sum;
  * everything else is compared element by element with the float64 model under a bound computed from the shape:
      reductions     (n_chain + n_tree + c) * 2^-24 * sum|terms|, n_chain the longest serial accumulation of one thread as
                     the kernel is written, n_tree the combine levels, c the roundings of the elementwise tail (stated at
                     each use), plus the propagated error of any reduced quantity the output is computed from;
      transcendental 4 x the per-element error of the float32 CPU restatement of the same formula on the test's own inputs,
                     relative to the magnitude of the added terms (the `mag` arrays of the model): device tanhf / expf / logf
                     may differ from the host's by a few ulp and one contraction into fma is allowed.
    No bound is a tuned number."""
import math

import numpy as np
import pytest
import torch

import _elementwise_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = R.U
F32 = np.float32
SENT_BITS = 0x449A522B                                   # 1234.5677: of a size at which adding an O(1) value changes the bits
                                                         # (a huge or NaN pattern would swallow a stray accumulation)
SENT = float(np.array([SENT_BITS], dtype=np.uint32).view(F32)[0])


def _api():
    from rad_mmm_amd import _lib
    return _lib


def _sent(n):
    return torch.full((n,), SENT, dtype=torch.float32, device=DEV)


def _sent_np(*shape):
    return np.full(shape, SENT, dtype=F32)


def _dev(a, off=0):
    """a float32 copy of `a` on the device, as a flat view that starts `off` floats into its allocation"""
    a = np.ascontiguousarray(a, dtype=F32).reshape(-1)
    buf = torch.empty(a.size + off, dtype=torch.float32, device=DEV)
    buf[off:] = torch.from_numpy(a).to(DEV)
    return buf[off:]


def _ints(a):
    return torch.tensor(list(a), dtype=torch.int32, device=DEV)


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = _bits(got) != _bits(want)
    if bad.any():
        idx = np.argwhere(bad)[:6]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ in their bits, first at {idx.tolist()}: "
                             f"device {[float(got[tuple(i)]) for i in idx]} expected {[float(want[tuple(i)]) for i in idx]}")


def _assert_untouched(got, what):
    bad = _bits(got) != SENT_BITS
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements outside the written range changed, first at " \
                          f"{np.argwhere(bad)[:6].tolist()}"


def _ratio(err, scale):
    """max of err / scale; where scale is 0 the error has to be 0"""
    err, scale = np.broadcast_arrays(np.asarray(err, dtype=np.float64), np.asarray(scale, dtype=np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(scale > 0, err / scale, np.where(err == 0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0


def _assert_bound(got, ref, bound, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), ref.shape)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    bad = ~(err <= bound)                                 # (a NaN on either side is bad)
    norm = float(err.max() / (np.abs(ref).max() + 1e-300)) if err.size else 0.0
    print(f"{what}: max err / bound {_ratio(err, bound):.3f}, norm-wise rel err {norm:.2e}")
    if bad.any():
        idx = np.argwhere(bad)[:6]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements beyond their bound, first at {idx.tolist()}: device "
                             f"{[got[tuple(i)] for i in idx]} model {[ref[tuple(i)] for i in idx]} bound {[bound[tuple(i)] for i in idx]}")


def _up4(n):
    return (n + 3) // 4 * 4


# =====================================================================================================================
# weight norm fold and its gradient
# Which kernel radmmm_weightnorm_bwd launches (elementwise.hip, the launcher's conditions in its order):
#   Cin * taps * 4 > 48 KiB                                                        -> plain   weightnorm_bwd_kernel
#   vec := Cin, perm_split, off_lo, off_hi, ldw, split_stride all % 4 == 0 and dW, v, dv 16-byte aligned
#   vec and Cin <= 2048 and taps in {1, 3, 5}                                      -> reg<taps>  (unless RADMMM_WNBWD_REG=0)
#   vec                                                                            -> lds<true>
#   else                                                                           -> lds<false>
# Every case below has ldw = round_up(Cin, 4) + 8, a split stride of one slab + 12 floats and the permutations (0, 0, 0) and
# (8, ldw - 8, 0): all multiples of 4, and v, dv are fresh allocations, so vec is decided by Cin % 4 and the offset of dW:
#   reg<T>-Cin*      Cin in {4, 1024, 1028, 2048} % 4 == 0, <= 2048, T in {1, 3, 5}, Cin * T <= 10240 floats = 40 KiB: the
#                    register kernel; Cin > 1024 runs its second channel pass (j = 1), Cin = 1028 with one thread in it
#   lds-true-*       Cin % 4 == 0 but taps in {2, 7}, or Cin = 2052 > 2048 (8 KiB of LDS)
#   lds-false-*      Cin = 10 (not % 4); or Cin = 8, taps = 3 (register shape) with dW one float off 16-byte alignment
#   plain-*          Cin = 2460, taps = 5: 12300 floats > 12288
WN_CASES = [(f"reg<{t}>-Cin{c}", "reg", c, t, 0) for t in (1, 3, 5) for c in (4, 1024, 1028, 2048)] + [
    ("lds-true-taps2", "lds-true", 12, 2, 0), ("lds-true-taps7", "lds-true", 8, 7, 0),
    ("lds-true-Cin2052-taps1", "lds-true", 2052, 1, 0),
    ("lds-false-Cin10-taps5", "lds-false", 10, 5, 0), ("lds-false-dW-off-by-one-float", "lds-false", 8, 3, 1),
    ("plain-Cin2460-taps5", "plain", 2460, 5, 0)]


def _wn_branch(Cin, taps, ldw, perm, stride, dw_off):
    if Cin * taps * 4 > 48 * 1024:
        return "plain"
    vec = all(q % 4 == 0 for q in (Cin, ldw, stride) + tuple(perm)) and dw_off % 4 == 0
    if vec and Cin <= 2048 and taps in (1, 3, 5):
        return "reg"
    return "lds-true" if vec else "lds-false"


@pytest.mark.parametrize("branch,Cin,taps,dw_off", [pytest.param(*c[1:], id=c[0]) for c in WN_CASES])
def test_weightnorm_fwd_bwd(branch, Cin, taps, dw_off):
    """Bounds.  Forward: ss = sum v^2 has ceil(n / 256) serial fmas per thread and 12 shuffle levels (two 64-lane
    butterflies), all terms positive; sqrt, g / nrm and v * scale are three correctly rounded operations:
    |dW| <= (n_chain + 12 + 4) u |W|, the same for inv_norm.
    Backward: gw = the slabs added in order, (splits - 1) u sum|slab terms| =: e_gw.  dot = sum gw v: n_chain = 8 * taps fmas
    per thread in the register kernel (two passes of four channels, absent channels add zeros), ceil(n / 256) in the LDS and
    the plain kernel, 12 levels: e_dot = (n_chain + 12) u sum|gw v| + sum e_gw |v|.  dg = dot * inv + poison: |inv| e_dot + 2 u
    |dg|.  dv = a gw - b v with a = g inv (1 rounding), b = g dot inv^3 (4), two products and a difference (3):
    |a| e_gw + |g inv^3 v| e_dot + 8 u (|a gw| + |b v|)."""
    L = _api()
    rng = np.random.RandomState(Cin * 10 + taps)
    Cout, n = 3, Cin * taps
    ldw = _up4(Cin) + 8
    slab = taps * Cout * ldw
    stride = slab + 12
    v = rng.standard_normal((Cout, Cin, taps)).astype(F32)
    g = (rng.rand(Cout) + 0.5).astype(F32)
    vd, gd = _dev(v), _dev(g)
    nch_thread = -(-n // 256)
    for perm in (R.IDENTITY, (8, ldw - 8, 0)):
        assert _wn_branch(Cin, taps, ldw, perm, stride, dw_off) == branch
        cols = R.perm_col(np.arange(Cin), perm)
        hit = np.zeros(ldw, dtype=bool)
        hit[cols] = True
        # ---- forward
        Wd, invd = _sent(slab + 8), _sent(Cout + 8)
        L.check(L.lib.radmmm_weightnorm_fwd(L.ptr(vd), L.ptr(gd), L.ptr(Wd), L.ptr(invd), Cout, Cin, taps, ldw, *perm,
                                            L.stream()), "weightnorm_fwd")
        W, inv = _host(Wd), _host(invd)
        W_ref, inv_ref = R.weightnorm_fwd(v, g, ldw, perm)
        tag = f"weightnorm_fwd {branch} Cin {Cin} taps {taps} perm {perm}"
        _assert_untouched(W[slab:], tag + ": past W")
        _assert_untouched(inv[Cout:], tag + ": past inv_norm")
        Wm = W[:slab].reshape(taps, Cout, ldw)
        _assert_untouched(Wm[:, :, ~hit], tag + ": columns no col(ci) names")
        c_fwd = (nch_thread + 12 + 4) * U
        _assert_bound(Wm[:, :, hit], W_ref[:, :, hit], c_fwd * np.abs(W_ref[:, :, hit]), tag + ": W")
        _assert_bound(inv[:Cout], inv_ref, c_fwd * np.abs(inv_ref), tag + ": inv_norm")
        inv32 = inv_ref.astype(F32)                       # what the backward is given (and its model): exact inputs
        invd2 = _dev(inv32)
        # ---- backward
        for splits in (1, 2, 5):
            flat = (rng.standard_normal(splits * stride + dw_off + 4) * 100).astype(F32)      # gaps: values never to be read
            S = rng.standard_normal((splits, taps, Cout, ldw)).astype(F32)
            S[:, :, :, ~hit] = 1000.0
            for sp in range(splits):
                flat[dw_off + sp * stride: dw_off + sp * stride + slab] = S[sp].reshape(-1)
            dWd = _dev(flat[dw_off:], dw_off)
            gw, gw_abs = R.weightnorm_gather(S, Cin, perm)
            for poison in (None, 0.0, float("nan")):
                dvd, dgd = _sent(Cout * n + 8), _sent(Cout + 8)
                pd = None if poison is None else _dev([poison])
                L.check(L.lib.radmmm_weightnorm_bwd(L.ptr(vd), L.ptr(gd), L.ptr(invd2), L.ptr(dWd), splits, stride, L.ptr(dvd),
                                                    L.ptr(dgd), Cout, Cin, taps, ldw, *perm, L.ptr(pd), L.stream()),
                        "weightnorm_bwd")
                dv, dg = _host(dvd), _host(dgd)
                tag = f"weightnorm_bwd {branch} Cin {Cin} taps {taps} perm {perm} splits {splits} poison {poison}"
                _assert_untouched(dv[Cout * n:], tag + ": past dv")
                _assert_untouched(dg[Cout:], tag + ": past dg")
                dv_ref, dg_ref, t = R.weightnorm_bwd(v, g, inv32, gw, None)
                n_chain = 8 * taps if branch == "reg" else nch_thread
                e_gw = (splits - 1) * U * gw_abs
                e_dot = (n_chain + 12) * U * t["absdot"] + (e_gw * np.abs(v)).reshape(Cout, -1).sum(1)
                i64 = inv32.astype(np.float64)
                if poison is not None and math.isnan(poison):
                    assert np.isnan(dg[:Cout]).all(), tag + ": dg must be NaN"
                else:
                    _assert_bound(dg[:Cout], dg_ref, i64 * e_dot + 2 * U * np.abs(dg_ref), tag + ": dg")
                a, b = t["a"][:, None, None], t["b"][:, None, None]
                bound = np.abs(a) * e_gw + np.abs((g * i64 ** 3)[:, None, None] * v) * e_dot[:, None, None] \
                    + 8 * U * (np.abs(a * gw) + np.abs(b * v))
                _assert_bound(dv[:Cout * n].reshape(Cout, Cin, taps), dv_ref, bound, tag + ": dv")


# =====================================================================================================================
# WN input gradient scatter
def _wn_input_bwd_case(rng, rows, D, h, ldx0, ldctx, ldz, accum, off_z=0):
    L = _api()
    gX0 = rng.standard_normal((rows, ldx0)).astype(F32)
    gX0[:, D + h:] = 3.0                                          # values that must go nowhere: added to a sentinel, they show
    gctx0, gz0 = _sent_np(rows, ldctx), _sent_np(rows, ldz)
    gctx0[:, :D] = rng.standard_normal((rows, D))
    gz0[:, :h] = rng.standard_normal((rows, h))
    want_ctx, want_z = R.wn_input_bwd(gX0, gctx0, gz0, D, h, accum)   # float32 in: the kernel's single rounded additions
    gxd, gcd, gzd = _dev(gX0), _dev(gctx0), _dev(gz0, off_z)
    L.check(L.lib.radmmm_wn_input_bwd(L.ptr(gxd), ldx0, L.ptr(gcd), ldctx, accum, L.ptr(gzd), ldz, rows, D, h, L.stream()),
            "wn_input_bwd")
    tag = f"wn_input_bwd rows {rows} D {D} h {h} ldx0 {ldx0} ldz {ldz} accum {accum} gz offset {off_z}"
    _assert_bits(_host(gzd).reshape(rows, ldz), want_z, tag + ": gz (columns >= h untouched)")
    _assert_bits(_host(gcd).reshape(rows, ldctx), want_ctx, tag + ": gctx (columns >= D untouched)")


@pytest.mark.parametrize("h", [1, 2, 3, 4, 5, 79])
def test_wn_input_bwd_four_wide(h):
    """D, ldctx, ldz, ldx0 multiples of 4 and aligned bases: wn_input_bwd4_kernel; (D + h) % 4 runs through 1, 2, 3, 0"""
    rng = np.random.RandomState(h)
    D = 8
    for ldx0 in (_up4(D + h), _up4(D + h) + 8):
        for accum in (0, 1):
            _wn_input_bwd_case(rng, 5, D, h, ldx0, D + 4, _up4(h) + 4, accum)


@pytest.mark.parametrize("D,h,off_z", [(7, 5, 0), (8, 5, 1), (8, 4, 1)], ids=["D7", "gz-off-by-one-float", "gz-off-h4"])
def test_wn_input_bwd_scalar(D, h, off_z):
    rng = np.random.RandomState(D + h)
    for accum in (0, 1):
        _wn_input_bwd_case(rng, 5, D, h, _up4(D + h) + 4, D + 4, _up4(h) + 4, accum, off_z)


def test_wn_input_bwd_grid_stride():
    """rows * ceil((D + h) / 4) = 525 000 > 2048 * 256 work items: the grid-stride loop runs a second round"""
    _wn_input_bwd_case(np.random.RandomState(0), 175000, 8, 4, 12, 8, 8, 1)


# =====================================================================================================================
# affine coupling
def _coupling_inputs(rng, rows, h, ldz, ldo, su_draw):
    O = rng.standard_normal((rows, ldo)).astype(F32)
    O[:, :h] = su_draw((rows, h))
    O[:, 2 * h:] = 77.0                                           # beyond 2h: never read
    z, gzout = rng.standard_normal((rows, ldz)).astype(F32), rng.standard_normal((rows, ldz)).astype(F32)
    gl = rng.standard_normal((rows, h)).astype(F32)
    return O, z, gzout, gl


def _coupling_r32(O, z, gzout, gl, h, mode):
    """per-element error of the float32 CPU restatement against float64 on these inputs, relative to the added terms"""
    zout, ls, fm = R.coupling_fwd(O, z, h, mode)
    gsu, _, gz, bm = R.coupling_bwd(O, z, gzout, gl, h, mode)
    z32, l32 = R.coupling_fwd_f32(O, z, h, mode)
    s32, g32 = R.coupling_bwd_f32(O, z, gzout, gl, h, mode)
    sl = slice(h, 2 * h)
    return dict(zout1=_ratio(np.abs(z32[:, sl] - zout[:, sl]), fm["zout1"]), log_s=_ratio(np.abs(l32 - ls), fm["log_s"]),
                gsu=_ratio(np.abs(s32 - gsu), bm["gsu"]), gz1=_ratio(np.abs(g32[:, sl] - gz[:, sl]), bm["gz1"]))


def _coupling_run(O, z, gzout, gl, rows, h, ldz, ldo, mode):
    """both kernels on sentinel-filled outputs; the copies and the untouched ranges are checked here, the computed columns are
    returned: zout1, log_s, gsu, gz1"""
    L = _api()
    Od, zd, gd = _dev(O), _dev(z), _dev(gzout)
    gld = None if gl is None else _dev(gl)
    zoutd, lsd = _sent(rows * ldz + 8), _sent((rows + 2) * h)
    L.check(L.lib.radmmm_affine_coupling_fwd(L.ptr(Od), ldo, L.ptr(zd), ldz, L.ptr(zoutd), L.ptr(lsd[h:]), rows, h, mode,
                                             L.stream()), "affine_coupling_fwd")
    gOd, gzd = _sent(rows * ldo + 8), _sent(rows * ldz + 8)
    L.check(L.lib.radmmm_affine_coupling_bwd(L.ptr(Od), ldo, L.ptr(zd), ldz, L.ptr(gd), L.ptr(gld), L.ptr(gOd), L.ptr(gzd),
                                             rows, h, mode, L.stream()), "affine_coupling_bwd")
    zout, ls, gO, gz = _host(zoutd), _host(lsd).reshape(rows + 2, h), _host(gOd), _host(gzd)
    tag = f"coupling mode {mode} rows {rows} h {h} ldz {ldz} ldo {ldo} glog_s {gl is not None}"
    for name, a, n in (("zout", zout, rows * ldz), ("gO", gO, rows * ldo), ("gz", gz, rows * ldz)):
        _assert_untouched(a[n:], f"{tag}: past {name}")
    _assert_untouched(ls[[0, rows + 1]], tag + ": log_s outside its rows")
    zout, gO, gz = zout[:rows * ldz].reshape(rows, ldz), gO[:rows * ldo].reshape(rows, ldo), gz[:rows * ldz].reshape(rows, ldz)
    sl = slice(h, 2 * h)
    _assert_bits(zout[:, :h], z[:, :h], tag + ": zout[:, 0:h] is a copy")
    _assert_bits(zout[:, 2 * h:], z[:, 2 * h:], tag + ": zout[:, 2h:ldz] is a copy")
    _assert_bits(gz[:, :h], gzout[:, :h], tag + ": gz[:, 0:h] is a copy")
    _assert_bits(gz[:, 2 * h:], gzout[:, 2 * h:], tag + ": gz[:, 2h:ldz] is a copy")
    _assert_bits(gO[:, sl], gzout[:, sl], tag + ": gO[:, h:2h] is a copy")
    _assert_untouched(gO[:, 2 * h:], tag + ": gO[:, 2h:ldo]")
    return tag, dict(zout1=zout[:, sl], log_s=ls[1:rows + 1], gsu=gO[:, :h], gz1=gz[:, sl])


def _coupling_check(rng, rows, h, ldz, ldo, mode, with_gl):
    O, z, gzout, gl = _coupling_inputs(rng, rows, h, ldz, ldo, lambda s: rng.uniform(-4, 4, s))
    gl = gl if with_gl else None
    tag, got = _coupling_run(O, z, gzout, gl, rows, h, ldz, ldo, mode)
    zout, ls, fm = R.coupling_fwd(O, z, h, mode)
    gsu, _, gz, bm = R.coupling_bwd(O, z, gzout, gl, h, mode)
    r32 = _coupling_r32(O, z, gzout, gl, h, mode)
    sl = slice(h, 2 * h)
    for key, ref, mag in (("zout1", zout[:, sl], fm["zout1"]), ("log_s", ls, fm["log_s"]), ("gsu", gsu, bm["gsu"]),
                          ("gz1", gz[:, sl], bm["gz1"])):
        print(f"{tag}: {key}: float32 restatement {r32[key] / U:.2f} u of the added terms, device "
              f"{_ratio(np.abs(got[key] - ref), mag) / U:.2f} u, allowed {4 * r32[key] / U:.2f} u")
        _assert_bound(got[key], ref, 4 * r32[key] * mag, f"{tag}: {key}")


@pytest.mark.parametrize("h", [1, 5, 79])
@pytest.mark.parametrize("mode", [R.SCALE_TANH, R.SCALE_EXP, R.SCALE_SIGMOID, R.SCALE_TRANSLATE],
                         ids=["tanh", "exp", "sigmoid", "translate"])
def test_affine_coupling(mode, h):
    """su drawn from [-4, 4].  The tolerance is 4 x the measured error of the float32 CPU restatement on the same inputs,
    relative to the `mag` of the model (|tanh su| + 1 + 1e-6 for s, S / s + |log s| for log_s, ...).  Measured on the CPU for
    these inputs, in units of u = 2^-24 of the added terms (largest over h, ldz, ldo, glog_s), tanh / exp / sigmoid /
    translate: zout 2.40 / 2.09 / 2.44 / 1.00; log_s 1.61 / 0 (a copy) / 1.76 / 0; gO[:, 0:h] 2.02 / 2.28 / 0.72 / 0;
    gz[:, h:2h] 2.37 / 1.71 / 2.50 / 0 (gzout * 1).  The kernel gets 4 x the value of each run, which the test prints next to
    the device's."""
    rng = np.random.RandomState(100 * mode + h)
    for ldz in (2 * h, 2 * h + 3):
        for ldo in (2 * h, ldz + 2):
            for with_gl in (True, False):
                _coupling_check(rng, 7, h, ldz, ldo, mode, with_gl)


def test_affine_coupling_grid_stride():
    """rows * ldz = 525 200 > 2048 * 256: the grid-stride loops of both kernels run a second round"""
    _coupling_check(np.random.RandomState(5), 40400, 5, 13, 15, R.SCALE_TANH, True)


@pytest.mark.parametrize("mode", [R.SCALE_TANH, R.SCALE_EXP, R.SCALE_SIGMOID], ids=["tanh", "exp", "sigmoid"])
def test_affine_coupling_saturated(mode):
    """su in +-[8, 12]: tanh(su) + 1 + 1e-6 and the shifted sigmoid saturate in float32, as they do in the reference, so this
    case is judged against the float32 CPU restatement (never float64): finite, and within 4 x the error measured in the
    [-4, 4] case of the same shape, relative to the float64 magnitudes of the added terms on these inputs."""
    rng = np.random.RandomState(40 + mode)
    rows, h, ldz, ldo = 7, 5, 13, 15
    r32 = _coupling_r32(*_coupling_inputs(rng, rows, h, ldz, ldo, lambda s: rng.uniform(-4, 4, s)), h, mode)
    O, z, gzout, gl = _coupling_inputs(rng, rows, h, ldz, ldo, lambda s: rng.uniform(8, 12, s) * rng.choice([-1.0, 1.0], s))
    tag, got = _coupling_run(O, z, gzout, gl, rows, h, ldz, ldo, mode)
    _, _, fm = R.coupling_fwd(O, z, h, mode)
    _, _, _, bm = R.coupling_bwd(O, z, gzout, gl, h, mode)
    z32, l32 = R.coupling_fwd_f32(O, z, h, mode)
    s32, g32 = R.coupling_bwd_f32(O, z, gzout, gl, h, mode)
    sl = slice(h, 2 * h)
    for key, ref, mag in (("zout1", z32[:, sl], fm["zout1"]), ("log_s", l32, fm["log_s"]), ("gsu", s32, bm["gsu"]),
                          ("gz1", g32[:, sl], bm["gz1"])):
        assert np.isfinite(got[key]).all() and np.isfinite(ref).all(), f"{tag}: {key} not finite"
        _assert_bound(got[key], ref, 4 * r32[key] * mag, f"{tag} saturated: {key} against the float32 restatement")


# =====================================================================================================================
# dact_mul, fp32 outputs
_SOFTPLUS_EDGES = [19.999998, 20.0, 20.000002, 25.0, 1e-6, 2e-6, 0.24999999, 0.25, 0.25000003, 0.0]


@pytest.mark.parametrize("rowscale", [0, 1, 2])
@pytest.mark.parametrize("dact", [R.ACT_NONE, R.ACT_SOFTPLUS, R.ACT_RELU, R.ACT_LEAKY], ids=["none", "softplus", "relu", "leaky"])
def test_dact_mul(dact, rowscale):
    """cols 4 (ld 8: vector loop; ld 5: scalar loop), 6 (scalar), 160 (vector).  Without the softplus derivative and with row
    weights 0 / 1 the result is (g * act') * w, one rounded product at most: bit for bit.  Otherwise per element against
    float64: |g| w (4 r32 mag + c u |act'|), r32 the measured error of the float32 CPU restatement of the softplus derivative
    on these saved values relative to mag (y below 0.25, 1 + exp(-y) above, 1 above 20; measured 1.46 u at most), c = 2 for the two products, + 2
    for the ratio's addition and division with rowscale 2."""
    L = _api()
    rng = np.random.RandomState(10 * dact + rowscale)
    B, T, lens = 3, 7, [0, 1, 7]
    rows = B * T
    lensd = _ints(lens)
    for cols, ld in ((4, 8), (4, 5), (6, 8), (160, 164)):
        for taps, dil in (((1, 1), (3, 1), (5, 4)) if rowscale == 2 else ((1, 1),)):
            g = rng.standard_normal((rows, ld)).astype(F32)
            if dact == R.ACT_SOFTPLUS:
                saved = (np.abs(rng.standard_normal((rows, ld))) * 3).astype(F32)
                for r in (0, 7, 14):                              # first frames of the items of length 0, 1 and 7
                    for j, e in enumerate(_SOFTPLUS_EDGES):
                        saved[r + j // cols, j % cols] = e
            else:
                saved = rng.standard_normal((rows, ld)).astype(F32)
                saved[rng.rand(rows, ld) < 0.2] = 0.0
                if dact == R.ACT_RELU:
                    saved = np.maximum(saved, 0)
            yd, gd, sd = _sent(rows * ld + 8), _dev(g), _dev(saved)
            L.check(L.lib.radmmm_dact_mul(L.ptr(gd), ld, L.ptr(sd) if dact else None, ld, L.ptr(yd), ld, rows, cols,
                                          dact, rowscale, T, L.ptr(lensd), taps, dil, None, None, 0, 1.0, None, L.stream()),
                    "dact_mul")
            y = _host(yd)
            tag = f"dact_mul dact {dact} rowscale {rowscale} cols {cols} ld {ld} taps {taps} dil {dil}"
            _assert_untouched(y[rows * ld:], tag + ": past y")
            y = y[:rows * ld].reshape(rows, ld)
            _assert_untouched(y[:, cols:], tag + ": y[:, cols:ld]")
            w = R.dact_row_weight(rowscale, T, lens, taps, dil)
            d = R.dact_from_out(saved[:, :cols], dact)
            if rowscale <= 1 and dact != R.ACT_SOFTPLUS:
                want = (g[:, :cols] * d.astype(F32)) * w.astype(F32)[:, None]
                _assert_bits(y[:, :cols], want, tag)
                continue
            ref = R.dact_mul(g[:, :cols], saved[:, :cols], dact, w)
            tail = (2 + 2 * (rowscale == 2)) * U * np.abs(d)
            if dact == R.ACT_SOFTPLUS:
                mag = R.dsoftplus_mag(saved[:, :cols])
                r32 = _ratio(np.abs(R.dsoftplus_from_out_f32(saved[:, :cols]) - d), mag)
                dev_d = _ratio(np.abs(y[:, :cols] - ref), np.abs(g[:, :cols]) * w[:, None] * mag)
                print(f"{tag}: softplus': float32 restatement {r32 / U:.2f} u of mag, device (with its products) {dev_d / U:.2f} u, "
                      f"allowed {4 * r32 / U:.2f} u of mag + {2 + 2 * (rowscale == 2)} u of |act'|")
                tail = tail + 4 * r32 * mag
            _assert_bound(y[:, :cols], ref, np.abs(g[:, :cols]) * w[:, None] * tail, tag)
            _assert_bits(y[w == 0, :cols], g[w == 0, :cols] * F32(0), tag + ": masked rows are exact zeros")


# =====================================================================================================================
# column sums
def _exact_ints(rng, *shape):
    """non-zero integers in [-8, 8] / 8: float32 adds thousands of them, or of their squares, exactly in any order"""
    return (rng.randint(1, 9, shape) * rng.choice([-1, 1], shape) / 8.0).astype(F32)


def _colsum_dev(X, ldx, rows, cols, row_weight, T, lens, taps, dil, square, off=0):
    L = _api()
    nsc = int(L.lib.radmmm_colsum_scratch_floats(rows, cols))
    assert nsc == R.colsum_scratch_floats(rows, cols)
    outd, scd, Xd = _sent(cols + 8), _sent(nsc + 16), _dev(X, off)
    lensd = None if lens is None else _ints(lens)
    L.check(L.lib.radmmm_colsum(L.ptr(Xd), ldx, L.ptr(outd), L.ptr(scd), rows, cols, row_weight, T, L.ptr(lensd), taps, dil,
                                square, L.stream()), "colsum")
    out, sc = _host(outd), _host(scd)
    _assert_untouched(out[cols:], "colsum: past out")
    _assert_untouched(sc[nsc:], "colsum: past the scratch radmmm_colsum_scratch_floats asks for")
    return out[:cols]


@pytest.mark.parametrize("cols", [1, 3, 4, 100, 160, 516, 1024, 1025, 1028])
def test_colsum_exact(cols):
    """rows 130 = 5 items of 26 frames (three row blocks, the last of 2 rows), weights 0 and 1, with and without the square, on
    an aligned pitch, on X one float off 16-byte alignment and on a pitch that is no multiple of 4 (both scalar loads).  cols
    <= 512 packs 256 / ceil(cols / 4) row lanes into a workgroup (cols 100: 10 lanes and 6 idle threads); cols > 1024 has a
    second slab of 1, 4 columns."""
    rng = np.random.RandomState(cols)
    B, T, lens = 5, 26, [26, 0, 1, 13, 25]
    rows = B * T
    lda = _up4(cols) + 4
    ldo = cols + 1 if (cols + 1) % 4 else cols + 2
    for ldx, off in ((lda, 0), (lda, 1), (ldo, 0)):
        X = _exact_ints(rng, rows, ldx)
        X[:, cols:] = 1000.0
        for row_weight in (0, 1):
            for square in (0, 1):
                out = _colsum_dev(X, ldx, rows, cols, row_weight, T, lens, 1, 1, square, off)
                want, _ = R.colsum(X[:, :cols], R.colsum_row_weight(row_weight, T, lens), bool(square))
                _assert_bits(out, want.astype(F32), f"colsum cols {cols} ldx {ldx} off {off} weight {row_weight} square {square}")


@pytest.mark.parametrize("rows,cols", [(4095, 512), (4096, 508), (4096, 512)])
def test_colsum_rows_per_block(rows, cols):
    """16 rows per block from rows >= 4096 and cols >= 512, 64 below either; the scratch size follows (checked against the
    model's count in _colsum_dev)"""
    rng = np.random.RandomState(rows + cols)
    X = _exact_ints(rng, rows, cols)
    assert R.colsum_scratch_floats(rows, cols) == (256 if (rows, cols) == (4096, 512) else 64) * cols
    for row_weight, lens in ((0, None), (1, [rows - 7])):
        out = _colsum_dev(X, cols, rows, cols, row_weight, rows, lens, 1, 1, 0)
        want, _ = R.colsum(X, R.colsum_row_weight(row_weight, rows, lens, B=1))
        _assert_bits(out, want.astype(F32), f"colsum rows {rows} cols {cols} weight {row_weight}")


@pytest.mark.parametrize("cols", [3, 160, 1028])
@pytest.mark.parametrize("taps,dil", [(3, 1), (5, 4)])
def test_colsum_weight2_ragged(cols, taps, dil):
    """row weight 2 = [t < len] (cnt + 1e-6) / taps on random data against float64.  Per column: a row lane adds
    ceil(64 / nrl) rows by fma (nrl = 256 / column groups of the slab), lane 0 adds the nrl - 1 other lanes, the final kernel
    adds ceil(nparts / 16) partials per wave, two levels of (s0 + s1) + (s2 + s3) and 16 waves; c = 3 for the weight (an
    addition, a division) and the square: (n_lane + nrl - 1 + n_final + 18 + 3) u sum |w x|."""
    rng = np.random.RandomState(cols + taps)
    B, T, lens = 5, 26, [26, 0, 1, 13, 25]
    rows, ldx = B * T, _up4(cols) + 4
    X = rng.standard_normal((rows, ldx)).astype(F32)
    nparts = -(-rows // 64)
    span = np.minimum(cols - np.arange(cols) // 1024 * 1024, 1024)
    nrl = 256 // -(-span // 4)
    levels = -(-64 // nrl) + nrl - 1 + -(-nparts // 16) + 18 + 3
    for square in (0, 1):
        out = _colsum_dev(X, ldx, rows, cols, 2, T, lens, taps, dil, square)
        want, a = R.colsum(X[:, :cols], R.colsum_row_weight(2, T, lens, taps, dil), bool(square))
        _assert_bound(out, want, levels * U * a, f"colsum weight 2 cols {cols} taps {taps} dil {dil} square {square}")


NPARTS = [1, 15, 16, 17, 33, 49, 64, 65, 113]


@pytest.mark.parametrize("nparts", NPARTS)
def test_colsum_final_exact(nparts):
    L = _api()
    rng = np.random.RandomState(nparts)
    for cols in (1, 63, 64, 65):
        part = np.concatenate((_exact_ints(rng, nparts * cols), np.full(64, 1000.0, dtype=F32)))
        outd, partd = _sent(cols + 8), _dev(part)
        L.check(L.lib.radmmm_colsum_final(L.ptr(partd), L.ptr(outd), nparts, cols, L.stream()), "colsum_final")
        out = _host(outd)
        _assert_untouched(out[cols:], f"colsum_final nparts {nparts} cols {cols}: past out")
        want = part[:nparts * cols].reshape(nparts, cols).astype(np.float64).sum(0).astype(F32)
        _assert_bits(out[:cols], want, f"colsum_final nparts {nparts} cols {cols}")


def test_colsum_final_multi_17_items():
    """17 items = two launches (16 + 1); cols 5 next to cols 130: the narrow items' second and third workgroups return early"""
    L = _api()
    rng = np.random.RandomState(17)
    items, keep = (L.CsItem * 17)(), []
    for i in range(17):
        nparts, cols = NPARTS[i % len(NPARTS)], (5, 130, 64)[i % 3]
        part = np.concatenate((_exact_ints(rng, nparts * cols), np.full(64, 1000.0, dtype=F32)))
        pd, od = _dev(part), _sent(cols + 8)
        keep.append((part, pd, od, nparts, cols))
        items[i].part, items[i].out, items[i].nparts, items[i].cols = L.ptr(pd), L.ptr(od), nparts, cols
    L.check(L.lib.radmmm_colsum_final_multi(items, 17, L.stream()), "colsum_final_multi")
    for i, (part, _, od, nparts, cols) in enumerate(keep):
        out = _host(od)
        _assert_untouched(out[cols:], f"colsum_final_multi item {i}: past out")
        want = part[:nparts * cols].reshape(nparts, cols).astype(np.float64).sum(0).astype(F32)
        _assert_bits(out[:cols], want, f"colsum_final_multi item {i} nparts {nparts} cols {cols}")


# =====================================================================================================================
# masked reductions
@pytest.mark.parametrize("layout", ["contiguous", "channels-last-view"])
@pytest.mark.parametrize("B,C,T,lens", [(3, 160, 300, [300, 0, 137]), (3, 160, 300, None), (1, 1, 7, [5]), (1, 7, 1, None)],
                         ids=["144000-ragged", "144000-full", "7-ragged", "7-full"])
def test_masked_reduce_and_bwd(B, C, T, lens, layout):
    """144 000 elements: 512 workgroups (the MR_BLOCKS cap) and a second round of the grid stride.  channels-last-view is the
    [B, C, T] view of a [B, T, C] tensor (sc = 1 < st = C).  Exactly summable values: both sums are exact; the gradient is one
    rounded product: bit for bit."""
    L = _api()
    rng = np.random.RandomState(B * C + T)
    x = _exact_ints(rng, B, C, T)                                 # logical [B][C][T], non-zero everywhere
    total = B * C * T
    if layout == "contiguous":
        mem, strides = x, (C * T, T, 1)
    else:
        mem, strides = np.ascontiguousarray(x.transpose(0, 2, 1)), (T * C, 1, C)
    xd = _dev(mem)
    lensd = None if lens is None else _ints(lens)
    nsc = int(L.lib.radmmm_masked_reduce_scratch_floats(B, C, T))
    for mode in (0, 1):
        outd, scd = _sent(8), _sent(nsc + 16)
        L.check(L.lib.radmmm_masked_reduce(L.ptr(xd), B, C, T, *strides, L.ptr(lensd), mode, L.ptr(outd[4:]), L.ptr(scd),
                                           L.stream()), "masked_reduce")
        out, sc = _host(outd), _host(scd)
        tag = f"masked_reduce {B}x{C}x{T} {layout} lens {lens} mode {mode}"
        _assert_untouched(out[[0, 1, 2, 3, 5, 6, 7]], tag + ": around out")
        _assert_untouched(sc[nsc:], tag + ": past the scratch")
        _assert_bits(out[4:5], np.array([R.masked_reduce(x, lens, mode)], dtype=F32), tag)
        coef = F32(0.37)
        xr = rng.standard_normal((B, C, T)).astype(F32)           # the gradient takes any values
        memr = xr if layout == "contiguous" else np.ascontiguousarray(xr.transpose(0, 2, 1))
        gxd, xrd, coefd = _sent(total + 8), _dev(memr), _dev([coef])
        L.check(L.lib.radmmm_masked_reduce_bwd(L.ptr(xrd), B, C, T, *strides, L.ptr(lensd), mode, L.ptr(coefd), L.ptr(gxd),
                                               L.stream()), "masked_reduce_bwd")
        gx = _host(gxd)
        _assert_untouched(gx[total:], tag + ": past gx")
        gx = gx[:total].reshape(B, C, T) if layout == "contiguous" else gx[:total].reshape(B, T, C).transpose(0, 2, 1)
        _assert_bits(gx, R.masked_reduce_bwd(xr, lens, mode, coef), tag + ": gradient")


# =====================================================================================================================
# masked instance norm
@pytest.mark.parametrize("lens", [[9, 0, 1, 3], None], ids=["ragged", "full"])
@pytest.mark.parametrize("C", [1, 64, 65, 130])
def test_instnorm_fwd_bwd(C, lens):
    """B 4, T 9, pitch C + 3; weight / bias present and NULL; relu 0 and 1 (bias -0.3: about half the outputs clamp to exactly
    0, and the backward is given the kernel's own y, as the caller does).
    Bounds, n = len, n_chain = ceil(len / 4) additions per row lane, 2 combine levels:
      mean   e_mu = (n_chain + 2 + 1) u sum|x| / n                                        (the sum and the division)
      rstd   d = x - mu: e_d = e_mu + u |d|;  q = sum d^2: e_q = sum 2 |d| e_d + (n_chain + 2) u q;  var = q / n:
             e_var = e_q / n + u var;  e_rs = rs (e_var + u (var + eps)) / (2 (var + eps)) + 2 u rs   (rsqrtf within 1 ulp)
      y      |w| (rs e_d + |d| e_rs) + 4 u (|d rs w| + |b|)              (two products, the bias addition, one to spare)
      db     (n_chain + 2) u sum|g|;   dw  (n_chain + 2 + 2) u sum|g xhat|  (xhat carries two roundings)
      gx     rs |w| / n (e_db + |xhat| e_dw) + 8 u rs (|g w| + |m1| + |xhat m2|): m1, m2 two roundings each, xhat two, one
             product, two differences, the product with rs -- at most 8 on any term."""
    L = _api()
    rng = np.random.RandomState(C)
    B, T, ld, eps = 4, 9, C + 3, 1e-5
    rows = B * T
    ll = np.array([T] * B if lens is None else lens)
    lensd = None if lens is None else _ints(lens)
    x = np.full((rows, ld), 55.0, dtype=F32)
    x[:, :C] = rng.standard_normal((rows, C)) + 0.5
    gy = rng.standard_normal((rows, ld)).astype(F32)
    xd, gyd = _dev(x), _dev(gy)
    x3, gy3 = x.reshape(B, T, ld)[:, :, :C], gy.reshape(B, T, ld)[:, :, :C]
    nch = np.maximum(-(-ll // 4), 1)[:, None]                     # [B][1]
    n = np.maximum(ll, 1)[:, None].astype(np.float64)
    m = R.length_mask(T, lens, B)[:, :, None]
    for affine in (True, False):
        w = (rng.standard_normal(C) * 0.5 + 1).astype(F32) if affine else None
        b = np.full(C, -0.3, dtype=F32) if affine else None
        for relu in (0, 1):
            yd, meand, rstdd = _sent(rows * ld + 8), _sent(B * C + 8), _sent(B * C + 8)
            wd, bd = None if w is None else _dev(w), None if b is None else _dev(b)
            L.check(L.lib.radmmm_instnorm_fwd(L.ptr(xd), ld, L.ptr(wd), L.ptr(bd), L.ptr(yd), ld, L.ptr(meand), L.ptr(rstdd),
                                              L.ptr(lensd), B, T, C, eps, relu, L.stream()), "instnorm_fwd")
            y, mean, rstd = _host(yd), _host(meand), _host(rstdd)
            tag = f"instnorm C {C} lens {lens} affine {affine} relu {relu}"
            for name, a, k in (("y", y, rows * ld), ("mean", mean, B * C), ("rstd", rstd, B * C)):
                _assert_untouched(a[k:], f"{tag}: past {name}")
            y, mean, rstd = y[:rows * ld].reshape(B, T, ld), mean[:B * C].reshape(B, C), rstd[:B * C].reshape(B, C)
            _assert_untouched(y[:, :, C:], tag + ": y[:, C:ld]")
            y_ref, mean_ref, rstd_ref = R.instnorm_fwd(x3, w, b, lens, eps, relu)
            ww = np.ones(C) if w is None else w.astype(np.float64)
            bb = np.zeros(C) if b is None else b.astype(np.float64)
            e_mu = (nch + 3) * U * (np.abs(x3) * m).sum(1) / n
            d = (x3 - mean_ref[:, None]) * m
            e_d = (e_mu[:, None] + U * np.abs(d)) * m
            q = (d * d).sum(1)
            var = q / n
            e_var = ((2 * np.abs(d) * e_d).sum(1) + (nch + 2) * U * q) / n + U * var
            e_rs = rstd_ref * (e_var + U * (var + eps)) / (2 * (var + eps)) + 2 * U * rstd_ref
            _assert_bound(mean, mean_ref, e_mu, tag + ": mean")
            _assert_bound(rstd, rstd_ref, e_rs, tag + ": rstd")
            e_y = np.abs(ww) * (rstd_ref[:, None] * e_d + np.abs(d) * e_rs[:, None]) \
                + 4 * U * (np.abs(d * rstd_ref[:, None] * ww) + np.abs(bb)) * m
            _assert_bound(y[:, :, :C], y_ref, e_y, tag + ": y")
            for i in range(B):
                _assert_bits(y[i, ll[i]:, :C], np.zeros((T - ll[i], C), dtype=F32), f"{tag}: item {i}: frames >= len are +0")
            if relu and affine:
                share = float((y_ref[m[:, :, 0] > 0] == 0).mean())
                assert 0.2 < share < 0.9, f"{tag}: {share:.2f} of the valid outputs are clamped"   # (the inputs' doing)
            # ---- backward, from the kernel's own y / mean / rstd
            gxd, dwd, dbd = _sent(rows * ld + 8), _sent(B * C + 8), _sent(B * C + 8)
            L.check(L.lib.radmmm_instnorm_bwd(L.ptr(gyd), ld, L.ptr(xd), ld, L.ptr(yd), ld, L.ptr(wd), L.ptr(meand), L.ptr(rstdd), L.ptr(gxd), ld, L.ptr(dwd), L.ptr(dbd), L.ptr(lensd),
                                              B, T, C, relu, L.stream()), "instnorm_bwd")
            gx, dw, db = _host(gxd), _host(dwd), _host(dbd)
            for name, a, k in (("gx", gx, rows * ld), ("dw_part", dw, B * C), ("db_part", db, B * C)):
                _assert_untouched(a[k:], f"{tag}: past {name}")
            gx, dw, db = gx[:rows * ld].reshape(B, T, ld), dw[:B * C].reshape(B, C), db[:B * C].reshape(B, C)
            _assert_untouched(gx[:, :, C:], tag + ": gx[:, C:ld]")
            gx_ref, dw_ref, db_ref, t = R.instnorm_bwd(gy3, x3, y[:, :, :C], w, mean, rstd, lens, relu)
            e_db, e_dw = (nch + 2) * U * t["absdb"], (nch + 4) * U * t["absdw"]
            _assert_bound(db, db_ref, e_db, tag + ": db_part")
            _assert_bound(dw, dw_ref, e_dw, tag + ": dw_part")
            rs = rstd.astype(np.float64)[:, None]
            e_gx = rs * np.abs(ww) / t["n"] * (e_db[:, None] + np.abs(t["xh"]) * e_dw[:, None]) \
                + 8 * U * rs * (np.abs(t["g"] * ww) + np.abs(t["m1"]) + np.abs(t["xh"] * t["m2"]))
            _assert_bound(gx[:, :, :C], gx_ref, e_gx * m, tag + ": gx")
            for i in range(B):
                _assert_bits(gx[i, ll[i]:, :C], np.zeros((T - ll[i], C), dtype=F32), f"{tag}: item {i}: gx at frames >= len is +0")
