"""The two kernels of csrc/vocoder_bwd.hip called directly through the C ABI against the host models of
tests/_vocoder_bwd_ref.py, and the backward of the polyphase transposed conv as a unit against float64
conv_transpose1d autograd.

The cases, their inputs, the comparison functions and the bars are those of _vocoder_bwd_ref.py (bars: its docstring);
tests/test_vocoder_bwd_cpu.py shows on the CPU that the models agree with torch autograd and that the planted bugs do
not.  Rows at or past an item's length hold NaN in every input a kernel must not read there, padding columns hold NaN in
the inputs and a sentinel in the outputs, every case is ragged and runs again with lens = NULL.  radmmm_voc_lrelu_bwd
is held to the float32 model bit for bit, radmmm_voc_conv_post_bwd to n * 2^-23 * sum |terms|; both are launched twice
and must repeat their bits.  Every case prints its worst ratio to its bar (pytest -s)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _vocoder_bwd_ref as K
from _gemm_ref import accumulation_bar

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN = float("nan")


def _lib():
    from rad_mmm_amd._lib import check, lib, ptr, stream
    return check, lib, ptr, stream()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _lens(lens):
    return None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)


def _ids(cases):
    return [K.case_id(c) for c in cases]


MODES = pytest.mark.parametrize("use_lens", [True, False], ids=["lens", "null"])


# ---- radmmm_voc_lrelu_bwd ---------------------------------------------------------------------------------------------

def _run_lrelu_bwd(c, inp):
    check, lib, ptr, s = _lib()
    rows, lens = inp["gy"].shape[0], _lens(inp["lens"])
    gy, a = _dev(inp["gy"]), _dev(inp["a"])
    gx = gy if c["inplace"] else _dev(inp["gx0"])
    check(lib.radmmm_voc_lrelu_bwd(ptr(gy), c["ldgy"], ptr(a), c["lda"], ptr(gx), c["ldgx"], rows, c["C"], c["T"],
                                   ptr(lens), c["div"], c["slope"], int(c["accum"]), s), "voc_lrelu_bwd")
    return gx.cpu().numpy()


@MODES
@pytest.mark.parametrize("c", K.LRELU_BWD_CASES, ids=_ids(K.LRELU_BWD_CASES))
def test_lrelu_bwd(c, use_lens):
    inp = K.lrelu_bwd_inputs(c, use_lens)
    got = _run_lrelu_bwd(c, inp)
    K.lrelu_bwd_check(c, inp, got)
    assert K.bit_equal(got, _run_lrelu_bwd(c, inp)).all(), "two launches differ"


def test_lrelu_bwd_refuses_bad_arguments():
    from rad_mmm_amd._lib import lib
    x = torch.zeros(8, 8, device=DEV)
    p = x.data_ptr()
    for args in ((p, 8, p, 8, p, 8, 8, 6, 4, None, 1.0, 0.1, 0),          # cols % 4
                 (p, 8, p, 8, p, 8, 8, 8, 3, None, 1.0, 0.1, 0),          # rows % T
                 (p, 8, p, 4, p, 8, 8, 8, 4, None, 1.0, 0.1, 0),          # lda < cols
                 (p, 8, p, 8, p, 8, 8, 8, 4, None, 0.0, 0.1, 0),          # div
                 (p + 4, 8, p, 8, p, 8, 4, 4, 4, None, 1.0, 0.1, 0),      # alignment
                 (None, 8, p, 8, p, 8, 8, 8, 4, None, 1.0, 0.1, 0)):
        assert lib.radmmm_voc_lrelu_bwd(*args, None) == -1
    assert not x.any()


# ---- radmmm_voc_conv_post_bwd -----------------------------------------------------------------------------------------

def _run_post_bwd(c, inp):
    check, lib, ptr, s = _lib()
    rows, lens = inp["x"].shape[0], _lens(inp["lens"])
    x, w, audio, g = _dev(inp["x"]), _dev(inp["w"]), _dev(inp["audio"]), _dev(inp["g"])
    dx = torch.full((rows, c["lddx"]), 7.0, device=DEV)
    dw = torch.full((c["taps"], c["ldw"]), NAN, device=DEV)
    db = torch.full((1,), NAN, device=DEV)
    n = int(lib.radmmm_voc_conv_post_bwd_scratch_floats(rows, c["C"], c["taps"], c["ldw"]))
    assert n > 0
    scratch = torch.full((n,), NAN, device=DEV)
    check(lib.radmmm_voc_conv_post_bwd(ptr(x), c["ldx"], ptr(w), c["ldw"], ptr(audio), ptr(g), ptr(dx), c["lddx"],
                                       ptr(dw), ptr(db), ptr(scratch), rows, c["C"], c["taps"], c["T"], ptr(lens),
                                       c["div"], c["slope"], s), "voc_conv_post_bwd")
    return dx.cpu().numpy(), dw.cpu().numpy(), db.cpu().numpy()


@MODES
@pytest.mark.parametrize("c", K.POST_BWD_CASES, ids=_ids(K.POST_BWD_CASES))
def test_conv_post_bwd(c, use_lens):
    inp = K.post_bwd_inputs(c, use_lens)
    got = _run_post_bwd(c, inp)
    K.post_bwd_check(c, inp, *got)
    again = _run_post_bwd(c, inp)
    assert all(K.bit_equal(a, b).all() for a, b in zip(got, again)), "two launches differ"


def test_conv_post_bwd_refuses_bad_arguments():
    from rad_mmm_amd._lib import lib
    x = torch.zeros(8, 8, device=DEV)
    p = x.data_ptr()
    assert lib.radmmm_voc_conv_post_bwd_scratch_floats(8, 6, 7, 8) == 0
    assert lib.radmmm_voc_conv_post_bwd_scratch_floats(8, 1028, 7, 1028) == 0
    for args in ((p, 8, p, 8, p, p, p, 8, p, p, p, 8, 6, 7, 4, None, 1.0, 0.01),      # C % 4
                 (p, 8, p, 8, p, p, p, 8, p, p, p, 8, 8, 9, 4, None, 1.0, 0.01),      # taps > 7
                 (p, 8, p, 8, p, p, p, 8, p, p, p, 8, 8, 4, 4, None, 1.0, 0.01),      # taps even
                 (p, 8, p, 4, p, p, p, 8, p, p, p, 8, 8, 7, 4, None, 1.0, 0.01),      # ldw < C
                 (p, 8, p, 8, p, p, p, 8, p, p, p, 8, 8, 7, 3, None, 1.0, 0.01),      # rows % T
                 (p, 8, p, 8, p, p, p, 8, p, p, None, 8, 8, 7, 4, None, 1.0, 0.01)):  # no scratch
        assert lib.radmmm_voc_conv_post_bwd(*args, None) == -1
    assert not x.any()


# ---- the transposed conv's backward as a unit -------------------------------------------------------------------------

@pytest.mark.parametrize("k,u", [(16, 8), (8, 4), (4, 2)])
def test_convtranspose_grads_against_float64_autograd(k, u):
    """ConvTranspose1d(8, 4, k, u, (k - u) // 2) on ragged items, one of one frame: the data gradient (one row GEMM over
    the packed polyphase weight), the un-packed weight gradient and the bias gradient against conv_transpose1d autograd
    in float64, item by item at its own length.  Bars: accumulation_bar over the products each output sums (the row
    GEMM's u * Cout * taps per element, the weight gradient's valid rows, the bias gradient's valid output rows), with
    sum |terms| from the same autograd on absolute values.  Operand rows at or past a length hold NaN; the gradient rows
    there are zeros, as the generator's own kernels leave them."""
    from rad_mmm_amd.vocoder import convtranspose_grads, pack_polyphase
    Cin, Cout, T, lens, p = 8, 4, 5, [5, 1, 3], (k - u) // 2
    g = torch.Generator().manual_seed(100 + k)
    w = torch.randn(Cin, Cout, k, generator=g) / (Cin * k / u) ** 0.5
    R = T * len(lens)
    a = torch.randn(R, Cin, generator=g)
    gy = torch.randn(R * u, Cout, generator=g)
    valid = torch.tensor([t < n for n in lens for t in range(T)])
    a_dev = a.clone()
    a_dev[~valid] = NAN
    gy[~valid.repeat_interleave(u)] = 0.0
    Wp = pack_polyphase(w.to(DEV), u, p).contiguous()
    gw, gb, ga = convtranspose_grads(gy.to(DEV), a_dev.to(DEV), Wp, k, u, R, T, _lens(lens))
    gw2, gb2, ga2 = convtranspose_grads(gy.to(DEV), a_dev.to(DEV), Wp, k, u, R, T, _lens(lens))
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2) and torch.equal(ga, ga2)

    def autograd(w_, a_, gy_):
        w_ = w_.double().requires_grad_(True)
        b_ = torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
        da = torch.zeros(R, Cin, dtype=torch.float64)
        for b, n in enumerate(lens):
            x = a_[b * T:b * T + n].double().t()[None].requires_grad_(True)
            y = F.conv_transpose1d(x, w_, b_, stride=u, padding=p)[0]                    # [Cout, n * u]
            y.backward(gy_[b * T * u:(b * T + n) * u].double().t())
            da[b * T:b * T + n] = x.grad[0].t()
        return w_.grad, b_.grad, da

    want = autograd(w, a, gy)
    mag = autograd(w.abs(), a.abs(), gy.abs())
    n_rows = sum(lens)
    taps = Wp.shape[0]
    for name, got, ref, m, n in (("weight", gw, want[0], mag[0], n_rows), ("bias", gb, want[1], mag[1], n_rows * u),
                                 ("data", ga, want[2], mag[2], taps * u * Cout)):
        err = (got.double().cpu() - ref).abs()
        bar = accumulation_bar(n, m)
        assert bool((err[bar == 0] == 0).all()), name
        ratio = float((err / bar.clamp_min(1e-300))[bar > 0].max())
        print(f"convtranspose k={k} u={u} {name} gradient: worst |hip - f64| / bar {ratio:.3f}")
        assert ratio <= 1.0, (name, ratio)
    assert not ga[~valid.to(DEV)].any()
