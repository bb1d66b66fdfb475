"""The six kernels of csrc/vocoder.hip and the framed reads of radmmm_rowgemm_f32, called directly through the C ABI
and compared with the numpy restatements of tests/_vocoder_kernels_ref.py (float64, and float32 where the kernel is one
or two IEEE operations per element and must agree bit for bit).

The cases, their inputs, the comparison functions and the bars are those of _vocoder_kernels_ref.py (bars: its
docstring); tests/test_vocoder_cpu.py shows on the CPU that each of them rejects the named wrong variants.  Output
buffers are pre-filled with NaN, input rows at or past an item's length hold NaN wherever the kernel promises not to
use them, every case is ragged and runs again with lens = NULL where the ABI allows that.  Every case prints its worst
ratio to its bar (pytest -s)."""
import numpy as np
import pytest
import torch

import _vocoder_kernels_ref as K

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN = float("nan")


def _lib():
    from rad_mmm_amd._lib import check, lib, ptr, stream
    return check, lib, ptr, stream()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# Every device tensor handed to a kernel is held in a local until the result has been copied back: a temporary would be
# returned to the caching allocator, and reused by the next allocation, before the launch.
def _lens(lens):
    return None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)


def _ids(cases):
    return [K.case_id(c) for c in cases]


MODES = pytest.mark.parametrize("use_lens", [True, False], ids=["lens", "null"])


# ---- radmmm_voc_lrelu -------------------------------------------------------------------------------------------------

def _run_lrelu(c, inp, x, y):
    check, lib, ptr, s = _lib()
    rows, lens = inp["x"].shape[0], _lens(inp["lens"])
    check(lib.radmmm_voc_lrelu(ptr(x), c["ldx"], ptr(y), c["ldy"], rows, c["cols"], c["T"], ptr(lens), c["div"],
                               c["slope"], s), "voc_lrelu")


@MODES
@pytest.mark.parametrize("c", K.LRELU_CASES, ids=_ids(K.LRELU_CASES))
def test_lrelu(c, use_lens):
    inp = K.lrelu_inputs(c, use_lens)
    y = torch.full((inp["x"].shape[0], c["ldy"]), NAN, device=DEV)
    _run_lrelu(c, inp, _dev(inp["x"]), y)
    K.lrelu_check(c, inp, y.cpu().numpy())


@pytest.mark.parametrize("cols", [5, 32, 130])
def test_lrelu_in_place_equals_out_of_place_bit_for_bit(cols):
    """the generator's own call (vocoder.py: ptr(t) as x and y): ldx == ldy, y == x"""
    ld = K.roundup4(cols) + 4
    c = dict(cols=cols, ldy=ld, ldx=ld, T=7, lens=[7, 0, 3, 1], div=3.0, slope=0.1, seed=77 + cols)
    inp = K.lrelu_inputs(c, True)
    x = _dev(inp["x"])
    y = torch.full_like(x, NAN)
    _run_lrelu(c, inp, x, y)
    _run_lrelu(c, inp, x, x)
    out, inplace = y.cpu().numpy(), x.cpu().numpy()
    K.lrelu_check(c, inp, out)
    assert K.bit_equal(out, inplace).all()


# ---- radmmm_voc_conv_post ---------------------------------------------------------------------------------------------

@MODES
@pytest.mark.parametrize("c", K.CONV_POST_CASES, ids=_ids(K.CONV_POST_CASES))
def test_conv_post(c, use_lens):
    check, lib, ptr, s = _lib()
    inp = K.conv_post_inputs(c, use_lens)
    rows = inp["x"].shape[0]
    out = torch.full((rows,), NAN, device=DEV)
    bias = None if inp["bias"] is None else torch.full((1,), float(inp["bias"]), device=DEV)
    x, w, lens = _dev(inp["x"]), _dev(inp["w"]), _lens(inp["lens"])
    check(lib.radmmm_voc_conv_post(ptr(x), c["ldx"], ptr(w), c["ldw"], ptr(bias), ptr(out), rows, c["C"], c["taps"], c["T"],
                                   ptr(lens), c["div"], c["slope"], s), "voc_conv_post")
    K.conv_post_check(c, inp, out.cpu().numpy())


# ---- radmmm_voc_reflect_pad -------------------------------------------------------------------------------------------

@MODES
@pytest.mark.parametrize("c", K.REFLECT_CASES, ids=_ids(K.REFLECT_CASES))
def test_reflect_pad(c, use_lens):
    check, lib, ptr, s = _lib()
    inp = K.reflect_inputs(c, use_lens)
    B = len(c["lens"])
    xpad = torch.full((B, c["pitch"]), NAN, device=DEV)
    audio, lens = _dev(inp["audio"]), _lens(inp["lens"])
    check(lib.radmmm_voc_reflect_pad(ptr(audio), c["lda"], ptr(lens), ptr(xpad), B, c["S"], c["pad"], c["pitch"], s),
          "voc_reflect_pad")
    K.reflect_check(c, inp, xpad.cpu().numpy())


# ---- radmmm_voc_spec_bins ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", K.SPEC_CASES, ids=_ids(K.SPEC_CASES))
def test_spec_bins(c):
    check, lib, ptr, s = _lib()
    inp = K.spec_inputs(c)
    spec, bias = _dev(inp["spec"]), _dev(inp["bias"])
    check(lib.radmmm_voc_spec_bins(ptr(spec), c["lds"], c["rows"], c["cutoff"], ptr(bias), c["strength"], None, s),
          "voc_spec_bins")
    K.spec_check(c, inp, spec.cpu().numpy())


@pytest.mark.parametrize("c", K.SPEC_CASES[:18:3] + K.SPEC_CASES[-1:], ids=_ids(K.SPEC_CASES[:18:3] + K.SPEC_CASES[-1:]))
def test_spec_bins_mag_out_leaves_spec_alone(c):
    check, lib, ptr, s = _lib()
    inp = K.spec_inputs(c)
    spec = _dev(inp["spec"])
    mag = torch.full((c["rows"] * c["cutoff"],), NAN, device=DEV)
    check(lib.radmmm_voc_spec_bins(ptr(spec), c["lds"], c["rows"], c["cutoff"], None, 0.0, ptr(mag), s), "voc_spec_bins")
    K.spec_mag_check(c, inp, mag.cpu().numpy(), spec.cpu().numpy())


# ---- radmmm_voc_istft_finish ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", K.ISTFT_CASES, ids=_ids(K.ISTFT_CASES))
def test_istft_finish(c):
    check, lib, ptr, s = _lib()
    inp = K.istft_inputs(c)
    y, frames, winsq = _dev(inp["y"]), _lens(c["frames"]), _dev(inp["winsq"])
    check(lib.radmmm_voc_istft_finish(ptr(y), len(c["frames"]), c["pitch"], ptr(frames), ptr(winsq), c["n_fft"], c["hop"], s),
          "voc_istft_finish")
    K.istft_check(c, inp, y.cpu().numpy())


# ---- radmmm_voc_normalize ---------------------------------------------------------------------------------------------

@MODES
@pytest.mark.parametrize("c", K.NORM_CASES, ids=_ids(K.NORM_CASES))
def test_normalize(c, use_lens):
    """lens 1 .. 1025 and S around the 64-lane wave and the 1024-thread workgroup; the maximum first, last valid and
    negative; a larger sample at lens[b]; the tail past lens[b] and the row padding bit-unchanged.  The all-zero item
    comes back as NaN: 0 / 0, exactly what the reference's audio / max|audio| gives for silence (pinned here)."""
    check, lib, ptr, s = _lib()
    inp = K.normalize_inputs(c, use_lens)
    a, lens = _dev(inp["audio"]), _lens(inp["lens"])
    check(lib.radmmm_voc_normalize(ptr(a), c["lda"], ptr(lens), len(c["lens"]), c["S"], s), "voc_normalize")
    got = a.cpu().numpy()
    K.normalize_check(c, inp, got)
    n0 = c["lens"][K.NORM_ZERO_ITEM] if use_lens else c["S"]
    assert np.isnan(got[K.NORM_ZERO_ITEM, :n0]).all()


# ---- framed reads of radmmm_rowgemm_f32 -------------------------------------------------------------------------------

@MODES
@pytest.mark.parametrize("c", K.FRAMED_CASES, ids=_ids(K.FRAMED_CASES))
def test_framed_rowgemm_forward(c, use_lens):
    """the STFT's operand: C[b*F + f, n] = sum_k A[b * a_item_stride + f * hop + k] * W[n, k], overlapping rows
    (lda = hop < K); ragged frame counts with a_mask_mode = 1 and postmask = 1, and unmasked (lens = NULL,
    a_mask_mode = 0), the whole-frame path of a full batch"""
    from rad_mmm_amd._lib import rowgemm
    inp = K.framed_inputs(c, use_lens)
    B, F, N, Kk = len(c["lens"]), c["F"], c["N"], c["K"]
    ldc = K.roundup4(N)
    out = torch.full((B * F, ldc), NAN, device=DEV)
    A, W, lens = _dev(inp["A"]), _dev(inp["W"]), _lens(inp["lens"])
    rowgemm(A=A, lda=c["hop"], a_item_stride=inp["pitch"], B=W, ldb=Kk, b_tap_stride=0, C=out, ldc=ldc, M=B * F, N=N,
            K=Kk, taps=1, T=F, lens=lens, a_mask_mode=1 if use_lens else 0, postmask=1 if use_lens else 0)
    K.framed_check(c, inp, out[:, :N].cpu().numpy())


@pytest.mark.parametrize("Kk,F,G", K.INVERSE_CASES)
def test_framed_rowgemm_inverse_form_is_batch_invariant(Kk, F, G):
    """the inverse STFT's operand (K.INVERSE_CASES): against float64, and each item bit-equal to that item alone"""
    from rad_mmm_amd._lib import rowgemm
    inp = K.inverse_inputs(Kk, F, G)
    B, N, lda, frames = inp["B"], inp["N"], inp["lda"], inp["frames"]
    Ad, Wd, lens = _dev(inp["A"]), _dev(inp["W"]), _lens(frames)
    out = torch.full((B * G, N), NAN, device=DEV)
    kw = dict(lda=lda, a_item_stride=F * lda, B=Wd, ldb=lda, b_tap_stride=N * lda, ldc=N, N=N, K=Kk, taps=3, dil=1, T=G,
              a_mask_mode=1)
    rowgemm(A=Ad, C=out, M=B * G, lens=lens, **kw)
    got = out.cpu().numpy()
    K.inverse_check(inp, got)
    for b in range(B):
        alone = torch.full((G, N), NAN, device=DEV)
        rowgemm(A=Ad[b * F:], C=alone, M=G, lens=lens[b:b + 1], **kw)
        assert K.bit_equal(alone.cpu().numpy(), got[b * G:(b + 1) * G]).all(), b


# ---- argument errors that return before any launch --------------------------------------------------------------------

def test_argument_errors_return_before_any_launch():
    from rad_mmm_amd._lib import RadmmmError
    check, lib, ptr, s = _lib()
    x = torch.zeros(64, 8, device=DEV)
    y = torch.full((64, 8), NAN, device=DEV)
    w = torch.zeros(4200, device=DEV)
    fr = torch.ones(2, dtype=torch.int32, device=DEV)
    wsq = torch.ones(16, dtype=torch.float64, device=DEV)
    calls = {
        "ldx % 4 != 0": lambda: lib.radmmm_voc_lrelu(ptr(x), 6, ptr(y), 8, 8, 5, 4, None, 1.0, 0.1, s),
        "misaligned pointer": lambda: lib.radmmm_voc_lrelu(ptr(x) + 4, 8, ptr(y), 8, 8, 5, 4, None, 1.0, 0.1, s),
        "even taps": lambda: lib.radmmm_voc_conv_post(ptr(x), 8, ptr(w), 8, None, ptr(y), 8, 8, 4, 4, None, 1.0, 0.1, s),
        "taps * ldw > 4096": lambda: lib.radmmm_voc_conv_post(ptr(x), 8, ptr(w), 1368, None, ptr(y), 8, 8, 3, 4, None, 1.0,
                                                              0.1, s),
        "n_fft % hop != 0": lambda: lib.radmmm_voc_istft_finish(ptr(y), 2, 16, ptr(fr), ptr(wsq), 16, 6, s),
        "lds < 2 * cutoff": lambda: lib.radmmm_voc_spec_bins(ptr(y), 7, 8, 4, ptr(x), 0.5, None, s),
    }
    for what, call in calls.items():
        rc = call()
        assert rc != 0, what
        with pytest.raises(RadmmmError):
            check(rc, what)
    torch.cuda.synchronize()
    assert torch.isnan(y).all()                             # nothing was launched: no output was touched
