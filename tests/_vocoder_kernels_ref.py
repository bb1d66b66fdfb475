"""Plain numpy restatements of the six kernels of csrc/vocoder.hip and of the framed reads of radmmm_rowgemm_f32, in
the kernels' row layout ([B*T rows][ld], row r = b*T + t, per-item lengths), written from the reference's definitions
(vocoders/hifigan_models.py: conv_post + tanh and leaky_relu(x / n); vocoders/hifigan_denoiser.py; audio_processing.py:
window_sumsquare and STFT.inverse), not from the kernels.

Each restatement takes a `dtype`: float64 is the oracle, float32 is the same sequence of IEEE operations in the
kernels' precision (the bit-exact expectation of the one- or two-operation kernels).  `bug=` selects a named,
deliberately wrong variant; tests/test_vocoder_cpu.py shows that every case and bar of tests/test_hip_vocoder_direct.py
rejects them.  No variant is ever built into a kernel.

The cases, their inputs and the comparison functions live here too, so that the CPU discrimination checks and the GPU
tests use the very same inputs, comparison and bar.  Bars (u = 2^-24, the unit roundoff of float32):
  lrelu, reflect_pad, normalize, istft_finish: one or two IEEE operations per element (a division, a multiply, a copy;
      the envelope is the reference's own float32 running sum): bit-equal to the float32 restatement.
  conv_post: |hip - f64| <= n u sum|x_i w_i| + 4u per row, n = taps C + 1 (sequential fma accumulation, then a
      1-Lipschitz tanh of a few-ulp tanhf); the sum runs over the products, computed in float64.
  spec_bins: |hip - f64| <= 8u max(mag64, |bias strength|) per component; mag_out: 2u mag64.
  framed GEMM: rel_err < 2e-6, the bar tests/test_hip_parity.py::test_rowgemm_plain holds the same kernel to."""
import numpy as np

U = 2.0 ** -24
WRAP = 8192 * 256          # work items one sweep of the capped grid covers (grid_for of csrc/vocoder.hip, 256 threads)


def roundup4(n):
    return (n + 3) // 4 * 4


def bit_equal(a, b):
    """elementwise: the same float32 bits, or both NaN (a NaN's payload differs between hosts and the device)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _rows_valid(rows, T, lens):
    t = np.arange(rows) % T
    if lens is None:
        return np.ones(rows, bool)
    return t < np.repeat(np.asarray(lens), T)


def _f32(v):
    """a float argument as the C ABI receives it"""
    return float(np.float32(v))


def _leaky(v, slope):
    return np.where(v > 0, v, v * slope)


# ---- restatements ---------------------------------------------------------------------------------------------------

def lrelu_ref(x, cols, ldy, T, lens, div, slope, dtype=np.float64, bug=None):
    """x [rows, ldx] -> y [rows, ldy]: leaky_relu(x / div) in columns < cols of rows t < lens[b], 0 everywhere else"""
    rows = x.shape[0]
    if bug == "slope_other":
        slope = _f32(0.01) if slope == _f32(0.1) else _f32(0.1)
    v = x[:, :cols].astype(dtype)
    valid = _rows_valid(rows, T, lens)
    if bug == "mask_one_late" and lens is not None:
        valid = _rows_valid(rows, T, np.minimum(np.asarray(lens) + 1, T))
    y = np.full((rows, ldy), 7.0 if bug == "padding_not_zeroed" else 0.0, dtype)
    with np.errstate(invalid="ignore"):
        a = _leaky(v / dtype(div), dtype(slope))
    y[:, :cols] = np.where(valid[:, None], a, dtype(0))
    return y


def conv_post_ref(x, w, bias, C, taps, T, lens, div, slope, bug=None):
    """x [rows, ldx], w [taps, ldw], bias scalar or None -> (tanh(bias + conv) [rows] float64, sum |x_i w_i| [rows]).
    conv_post of hifigan_models.py (Conv1d(C, 1, taps, padding=taps//2) on leaky_relu(x / div), zero padded at each
    item's own length), rows at or past the length 0."""
    rows = x.shape[0]
    valid = _rows_valid(rows, T, lens)
    t = np.arange(rows) % T
    with np.errstate(invalid="ignore"):
        a = _leaky(x[:, :C].astype(np.float64) / np.float64(div), np.float64(slope))
    if bug != "tap_from_neighbour":
        a = np.where(valid[:, None], a, 0.0)
    acc, absum = np.zeros(rows), np.zeros(rows)
    for tap in range(taps):
        if bug == "tap_dropped" and tap == 0:
            continue
        s = tap - taps // 2
        src = np.arange(rows) + s
        inside = (t + s >= 0) & (t + s < T)
        if bug == "tap_from_neighbour":                      # the item border is ignored: row r + s of the whole buffer
            inside = (src >= 0) & (src < rows)
        rows_a = np.where(inside[:, None], a[np.clip(src, 0, rows - 1)], 0.0)
        ww = w[tap, :C].astype(np.float64)
        acc += rows_a @ ww
        absum += np.abs(rows_a) @ np.abs(ww)
    b0 = 0.0 if bias is None else float(bias)
    return np.where(valid, np.tanh(acc + b0), 0.0), np.where(valid, absum, 0.0)


def reflect_pad_ref(audio, lens, S, pad, pitch, bug=None):
    """audio [B, lda] -> xpad [B, pitch]: F.pad(audio[b, :lens[b]], (pad, pad), mode='reflect') (no edge repeat), zeros
    beyond lens[b] + 2 pad.  Items with lens[b] <= pad have no reflect pad (the reference raises): their row is NaN up
    to lens[b] + 2 pad here and the callers treat them apart."""
    B = audio.shape[0]
    out = np.zeros((B, pitch), audio.dtype)
    if bug == "tail_not_zeroed":
        out[:] = 1.0
    for b in range(B):
        n = S if lens is None else min(int(lens[b]), S)
        if n <= 0:
            continue
        if n <= pad:
            out[b, :n + 2 * pad] = np.nan
            continue
        j = np.arange(n + 2 * pad) - pad
        j = np.abs(j)
        edge = n if bug == "reflect_about_len" else n - 1
        j = np.where(j >= n, 2 * edge - j, j)
        out[b, :n + 2 * pad] = audio[b, np.clip(j, 0, audio.shape[1] - 1)]
    return out


def spec_mag_ref(spec, cutoff):
    s = spec.astype(np.float64)
    return np.sqrt(s[:, :cutoff] ** 2 + s[:, cutoff:2 * cutoff] ** 2)


def spec_bins_ref(spec, cutoff, bias, strength, bug=None):
    """spec [rows, lds] (re | im | untouched padding) -> float64 copy with every bin rescaled to the magnitude
    max(|bin| - bias[c] * strength, 0) at its own phase (hifigan_denoiser.py:54-58 with STFT.inverse's recombination);
    a zero bin has phase atan2(0, 0) = 0 and becomes (mag', 0)."""
    out = spec.astype(np.float64)
    re, im = out[:, :cutoff].copy(), out[:, cutoff:2 * cutoff].copy()
    mag = np.sqrt(re ** 2 + im ** 2)
    m2 = mag - bias.astype(np.float64)[None, :] * np.float64(strength)
    if bug != "clamp_missing":
        m2 = np.maximum(m2, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = m2 / mag
        zero_re = 0.0 if bug == "zero_bin_dropped" else m2
        out[:, :cutoff] = np.where(mag > 0, re * s, zero_re)
        out[:, cutoff:2 * cutoff] = np.where(mag > 0, (-im if bug == "imag_conjugated" else im) * s, 0.0)
    return out


def window_sumsquare_ref(winsq, n_frames, hop, n_fft, dtype=np.float32):
    """audio_processing.py:27-76 for an already squared window: the running sum is kept in `dtype` (float32 in the
    reference's call), the terms are float64."""
    n = n_fft + hop * (n_frames - 1)
    x = np.zeros(n, dtype=dtype)
    for i in range(n_frames):
        s = i * hop
        x[s:min(n, s + n_fft)] += winsq[:max(0, min(n_fft, n - s))]
    return x


def istft_finish_ref(y, frames, winsq, n_fft, hop, dtype=np.float64, env_dtype=np.float32, bug=None):
    """y [B, pitch]: the overlap-add of STFT.inverse with its first n_fft/2 samples already trimmed.  Per item
    (audio_processing.py:267-284): divide by window_sumsquare(frames[b]) where that exceeds tiny(float32), scale by
    n_fft / hop, keep (frames[b] - 1) * hop samples; zeros beyond."""
    B, pitch = y.shape
    out = np.zeros((B, pitch), dtype)
    if bug == "tail_not_zeroed":
        out[:] = y.astype(dtype) * dtype(n_fft / hop)
    tiny = np.finfo(np.float32).tiny
    for b in range(B):
        nf = int(frames[b])
        keep = min((nf - 1) * hop, pitch)
        if keep <= 0:
            continue
        ws = window_sumsquare_ref(winsq, nf + (n_fft // hop if bug == "f1_uncapped" else 0), hop, n_fft, env_dtype)
        m0 = n_fft // 2
        if bug == "envelope_shifted_one_frame":
            m0, ws = m0 + hop, np.concatenate([ws, np.zeros(hop, ws.dtype)])
        ws = ws[m0:m0 + keep].astype(dtype)
        v = y[b, :keep].astype(dtype)
        nz = ws > tiny
        v[nz] = v[nz] / ws[nz]
        out[b, :keep] = v * dtype(float(n_fft) / hop)
    return out


def normalize_ref(audio, lens, S, dtype=np.float64, bug=None):
    """audio [B, lda]: audio[b, :lens[b]] / max|audio[b, :lens[b]]| (vocoder_utils.py: audio / max|audio| of one
    utterance); everything at or past lens[b] as it was.  An all-zero item is 0 / 0 = NaN, as in the reference."""
    out = audio.astype(dtype)
    for b in range(audio.shape[0]):
        n = S if lens is None else min(int(lens[b]), S)
        if n <= 0:
            continue
        a = audio[b].astype(dtype)
        over = a[:S] if bug == "max_over_S" else a[:n]
        mx = over.max() if bug == "max_signed" else np.abs(over).max()
        hi = S if bug == "tail_scaled" else n
        with np.errstate(invalid="ignore", divide="ignore"):
            out[b, :hi] = a[:hi] / dtype(mx)
    return out


def framed_gemm_ref(A, a_item_stride, lda, W, F, B, lens=None, bug=None):
    """C[b*F + f, n] = sum_k A[b * a_item_stride + f * lda + k] * W[n, k] (float64), rows f >= lens[b] zero"""
    N, K = W.shape
    out = np.zeros((B * F, N))
    Wd = W.astype(np.float64)
    if bug:                                                 # the wrong strides reach a little past the buffer
        A = np.concatenate([A, np.zeros(K + 2 * F + 4 * B, A.dtype)])
    for b in range(B):
        n = F if lens is None or bug == "lens_ignored" else int(lens[b])
        base = b * (a_item_stride + (4 if bug == "item_stride_off" else 0))
        for f in range(n):
            s = base + f * (lda + (1 if bug == "frame_stride_off" else 0))
            out[b * F + f] = Wd @ A[s:s + K].astype(np.float64)
    return out


def tap_gemm_ref(A, a_item_stride, lda, W, G, B, lens, bug=None):
    """the inverse form: C[b*G + g, n] = sum_tap sum_k A[b * a_item_stride + (g + tap - taps/2) * lda + k] * W[tap, n, k]
    over frames 0 <= g + tap - taps/2 < lens[b] (float64)"""
    taps, N, K = W.shape
    out = np.zeros((B * G, N))
    Wd = W.astype(np.float64)
    for b in range(B):
        for g in range(G):
            for tap in range(taps):
                f = g + tap - taps // 2 + (1 if bug == "tap_shifted" else 0)
                if 0 <= f < (min(int(lens[b]), G) if bug == "mask_at_T" else int(lens[b])):
                    s = b * a_item_stride + f * lda
                    out[b * G + g] += Wd[tap] @ A[s:s + K].astype(np.float64)
    return out


# ---- cases: the shapes of tests/test_hip_vocoder_direct.py, their inputs, comparison and bar ----------------------
# Every case is ragged (an item of full length, an item of length 0 or the minimum) and runs a second time with
# lens = NULL where the ABI allows that (`use_lens`).  With lengths, input rows / samples at or past an item's length
# hold NaN wherever the kernel promises not to use them.

def _rng(case):
    return np.random.default_rng(case["seed"])


def _seeded(cases):
    for i, c in enumerate(cases):
        c["seed"] = 1000 + i
    return cases


def case_id(c):
    return "-".join(f"{k}{v}" for k, v in c.items() if k not in ("seed", "lens", "frames") and v is not None)


# lrelu: cols 1, 5, 32, 130; ldy == and > roundup4(cols); ldx != ldy; div 1 / 3, slope 0.1 / 0.01; one shape whose
# rows * ldy / 4 just exceeds one sweep of the capped grid.
LRELU_CASES = _seeded(
    [dict(cols=c, ldy=roundup4(c) + e, ldx=roundup4(c) + e + 4, T=7, lens=[7, 0, 3, 1], div=d, slope=s)
     for (c, d, s) in ((1, 1.0, 0.1), (5, 3.0, 0.01), (32, 3.0, 0.1), (130, 1.0, 0.01)) for e in (0, 8)]
    + [dict(cols=5, ldy=8, ldx=12, T=262145, lens=[262145, 0, 1, 131000], div=3.0, slope=0.1)])
assert LRELU_CASES[-1]["T"] * 4 * 2 > WRAP and (LRELU_CASES[-1]["T"] * 4 - 4) * 2 <= WRAP
LRELU_BUGS = ("padding_not_zeroed", "slope_other", "mask_one_late")


def lrelu_inputs(c, use_lens):
    g = _rng(c)
    rows = c["T"] * len(c["lens"])
    x = (2.0 * g.standard_normal((rows, c["ldx"]))).astype(np.float32)
    x[:, c["cols"]:] = np.nan
    lens = c["lens"] if use_lens else None
    x[~_rows_valid(rows, c["T"], lens)] = np.nan
    return dict(x=x, lens=lens)


def lrelu_expect(c, inp, dtype=np.float32, bug=None):
    return lrelu_ref(inp["x"], c["cols"], c["ldy"], c["T"], inp["lens"], _f32(c["div"]), _f32(c["slope"]), dtype, bug)


def check_bits(name, got, want32, want64):
    """the bar of the one- and two-operation kernels: every element bit-equal to the float32 restatement"""
    bad = int((~bit_equal(got, want32)).sum())
    with np.errstate(invalid="ignore"):
        d = np.abs(got.astype(np.float64) - want64)
    fin = np.isfinite(want64)
    err = float(d[fin].max()) if fin.any() else 0.0
    print(f"{name}: {bad} of {got.size} elements differ from the float32 restatement (bar: 0); "
          f"max |hip - f64| {err:.3e}")
    assert bad == 0, f"{name}: {bad} elements differ from the float32 restatement"
    return bad


def lrelu_check(c, inp, got, name="lrelu"):
    return check_bits(name, got, lrelu_expect(c, inp, np.float32), lrelu_expect(c, inp, np.float64))


# conv_post: (C, taps) (32, 7), (6, 3), (1, 1), (128, 31) and taps * ldw == 4096; ldw > C; bias NULL / not; T small
# enough that every tap offset is cut at a border; items of length 1 and taps/2; > 8192 * 256 rows at C = 4.
CONV_POST_CASES = _seeded([
    dict(C=32, taps=7, ldw=36, ldx=32, T=5, lens=[5, 1, 3, 0], bias=True, div=3.0, slope=0.01),
    dict(C=6, taps=3, ldw=8, ldx=8, T=4, lens=[4, 1, 0, 2], bias=False, div=1.0, slope=0.1),
    dict(C=1, taps=1, ldw=2, ldx=4, T=3, lens=[3, 1, 0], bias=True, div=3.0, slope=0.1),
    dict(C=128, taps=31, ldw=132, ldx=132, T=20, lens=[20, 1, 15, 0], bias=True, div=1.0, slope=0.01),
    dict(C=4094, taps=1, ldw=4096, ldx=4096, T=3, lens=[3, 0, 1], bias=False, div=3.0, slope=0.01),
    dict(C=4, taps=3, ldw=5, ldx=4, T=1048580, lens=[1048580, 1], bias=True, div=3.0, slope=0.1),
])
assert CONV_POST_CASES[-1]["T"] * 2 > WRAP and CONV_POST_CASES[4]["taps"] * CONV_POST_CASES[4]["ldw"] == 4096
CONV_POST_BUGS = ("tap_dropped", "tap_from_neighbour")


def conv_post_inputs(c, use_lens):
    g = _rng(c)
    rows = c["T"] * len(c["lens"])
    x = (2.0 * g.standard_normal((rows, c["ldx"]))).astype(np.float32)
    x[:, c["C"]:] = np.nan
    lens = c["lens"] if use_lens else None
    x[~_rows_valid(rows, c["T"], lens)] = np.nan
    w = (g.standard_normal((c["taps"], c["ldw"])) / np.sqrt(c["C"] * c["taps"])).astype(np.float32)
    w[:, c["C"]:] = np.nan
    bias = np.float32(0.3) if c["bias"] else None
    return dict(x=x, w=w, bias=bias, lens=lens)


def conv_post_expect(c, inp, bug=None):
    return conv_post_ref(inp["x"], inp["w"], inp["bias"], c["C"], c["taps"], c["T"], inp["lens"], _f32(c["div"]),
                         _f32(c["slope"]), bug)


def conv_post_check(c, inp, got, name="conv_post"):
    ref, absum = conv_post_expect(c, inp)
    bound = (c["taps"] * c["C"] + 1) * U * absum + 4 * U
    valid = _rows_valid(ref.shape[0], c["T"], inp["lens"])
    with np.errstate(invalid="ignore"):
        ratio = np.abs(got.astype(np.float64) - ref) / bound
    worst = float(np.nanmax(ratio)) if not np.isnan(ratio).all() else np.nan
    print(f"{name}: worst |hip - f64| / bar {worst:.3f}, max |hip - f64| "
          f"{float(np.nanmax(np.abs(got.astype(np.float64) - ref))):.3e}")
    assert not np.isnan(got).any(), f"{name}: NaN in the output"
    assert (ratio <= 1.0).all(), f"{name}: worst ratio {worst}"
    assert not got[~valid].any(), f"{name}: rows past the length are not 0"
    return worst


# reflect_pad: pad 0, 3, 512; lens pad + 1, S and between; lda > S, pitch > S + 2 pad; one item with 1 <= len <= pad
# (`clamp`: its index); one grid-wrapping shape.
REFLECT_CASES = _seeded([
    dict(pad=0, S=10, lda=12, pitch=13, lens=[10, 1, 4, 0], clamp=None),
    dict(pad=3, S=11, lda=11, pitch=17, lens=[11, 4, 7, 2], clamp=3),
    dict(pad=3, S=11, lda=16, pitch=21, lens=[4, 11, 0, 9], clamp=None),
    dict(pad=512, S=1500, lda=1504, pitch=2530, lens=[1500, 513, 900, 0, 200], clamp=4),
    dict(pad=512, S=698100, lda=698100, pitch=699124, lens=[698100, 513, 350000], clamp=None),
])
assert REFLECT_CASES[-1]["pitch"] * 3 > WRAP
REFLECT_BUGS = ("reflect_about_len", "tail_not_zeroed")


def reflect_inputs(c, use_lens):
    g = _rng(c)
    B = len(c["lens"])
    a = g.standard_normal((B, c["lda"])).astype(np.float32)
    a[:, c["S"]:] = np.nan
    lens = c["lens"] if use_lens else None
    if use_lens:
        for b, n in enumerate(lens):
            a[b, n:] = np.nan
    return dict(audio=a, lens=lens)


def reflect_expect(c, inp, bug=None):
    return reflect_pad_ref(inp["audio"], inp["lens"], c["S"], c["pad"], c["pitch"], bug)


def reflect_check(c, inp, got, name="reflect_pad"):
    want = reflect_expect(c, inp)
    spec = np.ones(got.shape[0], bool)
    if inp["lens"] is not None and c["clamp"] is not None:
        b, n = c["clamp"], c["lens"][c["clamp"]]
        spec[b] = False                 # no reflect pad is defined: every written value is one of the item's own samples
        head = got[b, :n + 2 * c["pad"]]
        own = np.isin(head.view(np.uint32), inp["audio"][b, :n].view(np.uint32))
        print(f"{name}: item of {n} <= pad {c['pad']}: {int((~own).sum())} values are not the item's own samples")
        assert own.all(), f"{name}: a short item's pad holds values from outside the item"
        assert not got[b, n + 2 * c["pad"]:].any()
    return check_bits(name, got[spec], want[spec], want[spec].astype(np.float64))


# spec_bins: cutoff 1, 7, 513; lds == and > 2 cutoff; magnitudes above, equal to and below bias * strength; exact
# (0, 0) bins with bias * strength > 0 and < 0; strength 0; one grid-wrapping shape.
SPEC_CASES = _seeded(
    [dict(cutoff=k, lds=2 * k + e, rows=6, strength=s) for k in (1, 7, 513) for e in (0, 3) for s in (0.5, -0.5, 0.0)]
    + [dict(cutoff=513, lds=1028, rows=4090, strength=0.5)])
assert SPEC_CASES[-1]["rows"] * 513 > WRAP
SPEC_BUGS = ("clamp_missing", "zero_bin_dropped", "imag_conjugated")


def spec_inputs(c, use_lens=True):
    g = _rng(c)
    k, rows = c["cutoff"], c["rows"]
    bias = (0.5 + g.random(k)).astype(np.float32)
    spec = np.full((rows, c["lds"]), 7.0, np.float32)
    z = (4.0 * g.standard_normal((rows, 2 * k))).astype(np.float32)
    for r in range(rows):
        kind = r % 6
        if kind == 1:                              # |bin| == bias * 0.5 exactly (a power-of-two multiple is exact)
            z[r, :k], z[r, k:] = bias * np.float32(0.5), 0.0
        elif kind == 2:                            # below the threshold
            z[r] *= np.float32(0.01)
        elif kind == 3:                            # exact (0, 0) bins
            z[r] = 0.0
        elif kind == 4:                            # purely imaginary, negative
            z[r, :k], z[r, k:] = 0.0, -np.abs(z[r, k:])
    spec[:, :2 * k] = z
    return dict(spec=spec, bias=bias)


def spec_expect(c, inp, bug=None):
    return spec_bins_ref(inp["spec"], c["cutoff"], inp["bias"], _f32(c["strength"]), bug)


def spec_check(c, inp, got, name="spec_bins"):
    k = c["cutoff"]
    want = spec_expect(c, inp)
    mag = spec_mag_ref(inp["spec"], k)
    thr = np.abs(inp["bias"].astype(np.float64) * np.float64(np.float32(c["strength"])))[None, :]
    bound = 8 * U * np.maximum(mag, thr)
    bound = np.concatenate([bound, bound], 1)
    d = np.abs(got[:, :2 * k].astype(np.float64) - want[:, :2 * k])
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0, d / bound, np.where(d == 0, 0.0, np.inf))
    worst = float(ratio.max())
    print(f"{name}: worst |hip - f64| / bar {worst:.3f}, max |hip - f64| {float(d.max()):.3e}")
    assert not np.isnan(got).any() and worst <= 1.0, f"{name}: worst ratio {worst}"
    assert bit_equal(got[:, 2 * k:], inp["spec"][:, 2 * k:]).all(), f"{name}: the row padding was written"
    return worst


def spec_mag_check(c, inp, got_mag, got_spec, name="spec_bins mag_out"):
    mag = spec_mag_ref(inp["spec"], c["cutoff"])
    d = np.abs(got_mag.reshape(mag.shape).astype(np.float64) - mag)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(mag > 0, d / (2 * U * mag), np.where(d == 0, 0.0, np.inf))
    worst = float(ratio.max())
    print(f"{name}: worst |hip - f64| / bar {worst:.3f}, max |hip - f64| {float(d.max()):.3e}")
    assert not np.isnan(got_mag).any() and worst <= 1.0, f"{name}: worst ratio {worst}"
    assert bit_equal(got_spec, inp["spec"]).all(), f"{name}: spec was written in mag_out mode"
    return worst


# istft_finish: (n_fft, hop) (16, 4), (16, 8), (16, 16), (1024, 256); frames 0 .. 5 and a long item in one batch;
# pitch > (nf - 1) * hop; a Hann window and one with runs of zeros (the FLT_MIN branch); one grid-wrapping shape.
ISTFT_CASES = _seeded(
    [dict(n_fft=n, hop=h, frames=[0, 1, 2, 3, 4, 5, long], pitch=(long - 1) * h + 5, win=w)
     for (n, h, long) in ((16, 4, 12), (16, 8, 12), (16, 16, 12), (1024, 256, 9)) for w in ("hann", "zeros")]
    + [dict(n_fft=1024, hop=256, frames=[2736, 0, 1000], pitch=700160, win="hann")])
assert ISTFT_CASES[-1]["pitch"] * 3 > WRAP
ISTFT_BUGS = ("envelope_shifted_one_frame", "f1_uncapped", "tail_not_zeroed")


def hann_sq(n):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)) ** 2


def istft_inputs(c, use_lens=True):
    g = _rng(c)
    n, h = c["n_fft"], c["hop"]
    winsq = hann_sq(n)
    if c["win"] == "zeros":
        winsq[:n // 4] = 0.0                       # a run of zeros: with n_fft == hop the envelope there is exactly 0
        winsq[1::h] = 0.0                          # every frame's term at these samples is 0: envelope 0 for any n_fft/hop
        if h >= 4:
            winsq[2::h] = 1e-41                    # sums below FLT_MIN (and not 0)
    y = g.standard_normal((len(c["frames"]), c["pitch"])).astype(np.float32)
    return dict(y=y, winsq=winsq, frames=c["frames"])


def istft_expect(c, inp, dtype=np.float32, bug=None):
    return istft_finish_ref(inp["y"], inp["frames"], inp["winsq"], c["n_fft"], c["hop"], dtype, np.float32, bug)


def istft_check(c, inp, got, name="istft_finish"):
    return check_bits(name, got, istft_expect(c, inp, np.float32), istft_expect(c, inp, np.float64))


# normalize: lens 1, 63, 64, 65, 1023, 1024, 1025, S; the maximum first, last valid and negative; a larger value at
# lens[b]; the tail untouched; an all-zero item (NaN, as the reference's 0 / 0).
NORM_CASES = _seeded([dict(S=2050, lda=2052, lens=[1, 63, 64, 65, 1023, 1024, 1025, 2050, 100, 0])])
NORM_ZERO_ITEM = 8
NORM_BUGS = ("max_over_S", "tail_scaled", "max_signed")


def normalize_inputs(c, use_lens):
    g = _rng(c)
    B = len(c["lens"])
    a = g.standard_normal((B, c["lda"])).astype(np.float32)
    a[:, c["S"]:] = 1e7                            # the row padding: larger than anything inside
    lens = c["lens"] if use_lens else None
    for b in range(B):
        n = c["lens"][b] if use_lens else c["S"]
        if n > 0:
            where = (0, n - 1, n // 2)[b % 3]      # the maximum first, last valid, in the middle; negative for odd b
            a[b, where] = 9.5 if b % 2 == 0 else -9.5
        if use_lens and n < c["S"]:
            a[b, n] = 1e6                          # a larger sample just past the length
            a[b, n + 1:c["S"]] *= 50.0
    a[NORM_ZERO_ITEM, :c["lens"][NORM_ZERO_ITEM] if use_lens else c["S"]] = 0.0
    return dict(audio=a, lens=lens)


def normalize_expect(c, inp, dtype=np.float32, bug=None):
    return normalize_ref(inp["audio"], inp["lens"], c["S"], dtype, bug)


def normalize_check(c, inp, got, name="normalize"):
    want = normalize_expect(c, inp, np.float32)
    n0 = c["lens"][NORM_ZERO_ITEM] if inp["lens"] is not None else c["S"]
    assert np.isnan(want[NORM_ZERO_ITEM, :n0]).all()          # the pinned 0 / 0 of the all-zero item
    return check_bits(name, got, want, normalize_expect(c, inp, np.float64))


# framed GEMM: (hop, K, N, F, B): K = 72 takes the generic kernel (K % 16 != 0), the other two the 16-row kernel.
FRAMED_CASES = _seeded([
    dict(hop=8, K=72, N=38, F=50, lens=[50, 0, 7]),
    dict(hop=8, K=64, N=130, F=50, lens=[50, 1, 23]),
    dict(hop=256, K=1024, N=1026, F=9, lens=[9, 4]),
])
FRAMED_BUGS = ("frame_stride_off", "lens_ignored", "item_stride_off")


def framed_inputs(c, use_lens=True):
    g = _rng(c)
    B = len(c["lens"])
    pitch = roundup4((c["F"] - 1) * c["hop"] + c["K"]) + 4
    A = g.standard_normal(B * pitch).astype(np.float32)
    lens = c["lens"] if use_lens else None         # NULL: a_mask_mode 0, every item has all F frames
    for b, n in enumerate(c["lens"] if use_lens else [c["F"]] * B):     # samples no frame below the length reaches
        A[b * pitch + (((n - 1) * c["hop"] + c["K"]) if n else 0):(b + 1) * pitch] = np.nan
    W = (g.standard_normal((c["N"], c["K"])) / np.sqrt(c["K"])).astype(np.float32)
    return dict(A=A, W=W, pitch=pitch, lens=lens)


def framed_expect(c, inp, bug=None):
    return framed_gemm_ref(inp["A"], inp["pitch"], c["hop"], inp["W"], c["F"], len(c["lens"]), inp["lens"], bug)


def rel_err(a, b):
    """conftest.rel_err"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def framed_check(c, inp, got, name="framed gemm"):
    want = framed_expect(c, inp)
    err = rel_err(got, want)
    print(f"{name}: rel_err {err:.3e} = {err / 2e-6:.3f} of the bar")
    assert err < 2e-6, f"{name}: rel_err {err}"          # NaN fails too
    if inp["lens"] is not None:
        rows = np.repeat(np.asarray(c["lens"]), c["F"]) <= np.tile(np.arange(c["F"]), len(c["lens"]))
        assert not got[rows].any(), f"{name}: rows past the length are not 0"
    return err / 2e-6


# the inverse form: items F rows apart (a_item_stride = F * lda) read as T = G frames each with taps = 3 and
# a_mask_mode = 1.  G = F - 1 is the denoiser's own call (a full item has lens[b] = F = T + 1 frames); with G > F an
# item's frames past F lie in the next item's rows and only the length mask keeps them out.  K = 64 takes the 16-row
# kernel, K = 72 the generic one.
INVERSE_CASES = [(64, 6, 8), (72, 6, 8), (64, 6, 5), (72, 6, 5)]
INVERSE_BUGS = ("tap_shifted", "mask_at_T")


def inverse_inputs(Kk, F, G):
    g = np.random.default_rng(Kk + G)
    B, N, lda, frames = 3, 8, Kk, [F, 1, 4]
    A = g.standard_normal(((B - 1) * F + max(F, G) + 1, lda)).astype(np.float32)     # + the row a tap may reach
    for b, n in enumerate(frames):
        A[b * F + n:(b + 1) * F] = np.nan                   # the item's own rows at or past its frame count
    A[B * F:] = np.nan
    W = (g.standard_normal((3, N, lda)) / np.sqrt(3 * Kk)).astype(np.float32)
    return dict(A=A, W=W, B=B, N=N, lda=lda, frames=frames, F=F, G=G)


def inverse_expect(inp, bug=None):
    return tap_gemm_ref(inp["A"].reshape(-1), inp["F"] * inp["lda"], inp["lda"], inp["W"], inp["G"], inp["B"],
                        inp["frames"], bug)


def inverse_check(inp, got, name="inverse form"):
    err = rel_err(got, inverse_expect(inp))
    print(f"{name} K={inp['lda']} F={inp['F']} G={inp['G']}: rel_err {err:.3e} = {err / 2e-6:.3f} of the bar")
    assert err < 2e-6, f"{name}: rel_err {err}"          # NaN fails too
    return err / 2e-6
