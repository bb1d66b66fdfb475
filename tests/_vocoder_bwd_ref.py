"""Plain numpy restatements of the two kernels of csrc/vocoder_bwd.hip (radmmm_voc_lrelu_bwd, radmmm_voc_conv_post_bwd)
in the kernels' row layout ([B*T rows][ld], row r = b*T + t, per-item lengths), written from the derivatives of the
reference's operations (vocoders/hifigan_models.py: leaky_relu(x / n), conv_post + tanh), not from the kernels.

`bug=` selects a named, deliberately wrong variant: tests/test_vocoder_bwd_cpu.py shows that torch autograd in float64
rejects each of them, and accepts the models.  No variant is ever built into a kernel.

The cases, their inputs, the comparison functions and the bars live here, so that tests/test_hip_vocoder_bwd_direct.py
is a list of launches.  Bars (u = 2^-24, the unit roundoff of float32):
  lrelu_bwd: at most one multiply, one division and one addition per element in the order the header states: bit-equal
      to the float32 restatement, which performs the same IEEE operations.
  conv_post_bwd: n * 2^-23 * sum |terms| per output element (_gemm_ref.accumulation_bar: any order of an fp32
      accumulation of n products).  dpre = g (1 - audio^2) = g - g audio^2 enters every term with the magnitude
      |g| (1 + audio^2) (the subtraction may cancel) and costs three roundings, the slope and the division two more:
        dx[r, c]: n = taps + 5,        terms |w[tap, c]| |dpre|_mag [r - (tap - taps/2)] * |factor| / div
        dw[tap, c]: n = valid rows + 5, terms |dpre|_mag [r] |leaky_relu(x[r + tap - taps/2, c] / div)|
        dbias: n = valid rows + 3,     terms |dpre|_mag [r]"""
import numpy as np

from _vocoder_kernels_ref import U, _f32, _leaky, _rows_valid, bit_equal, case_id, check_bits

WRAP = 8192 * 256          # float4s one sweep of lrelu_bwd's capped grid covers


# ---- the generator's training step through the float64 restatement ------------------------------------------------

def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def restatement_leaves(sd, plain=False):
    """float64 leaf tensors by the generator's parameter names (new resblock keys); plain: the folded weights, the
    parameters after remove_weight_norm, instead of weight_g / weight_v"""
    import torch
    from _vocoder_ref import _new_keys, _w
    leaves = {k: v.detach().double().clone().requires_grad_(True) for k, v in _new_keys(sd).items()}
    if plain:
        names = sorted({k.rsplit(".", 1)[0] for k in leaves})
        folded = {n + ".weight": _w(leaves, n).detach().requires_grad_(True) for n in names}
        folded.update({n + ".bias": leaves[n + ".bias"] for n in names})
        leaves = folded
    return leaves


def restatement_loss(leaves, cfg, x, lens, target):
    """L = sum_b sum_t (y_b[t] - target_b[t])^2 / N through _vocoder_ref.generator_ref, one utterance at a time at its
    own length (as the reference runs them), float64; N = the number of valid samples"""
    from _vocoder_ref import generator_ref
    hop = int(np.prod(cfg["upsample_rates"]))
    N = int(sum(lens)) * hop
    loss = 0.0
    for b, n in enumerate(lens):
        y = generator_ref(leaves, cfg, x[b:b + 1, :, :n])[0, 0]
        loss = loss + ((y - target[b, :n * hop].double()) ** 2).sum() / N
    return loss


def restatement_step(cfg, sd, mel, lens, target, plain=False):
    """-> (loss, {name: gradient} with "mel"), float64"""
    leaves = restatement_leaves(sd, plain)
    x = mel.detach().double().clone().requires_grad_(True)
    loss = restatement_loss(leaves, cfg, x, lens, target)
    loss.backward()
    g = {k: v.grad for k, v in leaves.items()}
    g["mel"] = x.grad
    return loss.detach(), g


def restatement_adam(cfg, sd, mel, lens, target, steps, lr):
    """the losses of `steps` torch.optim.Adam steps on the weight-normed parameters, float64"""
    import torch
    leaves = restatement_leaves(sd)
    opt = torch.optim.Adam(list(leaves.values()), lr=lr)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = restatement_loss(leaves, cfg, mel.double(), lens, target)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


def _seeded(cases, base):
    for i, c in enumerate(cases):
        c["seed"] = base + i
    return cases


# ---- restatements ---------------------------------------------------------------------------------------------------

def lrelu_bwd_ref(gy, a, gx0, cols, T, lens, div, slope, accum, dtype=np.float64, bug=None):
    """gy [rows, ldgy], a [rows, lda] = leaky_relu(x / div, slope) as saved, gx0 [rows, ldgx] (what gx held) -> gx:
    in columns < cols of rows t < lens[b]  (accum ? gx0 : 0) + (a > 0 ? gy : gy * slope) / div, 0 in the other rows,
    gx0 in the columns at and past cols."""
    rows = gy.shape[0]
    valid = _rows_valid(rows, T, lens)
    if bug == "row_leaks" and lens is not None:
        valid = _rows_valid(rows, T, np.minimum(np.asarray(lens) + 1, T))
    g, s = gy[:, :cols].astype(dtype), a[:, :cols].astype(dtype)
    with np.errstate(invalid="ignore"):
        on = s >= 0 if bug == "slope_at_zero" else s > 0
        m = np.where(on, g, g * dtype(slope))
        q = m if bug == "div_missing" else m / dtype(div)
        v = gx0[:, :cols].astype(dtype) + q if accum else q
    out = gx0.astype(dtype).copy()
    out[:, :cols] = np.where(valid[:, None], v, dtype(0))
    return out


def conv_post_bwd_ref(x, w, audio, g, C, taps, T, lens, div, slope, bug=None):
    """x [rows, ldx], w [taps, ldw], audio [rows] = tanh(pre), g [rows] -> dict of float64 arrays: dx [rows, C],
    dw [taps, C], dbias (scalar) and the sums of |terms| of each (dx_abs, dw_abs, db_abs) for the bars; `rows_valid`."""
    rows = x.shape[0]
    h = taps // 2
    valid = _rows_valid(rows, T, lens)
    leak = valid
    if bug == "row_leaks" and lens is not None:
        leak = _rows_valid(rows, T, np.minimum(np.asarray(lens) + 1, T))
    t = np.arange(rows) % T
    with np.errstate(invalid="ignore"):
        a64, g64 = audio.astype(np.float64), g.astype(np.float64)
        dpre = np.where(leak, g64 * (1.0 - a64 * a64), 0.0)
        dmag = np.where(leak, np.abs(g64) * (1.0 + a64 * a64), 0.0)
        xd = np.where(valid[:, None], x[:, :C].astype(np.float64), 0.0)
        A = _leaky(xd / np.float64(div), np.float64(slope))
        on = xd >= 0 if bug == "slope_at_zero" else xd > 0
        fac = np.where(on, 1.0, np.float64(slope)) / (1.0 if bug == "div_missing" else np.float64(div))
    wd = w[:, :C].astype(np.float64)
    s, s_abs = np.zeros((rows, C)), np.zeros((rows, C))
    dw, dw_abs = np.zeros((taps, C)), np.zeros((taps, C))
    for tap in range(taps):
        sh = tap - h
        # pre[r] reads row r + sh: its gradient reaches row r' = r + sh from r = r' - sh
        back = sh if bug == "tap_not_flipped" else -sh
        src = np.arange(rows) + back
        inside = (t + back >= 0) & (t + back < T)
        d = np.where(inside, dpre[np.clip(src, 0, rows - 1)], 0.0)
        dm = np.where(inside, dmag[np.clip(src, 0, rows - 1)], 0.0)
        s += d[:, None] * wd[tap][None, :]
        s_abs += dm[:, None] * np.abs(wd[tap])[None, :]
        dw[tap] = (d[:, None] * A).sum(0)
        dw_abs[tap] = (dm[:, None] * np.abs(A)).sum(0)
    dx = np.where(valid[:, None], s * fac, 0.0)
    return dict(dx=dx, dx_abs=np.where(valid[:, None], s_abs * np.abs(fac), 0.0), dw=dw, dw_abs=dw_abs, dbias=dpre.sum(),
                db_abs=dmag.sum(), rows_valid=int(valid.sum()))


# ---- cases ------------------------------------------------------------------------------------------------------------
# Both kernels: C in {4, 32, 128, 512} (the widths of V1 and V3 and the narrowest), leading dimensions wider than C, div 1
# and 3, lengths [T, 1, 0 < n < T] and lens = NULL.  With lengths, rows at or past an item's length hold NaN in every
# input; padding columns hold NaN in the inputs and a sentinel in the outputs.

BUGS = ("slope_at_zero", "div_missing", "row_leaks")
POST_BUGS = BUGS + ("tap_not_flipped",)

# lrelu_bwd: accum on and off, slope 0.1 and 0.01, in place (gx is gy), one shape whose rows * cols / 4 just exceeds one
# sweep of the capped grid.
LRELU_BWD_CASES = _seeded(
    [dict(C=c, ldgy=c + e, lda=c + 2 * e, ldgx=c + e, T=7, lens=[7, 1, 3], div=d, slope=s, accum=acc, inplace=False)
     for (c, e) in ((4, 0), (32, 4), (128, 8), (512, 4))
     for (d, s, acc) in ((1.0, 0.1, False), (3.0, 0.1, True), (3.0, 0.01, False), (1.0, 0.01, True))]
    + [dict(C=32, ldgy=36, lda=32, ldgx=36, T=7, lens=[7, 1, 3], div=3.0, slope=0.1, accum=False, inplace=True),
       dict(C=4, ldgy=4, lda=4, ldgx=4, T=699051, lens=[699051, 1, 350000], div=3.0, slope=0.1, accum=True,
            inplace=False)], 2000)
assert LRELU_BWD_CASES[-1]["T"] * 3 > WRAP and (LRELU_BWD_CASES[-1]["T"] - 1) * 3 <= WRAP


def lrelu_bwd_inputs(c, use_lens):
    g = np.random.default_rng(c["seed"])
    rows, C = c["T"] * len(c["lens"]), c["C"]
    lens = c["lens"] if use_lens else None
    valid = _rows_valid(rows, c["T"], lens)
    gy = g.standard_normal((rows, c["ldgy"])).astype(np.float32)
    x = (2.0 * g.standard_normal((rows, c["lda"]))).astype(np.float32)
    x[g.random((rows, c["lda"])) < 0.1] = 0.0                   # exact zeros: the derivative there is the slope
    with np.errstate(invalid="ignore"):
        a = _leaky(x / np.float32(c["div"]), np.float32(c["slope"])).astype(np.float32)
    gx0 = g.standard_normal((rows, c["ldgx"])).astype(np.float32)
    gy[:, C:], a[:, C:], gx0[:, C:] = np.nan, np.nan, 7.0
    gy[~valid], a[~valid] = np.nan, np.nan
    gx0[~valid, :C] = np.nan
    return dict(gy=gy, a=a, gx0=gx0, lens=lens)


def lrelu_bwd_expect(c, inp, dtype=np.float32, bug=None):
    gx0 = inp["gx0"]
    if c["inplace"]:                                            # gx is gy: what gx held is gy (ldgx == ldgy)
        gx0 = inp["gy"].copy()
    return lrelu_bwd_ref(inp["gy"], inp["a"], gx0, c["C"], c["T"], inp["lens"], _f32(c["div"]), _f32(c["slope"]),
                         c["accum"], dtype, bug)


def lrelu_bwd_check(c, inp, got, name="lrelu_bwd"):
    return check_bits(name, got, lrelu_bwd_expect(c, inp, np.float32), lrelu_bwd_expect(c, inp, np.float64))


# conv_post_bwd: T no multiple of the rows of a workgroup's chunk (2048 / (C/4)) and more than one chunk; one shape with
# more chunks than the grid's 1024 workgroups; taps 7 (the generator's) and 3, 1; ldw > C.
POST_BWD_CASES = _seeded([
    dict(C=4, taps=7, ldw=4, ldx=8, lddx=4, T=1501, lens=[1501, 1, 700], div=3.0, slope=0.01),
    dict(C=32, taps=7, ldw=36, ldx=36, lddx=40, T=301, lens=[301, 1, 100], div=3.0, slope=0.01),
    dict(C=128, taps=7, ldw=128, ldx=132, lddx=128, T=77, lens=[77, 1, 5], div=1.0, slope=0.01),
    dict(C=512, taps=7, ldw=516, ldx=512, lddx=516, T=37, lens=[37, 1, 2], div=3.0, slope=0.1),
    dict(C=12, taps=3, ldw=12, ldx=12, lddx=12, T=5, lens=[5, 1, 3], div=1.0, slope=0.01),
    dict(C=8, taps=1, ldw=9, ldx=8, lddx=8, T=3, lens=[3, 1, 2], div=3.0, slope=0.01),
    dict(C=512, taps=7, ldw=512, ldx=512, lddx=512, T=5467, lens=[5467, 1, 2000], div=3.0, slope=0.01),
], 2100)
assert POST_BWD_CASES[-1]["T"] * 3 > 1024 * 16


def post_bwd_inputs(c, use_lens):
    g = np.random.default_rng(c["seed"])
    rows, C = c["T"] * len(c["lens"]), c["C"]
    lens = c["lens"] if use_lens else None
    valid = _rows_valid(rows, c["T"], lens)
    x = (2.0 * g.standard_normal((rows, c["ldx"]))).astype(np.float32)
    x[g.random((rows, c["ldx"])) < 0.05] = 0.0
    w = (g.standard_normal((c["taps"], c["ldw"])) / np.sqrt(C * c["taps"])).astype(np.float32)
    audio = np.tanh(1.5 * g.standard_normal(rows)).astype(np.float32)
    gr = g.standard_normal(rows).astype(np.float32)
    x[:, C:], w[:, C:] = np.nan, np.nan
    x[~valid], audio[~valid], gr[~valid] = np.nan, np.nan, np.nan
    return dict(x=x, w=w, audio=audio, g=gr, lens=lens)


def post_bwd_expect(c, inp, bug=None):
    return conv_post_bwd_ref(inp["x"], inp["w"], inp["audio"], inp["g"], c["C"], c["taps"], c["T"], inp["lens"],
                             _f32(c["div"]), _f32(c["slope"]), bug)


def _ratio(got, want, bar):
    d = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(bar > 0, d / bar, np.where(d == 0, 0.0, np.inf))
    return float(np.max(r))


def post_bwd_check(c, inp, dx, dw, dbias, name="conv_post_bwd"):
    """dx [rows, lddx] (pre-filled with the sentinel 7 in its padding columns), dw [taps, ldw], dbias [1]"""
    e = post_bwd_expect(c, inp)
    C, taps, n = c["C"], c["taps"], e["rows_valid"]
    unit = 2.0 * U
    r_dx = _ratio(dx[:, :C], e["dx"], (taps + 5) * unit * e["dx_abs"])
    r_dw = _ratio(dw[:, :C], e["dw"], (n + 5) * unit * e["dw_abs"])
    r_db = _ratio(dbias[0], e["dbias"], (n + 3) * unit * e["db_abs"])
    print(f"{name}: worst |hip - f64| / bar: dx {r_dx:.3f}, dw {r_dw:.3f}, dbias {r_db:.3f} ({n} valid rows)")
    assert not np.isnan(dx[:, :C]).any() and not np.isnan(dw[:, :C]).any() and not np.isnan(dbias).any(), f"{name}: NaN"
    assert r_dx <= 1.0 and r_dw <= 1.0 and r_db <= 1.0, f"{name}: ratios {r_dx} {r_dw} {r_db}"
    valid = _rows_valid(dx.shape[0], c["T"], inp["lens"])
    assert not dx[~valid, :C].any(), f"{name}: dx rows past the length are not 0"
    assert (dx[:, C:] == 7.0).all(), f"{name}: dx's row padding was written"
    assert not dw[:, C:].any(), f"{name}: dw's padding columns are not 0"
    return max(r_dx, r_dw, r_db)
