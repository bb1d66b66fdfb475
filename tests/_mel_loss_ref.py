"""numpy float64 restatement of the mel L1 loss as rad_mmm_amd/csrc/mel_loss.hip computes it, step by step (frame, DFT, mag,
mel projection, log-clamp terms, finish, bwd, dmag, dspec, dA, unframe), with the backward written out by hand.  It is the
model of the direct kernel tests and the oracle of the GPU tests; tests/test_mel_loss_cpu.py holds it to fixtures made by
the reference's own TacotronSTFT under torch autograd (tests/golden/make_golden_mel_loss.py).

The bases are the module's: float32 values (audio_processing.windowed_dft_basis, the fixture's mel_basis) taken to float64,
which is what the reference's float64 run does with its float32 buffers.

`bug=` plants one wrong variant (the CPU tests show that every comparison bar of the GPU tests rejects each of them that
moves the figure):
    reflectS     reflection about S - 1 instead of lens[b] - 1
    drop_mirror  the right mirror term dropped in the unframe
    normBF       the normaliser n_mel * F * B instead of n_mel * sum n
    clamp_grad   the clamp's gradient passed below the clip
    no_inv_melp  the 1 / melp of the log's derivative missing
    mag_pad      mag's pad columns left as the allocator gave them (NaN here) instead of 0
    sign_flip    the sign taken as target - mel
"""
import numpy as np

CLIP = 1e-5
CLIP32 = float(np.float32(1e-5))
BUGS = ("reflectS", "drop_mirror", "normBF", "clamp_grad", "no_inv_melp", "mag_pad", "sign_flip")
FIXTURES = ("small", "small_win", "shipped")


def round_up(n, m):
    return (n + m - 1) // m * m


class Geometry:
    def __init__(self, n_fft, hop, win, n_mel, B, S):
        self.n_fft, self.hop, self.win, self.n_mel, self.B, self.S = int(n_fft), int(hop), int(win), int(n_mel), int(B), int(S)
        self.h, self.cutoff = self.n_fft // 2, self.n_fft // 2 + 1
        self.F = 1 + self.S // self.hop
        self.rows = self.B * self.F
        self.lds, self.ldm, self.ldn = round_up(2 * self.cutoff, 4), round_up(self.cutoff, 4), round_up(self.n_mel, 4)


def fixture_geometry(d):
    n_fft, hop, win, n_mel = (int(v) for v in d["geometry"])
    return Geometry(n_fft, hop, win, n_mel, *d["x"].shape)


def forward_basis(n_fft, win):
    """[2 cutoff, n_fft]: the module's float32 buffer, as float64"""
    from rad_mmm_amd.audio_processing import windowed_dft_basis
    return windowed_dft_basis(n_fft, win).astype(np.float64)


def item_lens(lens, B, S):
    """lens as the kernels read them: clamped into [1, S]; None: S"""
    return np.full(B, S, dtype=np.int64) if lens is None else np.clip(np.asarray(lens, dtype=np.int64), 1, S)


def item_frames(lens, g):
    return 1 + item_lens(lens, g.B, g.S) // g.hop


def loss_frames(lens, frames, g, Ft):
    """n[b] = min(1 + lens[b] // hop, Ft, frames[b] clamped into [0, min(F, Ft)])"""
    n = np.minimum(item_frames(lens, g), min(g.F, Ft))
    if frames is not None:
        n = np.minimum(n, np.clip(np.asarray(frames, dtype=np.int64), 0, min(g.F, Ft)))
    return n


def frame_index(length, g, bug=None):
    """[F, n_fft] sample index of every frame column of an item of `length` samples: reflect(f*hop + j - h), clamped
    into the item"""
    p = np.arange(g.F)[:, None] * g.hop + np.arange(g.n_fft)[None, :] - g.h
    p = np.where(p < 0, -p, p)
    top = (g.S if bug == "reflectS" else length) - 1
    p = np.where(p > top, 2 * top - p, p)
    return np.clip(p, 0, top)


def frame(x, lens, g, bug=None):
    """x [B, >= S] -> A [B*F, n_fft] in x's dtype: the model of radmmm_melloss_frame"""
    L, nf = item_lens(lens, g.B, g.S), item_frames(lens, g)
    A = np.zeros((g.B, g.F, g.n_fft), dtype=x.dtype)
    for b in range(g.B):
        A[b, :nf[b]] = x[b][frame_index(L[b], g, bug)[:nf[b]]]
    return A.reshape(g.rows, g.n_fft)


def unframe(dA, lens, g, bug=None):
    """dA [B*F, n_fft] -> [B, S]: the adjoint of frame in gather form, in the kernel's order of additions (own position,
    left mirror, right mirror; frames ascending) and in dA's dtype: the model of radmmm_melloss_unframe"""
    L, nf = item_lens(lens, g.B, g.S), item_frames(lens, g)
    dA = dA.reshape(g.B, g.F, g.n_fft)
    out = np.zeros((g.B, g.S), dtype=dA.dtype)
    h, hop, n_fft = g.h, g.hop, g.n_fft

    def gather(b, P):
        if P < 0:
            return dA.dtype.type(0)
        f_hi = min(P // hop, nf[b] - 1)
        lo = P - n_fft + 1
        f_lo = -(-lo // hop) if lo > 0 else 0
        s = dA.dtype.type(0)
        for f in range(f_lo, f_hi + 1):
            s = s + dA[b, f, P - f * hop]
        return s

    for b in range(g.B):
        n = L[b]
        for s in range(n):
            v = gather(b, s + h)
            if 1 <= s <= h:
                v = v + gather(b, h - s)
            if n - 1 - h <= s <= n - 2 and bug != "drop_mirror":
                v = v + gather(b, h + 2 * (n - 1) - s)
            out[b, s] = v
    return out


def unframe_fast(dA, lens, g, bug=None):
    """the same adjoint as a scatter-add in float64 (where the order of additions does not matter)"""
    L, nf = item_lens(lens, g.B, g.S), item_frames(lens, g)
    dA = np.array(dA.reshape(g.B, g.F, g.n_fft), dtype=np.float64)
    out = np.zeros((g.B, g.S), dtype=np.float64)
    for b in range(g.B):
        idx = frame_index(L[b], g)[:nf[b]]
        w = dA[b, :nf[b]]
        if bug == "drop_mirror":
            p = np.arange(nf[b])[:, None] * g.hop + np.arange(g.n_fft)[None, :] - g.h
            w = w * (p <= L[b] - 1)
        np.add.at(out[b], idx.ravel(), w.ravel())
    return out


def valid_rows(nf, g):
    """[B*F] bool: f < nf[b]"""
    return (np.arange(g.F)[None, :] < np.asarray(nf)[:, None]).reshape(g.rows)


def mag(spec, lens, g, bug=None):
    """spec [rows, >= 2 cutoff] -> [rows, ldm]: sqrt(re^2 + im^2), zeros in the pad columns and the invalid rows"""
    re, im = spec[:, :g.cutoff], spec[:, g.cutoff:2 * g.cutoff]
    out = np.zeros((g.rows, g.ldm), dtype=spec.dtype)
    out[:, :g.cutoff] = np.sqrt(re * re + im * im)
    if bug == "mag_pad":
        out[:, g.cutoff:] = np.nan
    out[~valid_rows(item_frames(lens, g), g)] = 0
    return out


def pad_mel_basis(mel_basis, g):
    out = np.zeros((g.ldn, g.ldm), dtype=np.float64)
    out[:g.n_mel, :g.cutoff] = mel_basis
    return out


def to_layout(rows_c, g):
    """[B*F, n_mel] -> the reference layout [B, n_mel, F]"""
    return rows_c.reshape(g.B, g.F, g.n_mel).transpose(0, 2, 1)


def from_layout(mel, g, ld):
    """[B, n_mel, ld] -> [B*F, n_mel], zeros at frames >= ld"""
    out = np.zeros((g.B, g.F, g.n_mel), dtype=mel.dtype)
    k = min(g.F, ld)
    out[:, :k] = mel.transpose(0, 2, 1)[:, :k]
    return out.reshape(g.rows, g.n_mel)


def log_mel(melp, lens, g, clip=CLIP):
    """melp [rows, >= n_mel] -> log(max(melp, clip)) [rows, n_mel], zeros in rows past an item's frames.  clip: 1e-5 as the
    float64 reference reads it; the kernels (and the reference in float32) compare with float32(1e-5) = CLIP32"""
    with np.errstate(invalid="ignore"):
        out = np.log(np.maximum(melp[:, :g.n_mel], melp.dtype.type(clip)))
    out[~valid_rows(item_frames(lens, g), g)] = 0
    return out


def mel_forward(x, lens, g, mel_basis, bug=None):
    """-> dict(spec, mag, melp [rows, ldn], mel [rows, n_mel]) of one signal, float64"""
    fb = forward_basis(g.n_fft, g.win)
    A = frame(np.asarray(x, dtype=np.float64), lens, g, bug)
    spec = A @ fb.T
    m = mag(spec, lens, g, bug)
    melp = m @ pad_mel_basis(mel_basis, g).T
    return dict(spec=spec, mag=m, melp=melp, mel=log_mel(melp, lens, g))


def mel_backward(fw, dmelp, lens, g, mel_basis, bug=None, exact_order=False):
    """dmelp [rows, ldn] -> dx [B, S] (float64)"""
    dmag = dmelp @ pad_mel_basis(mel_basis, g)
    re, im = fw["spec"][:, :g.cutoff], fw["spec"][:, g.cutoff:2 * g.cutoff]
    m = np.sqrt(re * re + im * im)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(m > 0, dmag[:, :g.cutoff] / m, 0.0)       # the gradient of sqrt at re = im = 0 is 0
    dspec = np.concatenate([s * re, s * im], 1)
    dspec[~valid_rows(item_frames(lens, g), g)] = 0
    dA = dspec @ forward_basis(g.n_fft, g.win)
    return (unframe if exact_order else unframe_fast)(dA, lens, g, bug)


def plain_bwd(melp, dmel, lens, g, clip=CLIP):
    """upstream dmel [B, n_mel, F] -> dmelp [rows, ldn]: the model of radmmm_melloss_bwd without a target"""
    out = np.zeros((g.rows, g.ldn), dtype=np.float64)
    mp = melp[:, :g.n_mel]
    ok = valid_rows(item_frames(lens, g), g)[:, None] & (mp >= clip)
    with np.errstate(invalid="ignore", divide="ignore"):
        out[:, :g.n_mel] = np.where(ok, from_layout(np.asarray(dmel, dtype=np.float64), g, g.F) / mp, 0.0)
    return out


def loss_bwd(melp, mel, tgt_rows, n, g, grad=1.0, bug=None, clip=CLIP):
    """dmelp [rows, ldn] of grad * loss with respect to the melp that made `mel` (the other operand in rows as tgt_rows)"""
    cnt = float(g.F * g.B if bug == "normBF" else np.sum(n))
    coef = grad / (g.n_mel * cnt) if cnt > 0 else 0.0
    mp = melp[:, :g.n_mel]
    d = (tgt_rows - mel) if bug == "sign_flip" else (mel - tgt_rows)
    ok = valid_rows(n, g)[:, None] & (True if bug == "clamp_grad" else mp >= clip)
    out = np.zeros((g.rows, g.ldn), dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = coef * np.sign(d) / (1.0 if bug == "no_inv_melp" else mp)
        out[:, :g.n_mel] = np.where(ok, v, 0.0)
    return out


def mel_loss(x, target, lens, frames, g, mel_basis, bug=None, grad=1.0, exact_order=False):
    """The whole loss in float64.  target: a mel [B, n_mel, Ft] or audio [B, S].  -> dict(loss, norm, n, grad_x, grad_t (audio
    targets), part, fx = the forward of x, mel_x [B, n_mel, F])"""
    target = np.asarray(target)
    audio = target.ndim == 2
    fx = mel_forward(x, lens, g, mel_basis, bug)
    if audio:
        ft = mel_forward(target, lens, g, mel_basis, bug)
        Ft, tgt_rows = g.F, ft["mel"]
    else:
        Ft = target.shape[2]
        tgt_rows = from_layout(target.astype(np.float64), g, Ft)
    n = loss_frames(lens, frames, g, Ft)
    vr = valid_rows(n, g)
    part = np.where(vr, np.abs(fx["mel"] - tgt_rows).sum(1), 0.0)
    cnt = float(g.F * g.B if bug == "normBF" else n.sum())
    loss = part.sum() / (g.n_mel * cnt) if cnt > 0 else 0.0
    out = dict(loss=float(loss), norm=float(n.sum()), n=n, part=part, fx=fx, mel_x=to_layout(fx["mel"], g))
    out["grad_x"] = mel_backward(fx, loss_bwd(fx["melp"], fx["mel"], tgt_rows, n, g, grad, bug), lens, g, mel_basis, bug,
                                 exact_order)
    if audio:
        out["grad_t"] = mel_backward(ft, loss_bwd(ft["melp"], ft["mel"], fx["mel"], n, g, grad, bug), lens, g, mel_basis, bug,
                                     exact_order)
    return out


def fixture_inputs(d):
    """(x, target, lens, frames) of a fixture; absent lens / frames are None"""
    return d["x"], d["target"], d.get("lens"), d.get("frames")


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def fixture_bars(d):
    """the GPU tests' bars: losses max(10 |ref32 - ref64| / ref64, 1e-6) relative, gradients max(10 x the stored
    float32-against-float64 deviation, 1e-6) relative L2"""
    bars = {"loss": max(10.0 * abs(float(d["loss32"]) - float(d["loss64"])) / abs(float(d["loss64"])), 1e-6)}
    for k in d:
        if k.startswith("f32_vs_f64/grad_"):
            bars[k[len("f32_vs_f64/"):]] = max(10.0 * float(d[k]), 1e-6)
    return bars


def fixture_want(d):
    want = {"loss": float(d["loss64"]), "grad_x": d["grad/x"]}
    if "grad/t" in d:
        want["grad_t"] = d["grad/t"]
    return want


def measured_over_bar(got, want, bars):
    """{key: measured / bar} over the keys of bars; NaN or inf measure as inf"""
    out = {}
    for k, bar in bars.items():
        if np.ndim(want[k]) == 0:
            err = abs(float(got[k]) - float(want[k])) / abs(float(want[k]))
        else:
            err = rel_l2(got[k], want[k])
        out[k] = err / bar if np.isfinite(err) else np.inf
    return out


def silent_case(seed=0):
    """geometry 64 / 16 / 64, 12 mels, B = 2, S = 400, lens [400, 333]: item 0 holds 112 exact zeros from sample 128, so the
    four frames 10 .. 13 (padded positions 160 .. 271 = samples 128 .. 239) see nothing but zeros; samples 176 .. 191 lie
    in those four frames only.  -> (g, mel_basis, x, target mel, lens, frames, the silent frames, their own samples)"""
    from rad_mmm_amd.audio_processing import mel_filterbank
    g = Geometry(64, 16, 64, 12, 2, 400)
    mb = mel_filterbank(22050, 64, 12, 0.0, None)
    rng = np.random.RandomState(seed)
    x = (0.3 * rng.randn(2, 400)).astype(np.float32)
    x[0, 128:240] = 0
    lens = np.array([400, 333])
    x[1, 333:] = 0
    y = (x + 0.05 * rng.randn(2, 400)).astype(np.float32)
    y[0, 128:240] = 0
    target = to_layout(mel_forward(y, lens, g, mb)["mel"], g).astype(np.float32)
    return g, mb, x, np.ascontiguousarray(target), lens, None, (10, 14), (176, 192)


def forward_fp32_bar(x, lens, g, mel_basis):
    """Per element of the log-mel [B, n_mel, F]: how far ANY fp32 evaluation of frame -> DFT -> mag -> mel projection ->
    log-clamp may lie from the float64 model, whatever the order of its sums.  A K-term fp32 dot product is within
    gamma_K = K u / (1 - K u) of sum |a_k b_k| (u = 2^-24): e_spec = gamma_n_fft |A| |basis|^T.  |d mag| <= |d re| + |d im|
    plus 2u mag for the two squares, the sum and the root; e_melp = mel_basis (e_mag) + gamma_cutoff melp; log and the clamp
    are monotone, so the mel lies between log(max(melp -+ e_melp, clip)), widened by 4u |mel| for a logf within 2 ulp and by the
    difference between float32(1e-5) and 1e-5."""
    u = 2.0 ** -24
    gam = lambda k: k * u / (1 - k * u)   # noqa: E731
    fb = forward_basis(g.n_fft, g.win)
    fw = mel_forward(x, lens, g, mel_basis)
    A = frame(np.asarray(x, dtype=np.float64), lens, g)
    e_spec = gam(g.n_fft) * (np.abs(A) @ np.abs(fb).T)
    e_mag = e_spec[:, :g.cutoff] + e_spec[:, g.cutoff:2 * g.cutoff] + 2 * u * fw["mag"][:, :g.cutoff]
    mb = np.asarray(mel_basis, dtype=np.float64)
    melp = fw["melp"][:, :g.n_mel]
    e_melp = e_mag @ mb.T + gam(g.cutoff) * melp
    lo = np.log(np.maximum(melp - e_melp, min(CLIP, CLIP32)))
    hi = np.log(np.maximum(melp + e_melp, max(CLIP, CLIP32)))
    bar = np.maximum(hi - fw["mel"], fw["mel"] - lo) + 4 * u * np.abs(fw["mel"])
    bar[~valid_rows(item_frames(lens, g), g)] = 0
    return to_layout(bar, g), to_layout(fw["mel"], g)
