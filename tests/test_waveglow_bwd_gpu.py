"""GPU checks of WaveGlow training (rad_mmm_amd/waveglow.py nll_loss / forward in training mode / apply_weight_norm, the
radmmm_wg_coupling_bwd / wg_gate_bwd / wg_start_bwd / wg_outer_reduce / wg_inv_logdet / wg_ungroup_cond kernels of
csrc/waveglow.hip): the reference's recorded gradients (tests/golden/waveglow_bwd_tiny.npz), the reference's own
training lines, ragged batches against the float64 restatement, chunking, one case at the shipped WN size, every new
kernel directly against float64, no device -> host synchronisation, eval mode untouched, three Adam steps."""
import re

import numpy as np
import pytest
import torch

from _waveglow_bwd_ref import grads_ref, leaves_of, loss_ref, rel_l2
from _waveglow_ref import HOP, SHIPPED_WN, load_fixture, random_state

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
RAGGED = [9, 1, 5, 3, 2]


def _train_model(cfg, sd, weight_norm=True):
    from rad_mmm_amd.waveglow import WaveGlow
    m = WaveGlow(**cfg)
    if weight_norm:
        m.apply_weight_norm()
    m.load_state_dict(sd)
    return m.to(DEV).train()


def _grads(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def _step(m, mel, audio, lens=None):
    m.zero_grad(set_to_none=True)
    loss = m.nll_loss(mel, audio, lens)
    loss.backward()
    return loss.detach(), _grads(m)


def _same_bits(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.fixture(scope="module")
def tiny(golden):
    """the two fixtures, the weight-normed model in training mode, the equal-length batch and one nll_loss step on it"""
    fwd, bwd = golden("waveglow_fwd_tiny.npz"), golden("waveglow_bwd_tiny.npz")
    cfg, sd = load_fixture(fwd)
    m = _train_model(cfg, sd)
    n = int(fwd["eq_T"])
    mel = torch.from_numpy(fwd["mel"][:, :, :n].copy()).to(DEV)
    audio = torch.from_numpy(fwd["audio"][:, :n * HOP].copy()).to(DEV)
    loss, grads = _step(m, mel, audio)
    return fwd, bwd, cfg, sd, m, mel, audio, loss, grads


def _bars(bwd):
    return {k[len("f32_vs_f64/"):]: max(10 * float(v), 1e-6) for k, v in bwd.items() if k.startswith("f32_vs_f64/")}


def _check_against_fixture(bwd, grads, what):
    bars = _bars(bwd)
    assert set(grads) >= set(bars)
    worst, bad = 0.0, []
    for k, bar in sorted(bars.items()):
        err = rel_l2(grads[k].cpu().numpy(), bwd["grad/" + k])
        worst = max(worst, err / bar)
        print(f"{what} {k}: relative L2 {err:.3e} (bar {bar:.3e})")
        if not err <= bar:
            bad.append((k, err, bar))
    print(f"{what}: worst measured / bar {worst:.3f}")
    assert not bad, bad


def test_nll_loss_gradients_match_the_reference_fixture(tiny):
    fwd, bwd, cfg, sd, m, mel, audio, loss, grads = tiny
    bar = max(10 * float(fwd["f32_vs_f64_loss"]), 1e-6)
    print(f"loss {float(loss):.9f}, {abs(float(loss) - float(bwd['loss64'])):.3e} from the reference's float64 (bar {bar:.3e})")
    assert loss.dtype == torch.float64 and abs(float(loss) - float(bwd["loss64"])) <= bar
    assert set(grads) == set(sd) and mel.grad is None and audio.grad is None
    _check_against_fixture(bwd, grads, "nll_loss")


def test_reference_training_lines(tiny):
    from rad_mmm_amd.waveglow import WaveGlowLoss
    fwd, bwd, cfg, sd, m, mel, audio, loss1, grads1 = tiny
    m.zero_grad(set_to_none=True)
    out = m((mel, audio))
    assert out[0].grad_fn is not None and all(t.grad_fn is not None for t in out[1] + out[2])
    loss = WaveGlowLoss(1.0)(out)
    loss.backward()
    grads = _grads(m)
    assert abs(float(loss.detach()) - float(loss1)) <= 1e-9
    _check_against_fixture(bwd, grads, "forward + WaveGlowLoss")
    worst = max(rel_l2(grads[k].cpu().numpy(), grads1[k].cpu().numpy()) for k in grads1)
    print(f"forward + WaveGlowLoss against nll_loss: worst relative L2 {worst:.3e}")
    assert worst <= 1e-6


@pytest.fixture(scope="module")
def ragged(tiny):
    """the forward test's ragged batch, one training step on it and the float64 restatement's gradients"""
    fwd, bwd, cfg, sd, m, _, _, _, _ = tiny
    g = torch.Generator().manual_seed(19)
    T = max(RAGGED)
    mel = torch.randn(len(RAGGED), 8, T, generator=g) - 2.0
    audio = 0.3 * torch.randn(len(RAGGED), T * HOP, generator=g)
    ref_loss, ref = grads_ref(sd, cfg, mel, audio, RAGGED)
    mel, audio = mel.to(DEV), audio.to(DEV)
    loss, grads = _step(m, mel, audio, RAGGED)
    return mel, audio, loss, grads, ref_loss, ref


def _class_bars(bwd, names):
    """per parameter: the fixture entry of the same parameter, or of its class (the name without its flow number) at
    its largest"""
    bars = _bars(bwd)
    by_class = {}
    for k, v in bars.items():
        c = re.sub(r"^(WN|convinv)\.\d+\.", r"\1.*.", k)
        by_class[c] = max(by_class.get(c, 0.0), v)
    return {k: bars.get(k, by_class[re.sub(r"^(WN|convinv)\.\d+\.", r"\1.*.", k)]) for k in names}


def test_ragged_batch(tiny, ragged):
    fwd, bwd, cfg, sd, m, _, _, _, _ = tiny
    mel, audio, loss, grads, ref_loss, ref = ragged
    bar = max(10 * float(fwd["f32_vs_f64_loss"]), 1e-6)
    print(f"ragged loss {float(loss):.9f}, {abs(float(loss) - ref_loss):.3e} from the restatement (bar {bar:.3e})")
    assert abs(float(loss) - ref_loss) <= bar
    bars = _class_bars(bwd, ref)
    assert set(grads) == set(ref)
    bad = []
    for k in sorted(ref):
        err = rel_l2(grads[k].cpu().numpy(), ref[k].numpy())
        print(f"ragged {k}: relative L2 {err:.3e} (bar {bars[k]:.3e})")
        if not err <= bars[k]:
            bad.append((k, err, bars[k]))
        assert torch.isfinite(grads[k]).all(), k
    assert not bad, bad
    loss2, again = _step(m, mel, audio, RAGGED)                                  # two steps: the same bits
    assert torch.equal(loss, loss2) and _same_bits(grads, again)
    dl = torch.tensor(RAGGED, dtype=torch.int32, device=DEV)                     # device lengths: the same bits
    loss3, dev = _step(m, mel, audio, dl)
    assert torch.equal(loss, loss3) and _same_bits(grads, dev)
    poisoned = audio.clone()
    for b, n in enumerate(RAGGED):
        poisoned[b, n * HOP:] = float("nan")
    loss4, nan = _step(m, mel, poisoned, RAGGED)                                 # what lies past a length reaches nothing
    assert torch.equal(loss, loss4) and _same_bits(grads, nan)


def test_chunked_step(tiny, ragged):
    m = tiny[4]
    mel, audio, loss, grads, _, _ = ragged
    m._train_chunk_items = 2
    try:
        loss2, chunked = _step(m, mel, audio, RAGGED)
    finally:
        m._train_chunk_items = None
    worst = max(rel_l2(chunked[k].cpu().numpy(), grads[k].cpu().numpy()) for k in grads)
    print(f"chunks of 2 items: worst relative L2 {worst:.3e}, loss {abs(float(loss2) - float(loss)):.3e}")
    assert worst <= 1e-6 and abs(float(loss2) - float(loss)) <= 1e-12


def test_shipped_wn_size_against_fp64_restatement():
    # n_channels 256, n_layers 8: dilation 128 and K = 768; one item of 2 frames = 64 group steps, fewer than the largest
    # dilation: the forward test's case.  Bar: its relative-L2 bar.
    cfg = dict(n_mel_channels=80, n_flows=2, n_group=8, n_early_every=4, n_early_size=2, WN_config=SHIPPED_WN)
    sd = random_state(cfg, 7)
    m = _train_model(cfg, sd, weight_norm=False)
    g = torch.Generator().manual_seed(8)
    T = 2
    mel = torch.randn(1, 80, T, generator=g) - 2.0
    audio = 0.3 * torch.randn(1, T * HOP, generator=g)
    ref_loss, ref = grads_ref(sd, cfg, mel, audio, [T])
    loss, grads = _step(m, mel.to(DEV), audio.to(DEV), [T])
    print(f"shipped WN size: loss {float(loss):.7f} against {ref_loss:.7f}")
    bad = []
    for k in sorted(ref):
        err = rel_l2(grads[k].cpu().numpy(), ref[k].numpy())
        print(f"shipped WN size {k}: relative L2 {err:.3e}")
        if not err <= 1e-5:
            bad.append((k, err))
    assert not bad, bad


# ---- the new kernels directly, against float64 -----------------------------------------------------------------------
# Elementwise outputs: 1e-6 * max|ref|.  Row-reduced outputs: the worst case of an fp32 sum of n terms in any order,
# n * 2^-24 * sum|term| per output element (the products enter the sums through fma: no rounding of their own).

def _lib():
    from rad_mmm_amd._lib import check, lib, ptr, stream
    return check, lib, ptr, stream()


LENS, TG = [37, 32, 1, 300], 300        # group steps: 1200 rows = 75 passes of 16 rows and 4.7 blocks of 256 rows
R = len(LENS) * TG
C = 32


def _mask():
    return (torch.arange(TG)[None, :] < torch.tensor(LENS)[:, None]).reshape(-1)


def _lens():
    return torch.tensor(LENS, dtype=torch.int32, device=DEV)


def _poisoned(g, *shape):
    x = torch.randn(*shape, generator=g)
    x[~_mask()] = float("nan")                  # rows past a length: never read
    return x


def _elementwise(name, got, ref):
    err = (got.double() - ref).abs().max().item()
    bar = 1e-6 * ref.abs().max().item()
    print(f"  {name}: max-abs {err:.3e} (bar {bar:.3e})")
    assert err <= bar, name


def _outer_reduce(A, lda, M, Bm, ldb, N):
    """the kernel on device views, and its bar from the same float32 inputs"""
    check, lib, ptr, s = _lib()
    Mk = M if A is not None else 1
    out = torch.full((Mk, N), 7.0, device=DEV)
    scratch = torch.empty(int(lib.radmmm_wg_outer_reduce_scratch_floats(R, Mk, N)), device=DEV)
    check(lib.radmmm_wg_outer_reduce(ptr(A), lda, M, ptr(Bm), ldb, N, ptr(out), ptr(scratch), ptr(_lens()), R, TG, s),
          "wg_outer_reduce")
    return out.cpu()


def _reduced(name, got, a, b):
    """got [M, N] against sum_r a[r, m] * b[r, n] over the valid rows (a, b: float32 values on the host)"""
    mask = _mask()
    a, b = a[mask].double(), b[mask].double()
    terms = a[:, :, None] * b[:, None, :]
    ref, bar = terms.sum(0), int(mask.sum()) * 2.0 ** -24 * terms.abs().sum(0)
    err = (got.double() - ref).abs()
    print(f"  {name}: worst error / bar {(err / bar).max().item():.3f} (max-abs {err.max().item():.3e})")
    assert bool((err <= bar).all()), name


@pytest.mark.parametrize("c,ldx", [(4, 8), (6, 8), (8, 8), (8, 9)])
def test_coupling_and_mix_backward_kernels(c, ldx):
    check, lib, ptr, s = _lib()
    g = torch.Generator().manual_seed(40 + c + ldx)
    nh, col0 = c // 2, ldx - c
    mask, lens = _mask(), _lens()
    S, Xs, dX0 = _poisoned(g, R, C), _poisoned(g, R, ldx), _poisoned(g, R, ldx)
    We, be = 0.05 * torch.randn(c, C, generator=g), 0.05 * torch.randn(c, generator=g)
    o = torch.nan_to_num(S).double() @ We.double().T + be.double()
    e = torch.exp(o[:, nh:])
    g1, x1 = torch.nan_to_num(dX0[:, col0 + nh:]).double(), torch.nan_to_num(Xs[:, col0 + nh:]).double()
    for rows_mode in (False, True):                         # one value for all rows (nll_loss); materialised rows
        gls = _poisoned(g, R, nh) if rows_mode else torch.tensor([-0.37])
        gref = torch.nan_to_num(gls).double() if rows_mode else gls.double()
        dX = dX0.clone().to(DEV)
        dO = torch.full((R, c), 7.0, device=DEV)
        dS = torch.full((R, 2 * C), 7.0, device=DEV)          # the right half of a [R, 2 C] buffer, as the step uses it
        Sd, Wed, bed, Xd, gd = S.to(DEV), We.to(DEV), be.to(DEV), Xs.to(DEV), gls.to(DEV)
        check(lib.radmmm_wg_coupling_bwd(ptr(Sd), C, ptr(Wed), ptr(bed), ptr(Xd), ldx, ptr(dX), ldx, col0, nh, C, ptr(gd),
                                         nh if rows_mode else 0, ptr(dO), ptr(dS[:, C:]), 2 * C, ptr(lens), R, TG, s),
              "wg_coupling_bwd")
        print(f"coupling backward, c = {c}, ldx = {ldx}, g_ls {'rows' if rows_mode else 'one value'}:")
        dO_ref = torch.cat([g1, g1 * e * x1 + gref], 1) * mask[:, None]
        got_dO, got_dX, got_dS = dO.cpu(), dX.cpu(), dS.cpu()
        _elementwise("dO", got_dO, dO_ref)
        _elementwise("dX1", got_dX[:, col0 + nh:], g1 * e * mask[:, None])
        _elementwise("dS", got_dS[:, C:], dO_ref @ We.double())
        assert bool((got_dS[:, :C] == 7.0).all())
        keep = got_dX[:, :col0 + nh]                        # X0's gradient and the columns in front: not touched
        assert torch.equal(keep[mask], dX0[:, :col0 + nh][mask]) and bool(keep[~mask].isnan().all())
        assert not got_dO[~mask].any() and not got_dS[~mask][:, C:].any() and not got_dX[~mask][:, col0 + nh:].any()
        # the weight and bias gradients of `end` from the kernel's own float32 dO
        _reduced("dWend", _outer_reduce(dO, c, c, Sd, C, C), got_dO, torch.nan_to_num(S))
        _reduced("dbend", _outer_reduce(None, 0, 1, dO, c, c), torch.ones(R, 1), got_dO)

    # the 1x1 mix: dW from the gradient of its output and its saved input, then the data gradient in place
    W = (torch.linalg.qr(torch.randn(c, c, generator=g))[0] + 0.1 * torch.randn(c, c, generator=g)).contiguous()
    Xin, G0 = _poisoned(g, R, ldx), _poisoned(g, R, ldx)
    Xind, G = Xin.to(DEV), G0.clone().to(DEV)
    print(f"mix backward, c = {c}, ldx = {ldx}:")
    _reduced("dW", _outer_reduce(G[:, col0:], ldx, c, Xind[:, col0:], ldx, c), torch.nan_to_num(G0[:, col0:]),
             torch.nan_to_num(Xin[:, col0:]))
    Wt = W.t().contiguous().to(DEV)
    check(lib.radmmm_wg_mix_fwd(ptr(G), ldx, col0, c, ptr(Wt), ptr(lens), R, TG, s), "wg_mix_fwd")
    got = G.cpu()
    _elementwise("dX_in", got[:, col0:], (torch.nan_to_num(G0[:, col0:]).double() @ W.double()) * mask[:, None])
    assert torch.equal(got[:, :col0][mask], G0[:, :col0][mask]) and not got[~mask][:, col0:].any()


@pytest.mark.parametrize("nh", [2, 3, 4])
def test_start_backward_kernel(nh):
    check, lib, ptr, s = _lib()
    g = torch.Generator().manual_seed(50 + nh)
    ldx, col0 = 8, 8 - 2 * nh
    mask, lens = _mask(), _lens()
    dH, X, dX0 = _poisoned(g, R, 2 * C), _poisoned(g, R, ldx), _poisoned(g, R, ldx)   # dH: the left half of [R, 2 C]
    Ws = torch.randn(C, nh, generator=g)
    dHd, Xd, dX = dH.to(DEV), X.to(DEV), dX0.clone().to(DEV)
    print(f"start backward, n_half = {nh}:")
    _reduced("dWs", _outer_reduce(Xd[:, col0:], ldx, nh, dHd, 2 * C, C), torch.nan_to_num(X[:, col0:col0 + nh]),
             torch.nan_to_num(dH[:, :C]))
    _reduced("dbs", _outer_reduce(None, 0, 1, dHd, 2 * C, C), torch.ones(R, 1), torch.nan_to_num(dH[:, :C]))
    Wt = Ws.t().contiguous().to(DEV)
    check(lib.radmmm_wg_start_bwd(ptr(dHd), 2 * C, ptr(Wt), ptr(dX), ldx, col0, nh, C, ptr(lens), R, TG, s),
          "wg_start_bwd")
    got = dX.cpu()
    ref = torch.nan_to_num(dX0[:, col0:col0 + nh]).double() + torch.nan_to_num(dH[:, :C]).double() @ Ws.double()
    _elementwise("dX0", got[mask][:, col0:col0 + nh], ref[mask])
    rest = torch.ones(ldx, dtype=torch.bool)
    rest[col0:col0 + nh] = False
    assert torch.equal(got[mask][:, rest], dX0[mask][:, rest]) and bool(got[~mask].isnan().all())


def test_gate_backward_kernel():
    check, lib, ptr, s = _lib()
    g = torch.Generator().manual_seed(60)
    L, i = 3, 1
    mask, lens = _mask(), _lens()
    A, cond, gy = _poisoned(g, R, 2 * C), _poisoned(g, R, 2 * C * L), _poisoned(g, R, C)
    dcond = torch.full((R, 2 * C * L), 7.0, device=DEV)
    Ad, cd, gd = A.to(DEV), cond.to(DEV), gy.to(DEV)
    check(lib.radmmm_wg_gate_bwd(ptr(Ad), 2 * C, ptr(cd), 2 * C * L, 2 * C * i, ptr(gd), C, ptr(dcond[:, 2 * C * i:]),
                                 2 * C * L, C, ptr(lens), R, TG, s), "wg_gate_bwd")
    a = torch.nan_to_num(A).double() + torch.nan_to_num(cond[:, 2 * C * i:2 * C * (i + 1)]).double()
    t, sg, gg = torch.tanh(a[:, :C]), torch.sigmoid(a[:, C:]), torch.nan_to_num(gy).double()
    ref = torch.cat([gg * sg * (1 - t * t), gg * t * sg * (1 - sg)], 1) * mask[:, None]
    got = dcond.cpu()
    print("gate backward:")
    _elementwise("dA", got[:, 2 * C * i:2 * C * (i + 1)], ref)
    assert not got[~mask][:, 2 * C * i:2 * C * (i + 1)].any()
    assert bool((got[:, :2 * C * i] == 7.0).all()) and bool((got[:, 2 * C * (i + 1):] == 7.0).all())


def test_inverse_and_logdet_kernel(golden):
    from rad_mmm_amd.waveglow import inv_logdet
    cfg, sd = load_fixture(golden("waveglow_fwd_tiny.npz"))
    mats = [sd[f"convinv.{k}.conv.weight"][:, :, 0].contiguous() for k in range(cfg["n_flows"])]
    neg = mats[0].clone()
    neg[[0, 1]] = neg[[1, 0]]                               # two rows swapped: a negative determinant
    mats.append(neg)
    invs, logdet = inv_logdet([w.to(DEV) for w in mats])
    for k, w in enumerate(mats):
        w64 = w.double().numpy()
        sign, ld = np.linalg.slogdet(w64)
        ref = np.linalg.inv(w64)
        err, eld = np.abs(invs[k].cpu().double().numpy() - ref).max(), abs(float(logdet[k]) - ld)
        print(f"matrix {k} ({w.shape[0]} x {w.shape[0]}, sign {sign:+.0f}): W^-1 max-abs {err:.3e} (|ref| max "
              f"{np.abs(ref).max():.3f}), log|det| {ld:+.6f} off by {eld:.3e}")
        assert err <= 1e-6 * np.abs(ref).max() and eld <= 1e-12
    assert np.linalg.slogdet(neg.double().numpy())[0] < 0


def test_ungroup_cond_inverts_group_cond():
    check, lib, ptr, s = _lib()
    n_mel, ng, B = 5, 8, len(LENS)
    ldr = 44                                                # n_mel * ng = 40 and four columns of padding
    lens = _lens()
    valid = (torch.arange(TG * ng)[None, :] < (torch.tensor(LENS) * ng)[:, None])
    onehot = torch.zeros(B, TG * ng, n_mel)
    onehot[0, 3 * ng + 5, 2] = 1.0
    distinct = torch.arange(B * TG * ng * n_mel, dtype=torch.float32).reshape(B, TG * ng, n_mel) % 9973 + 1.0
    for up in (onehot, distinct):
        upd = up.to(DEV)
        rows = torch.full((B * TG, ldr), 7.0, device=DEV)
        check(lib.radmmm_wg_group_cond(ptr(upd), TG * ng * n_mel, ptr(rows), ldr, ptr(lens), B, TG, n_mel, ng, s),
              "wg_group_cond")
        rows[~_mask().to(DEV)] = float("nan")               # rows past a length: never read
        back = torch.full((B, TG * ng, n_mel), 7.0, device=DEV)
        check(lib.radmmm_wg_ungroup_cond(ptr(rows), ldr, ptr(back), TG * ng * n_mel, ptr(lens), B, TG, n_mel, ng, s),
              "wg_ungroup_cond")
        back = back.cpu()
        assert torch.equal(back[valid], up[valid]) and not back[~valid].any()


# ---- the step as a whole ---------------------------------------------------------------------------------------------

def test_no_device_to_host_sync_with_host_lengths(tiny):
    fwd, _, _, _, m = tiny[:5]
    mel, audio = torch.from_numpy(fwd["mel"]).to(DEV), torch.from_numpy(fwd["audio"]).to(DEV)
    _step(m, mel, audio, [7, 4])                             # warm
    torch.cuda.synchronize()
    m.zero_grad(set_to_none=True)
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = m.nll_loss(mel, audio, [7, 3])
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert loss.is_cuda and torch.isfinite(loss) and all(torch.isfinite(p.grad).all() for p in m.parameters())


def test_eval_mode_is_untouched(tiny):
    fwd, _, _, _, m, mel, audio = tiny[:7]
    try:
        m.eval()
        ev_a, ev_f = m.analyze(mel, audio), m((mel, audio))
        assert all(v.grad_fn is None for v in ev_a.values())
        assert ev_f[0].grad_fn is None and all(t.grad_fn is None for t in ev_f[1] + ev_f[2])
        assert m.nll_loss(mel, audio).grad_fn is None and torch.equal(m.nll_loss(mel, audio), ev_a["loss"])
        m.train()
        tr_a, tr_f = m.analyze(mel, audio), m((mel, audio))
        with torch.no_grad():
            ng_f = m((mel, audio))
    finally:
        m.train()
    assert all(torch.equal(ev_a[k], tr_a[k]) for k in ev_a)
    assert torch.equal(ev_f[0], tr_f[0]) and all(torch.equal(a, b) for a, b in zip(ev_f[1], tr_f[1]))
    assert ng_f[0].grad_fn is None and torch.equal(ev_f[0], ng_f[0])
    assert all(torch.equal(a, b) for a, b in zip(ev_f[2], ng_f[2]))
    # log|det W|: the training path takes it from the device kernel, the eval path from the host's LU; both float64
    worst = max(abs(float(a) - float(b.detach())) / mel.shape[0] / ev_f[0].shape[2] for a, b in zip(ev_f[2], tr_f[2]))
    print(f"log|det W| of the training path against the eval path: {worst:.3e}")
    assert worst <= 1e-12


def test_three_adam_steps(tiny):
    fwd, bwd, cfg, sd, _, mel, audio = tiny[:7]
    n = mel.shape[2]
    leaves = leaves_of(sd)
    opt = torch.optim.Adam(list(leaves.values()), lr=1e-4)
    want = []
    for _ in range(3):
        opt.zero_grad()
        loss = loss_ref(leaves, cfg, mel.cpu(), audio.cpu(), [n, n])
        loss.backward()
        opt.step()
        want.append(float(loss.detach()))
    runs = []
    for _ in range(2):
        m = _train_model(cfg, sd)
        opt = torch.optim.Adam(m.parameters(), lr=1e-4)
        losses = []
        for _ in range(3):
            opt.zero_grad()
            loss = m.nll_loss(mel, audio)
            loss.backward()
            opt.step()
            losses.append(loss.detach())
        runs.append((torch.stack(losses), {k: v.detach().clone() for k, v in m.state_dict().items()}))
    bar = 10 * max(10 * float(fwd["f32_vs_f64_loss"]), 1e-6)
    got = runs[0][0].tolist()
    print(f"three Adam steps: losses {got} against {want} (bar {bar:.3e})")
    assert want[2] < want[0]
    assert all(abs(a - b) <= bar for a, b in zip(got, want))
    assert torch.equal(runs[0][0], runs[1][0]) and _same_bits(runs[0][1], runs[1][1])
