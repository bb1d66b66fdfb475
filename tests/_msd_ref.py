"""A torch restatement of the HiFi-GAN multi-scale discriminator and the three GAN losses, written from the formulas (DESIGN
4.23), in any floating dtype on the CPU: weight norm, spectral norm with its power iteration, the pools, the eight convs of a
member, the masked losses.  tests/test_msd_cpu.py holds it against the reference's own figures (tests/golden/msd_*.npz); the
GPU tests use its float64 run where no fixture exists and its float32 run for the bars.

A state dict is the reference's: discriminators.0 under spectral norm (weight_orig, weight_u, weight_v, bias), .1 and .2 under
weight norm (weight_g, weight_v, bias), or plain (weight, bias).  The groups of a conv are read off its weight's shape.

`flaw` plants ONE error into the restatement (tests/test_msd_cpu.py shows that each misses the bars of the GPU tests by a wide
factor): one_iteration, same_weight, sigma_before_update, pool_divisor, pool_length, groups_transposed, stride_1, pad_2,
slope_001, floor, no_channels, factor_2."""
import numpy as np
import torch
import torch.nn.functional as F

KERNELS = (15, 41, 41, 41, 41, 41, 5, 3)
STRIDES = (1, 2, 2, 4, 4, 1, 1, 1)
SLOPE = 0.1
KINK_FACTOR = 8.0
LAYERS = [f"convs.{l}." for l in range(7)] + ["conv_post."]


def relative_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _normalize(x, eps=1e-12):
    return x / torch.clamp(x.norm(), min=eps)


def spectral_fold(w, u, v, training, flaw=None):
    """one module call of spectral norm -> (W / sigma, u', v'): in training mode v' = normalize(W^T u), u' = normalize(W v'),
    sigma = u' . (W v') with u', v' constants; in eval mode u, v as they are"""
    wm = w.flatten(1)
    u0, v0 = u, v
    if training:
        with torch.no_grad():
            v = _normalize(wm.t() @ u)
            u = _normalize(wm @ v)
    if flaw == "sigma_before_update":
        return w / torch.dot(u0, wm @ v0), u, v
    return w / torch.dot(u, wm @ v), u, v


def _leaves(sd, dtype):
    """the state dict as tensors of dtype; parameters require grad, the power-iteration vectors do not"""
    out = {}
    for k, v in sd.items():
        t = torch.as_tensor(np.asarray(v)).to(dtype).clone()
        if not k.endswith("weight_u") and not (k.endswith("weight_v") and k[:-1] + "u" in sd):
            t.requires_grad_(True)
        out[k] = t
    return out


def _member_weights(p, i, training, calls, flaw=None):
    """-> (per call a list of 8 (weight, bias), {name: vector after the calls})"""
    sets, after = [[] for _ in range(calls)], {}
    for name in LAYERS:
        pre = f"discriminators.{i}.{name}"
        b = p[pre + "bias"]
        if pre + "weight_orig" in p:
            u, v = p[pre + "weight_u"], p[pre + "weight_v"]
            for c in range(calls):
                if c == 0 or flaw not in ("one_iteration", "same_weight"):
                    w, u, v = spectral_fold(p[pre + "weight_orig"], u, v, training, flaw)
                elif flaw == "one_iteration":       # the second call folds again but does not iterate
                    w, u, v = spectral_fold(p[pre + "weight_orig"], u, v, False, flaw)
                sets[c].append((w, b))
            after[pre + "weight_u"], after[pre + "weight_v"] = u.detach(), v.detach()
        else:
            if pre + "weight_g" in p:
                vv, g = p[pre + "weight_v"], p[pre + "weight_g"]
                w = vv * (g / vv.flatten(1).norm(dim=1).reshape(-1, 1, 1))
            else:
                w = p[pre + "weight"]
            for c in range(calls):
                sets[c].append((w, b))
    return sets, after


def pool(x, flaw=None):
    """AvgPool1d(4, 2, padding 2), the zero pad counted: [B, 1, T] -> [B, 1, T // 2 + 1]"""
    win = F.pad(x, (2, 2)).unfold(-1, 4, 2)
    if flaw == "pool_length":
        win = win[..., :x.shape[-1] // 2, :]
    if flaw == "pool_divisor":
        cnt = F.pad(torch.ones_like(x), (2, 2)).unfold(-1, 4, 2)[..., :win.shape[-2], :].sum(-1)
        return win.sum(-1) / cnt
    return win.sum(-1) / 4


def member(x, wb, flaw=None, inputs=None):
    """[B, 1, T] through the eight convs -> (output [B, H], the eight maps [B, C, H])"""
    fmap = []
    for l, (w, b) in enumerate(wb):
        k, st = KERNELS[l], STRIDES[l]
        groups = x.shape[1] // w.shape[1]
        pad = k // 2
        if l == 2 and flaw == "stride_1":
            st = 1
        if l == 7 and flaw == "pad_2":           # conv_post padded as the 5-tap conv before it
            pad = 2
        if l == 1 and flaw == "groups_transposed" and groups > 1:
            co, ci = w.shape[0] // groups, w.shape[1]
            if co == ci:          # the (group, channel) order of the OUTPUT channels swapped
                w = w.reshape(groups, co, ci, k).transpose(1, 2).reshape(groups * co, ci, k)
            else:
                w = w.reshape(groups, co, ci, k).transpose(0, 1).reshape(groups * co, ci, k)
        x = F.conv1d(x, w, b, stride=st, padding=pad, groups=groups)
        if l < 7:
            if inputs is not None:
                inputs.append(x.detach().double().reshape(-1))
            x = torch.where(x > 0, x, x * (0.01 if flaw == "slope_001" else SLOPE))
        fmap.append(x)
    return x.flatten(1), fmap


def forward(p, y, y_hat, training=True, flaw=None, inputs=None):
    """-> (y_d_rs, y_d_gs, fmap_rs, fmap_gs, the spectral-norm vectors after the call)"""
    n = 1 + max(int(k.split(".")[1]) for k in p)
    rs, gs, frs, fgs, after = [], [], [], [], {}
    for i in range(n):
        if i:
            y, y_hat = pool(y, flaw), pool(y_hat, flaw)
        sets, aft = _member_weights(p, i, training, 2, flaw)
        after.update(aft)
        r, fr = member(y, sets[0], flaw, inputs)
        g, fg = member(y_hat, sets[0] if flaw == "same_weight" else sets[1], flaw, inputs)
        rs.append(r), gs.append(g), frs.append(fr), fgs.append(fg)
    return rs, gs, frs, fgs, after


def _mask(ratios, size, like, flaw=None):
    """[B, size]: item b counts ceil(ratios[b] * size) positions (evaluated in ratios' dtype)"""
    if ratios is None:
        return torch.ones(like.shape[0], size, dtype=like.dtype, device=like.device)
    r = torch.as_tensor(ratios, device=like.device)
    lens = (r * size).floor() if flaw == "floor" else (r * size).ceil()
    return (torch.arange(size, device=like.device)[None, :] < lens.long()[:, None]).to(like.dtype)


def feature_loss(frs, fgs, ratios=None, flaw=None):
    loss = 0
    for fr, fg in zip(frs, fgs):
        for r, g in zip(fr, fg):
            m = _mask(ratios, r.shape[2], r, flaw)
            loss = loss + ((r - g).abs() * m[:, None, :]).sum() / (m.sum() * (1 if flaw == "no_channels" else r.shape[1]))
    return loss * 2 if flaw == "factor_2" else loss


def generator_loss(gs, ratios=None, flaw=None):
    loss = 0
    for g in gs:
        m = _mask(ratios, g.shape[1], g, flaw)
        loss = loss + ((1 - g) ** 2 * m).sum() / m.sum()
    return loss


def discriminator_loss(rs, gs, ratios=None, flaw=None):
    r_l, g_l = [], []
    for r, g in zip(rs, gs):
        m = _mask(ratios, r.shape[1], r, flaw)
        r_l.append(((1 - r) ** 2 * m).sum() / m.sum())
        g_l.append((g ** 2 * m).sum() / m.sum())
    r_l, g_l = torch.stack(r_l), torch.stack(g_l)
    return (r_l + g_l).sum(), r_l, g_l


def run(sd, y, y_hat, ratios, dtype=torch.float64, training=True, w_fm=2.0, w_gen=1.0, w_disc=1.0, flaw=None):
    """L = w_fm fm + w_gen gen + w_disc disc and its gradients -> dict (numpy, float64)"""
    p = _leaves(sd, dtype)
    yy = torch.as_tensor(np.asarray(y)).to(dtype).clone().requires_grad_(True)
    yh = torch.as_tensor(np.asarray(y_hat)).to(dtype).clone().requires_grad_(True)
    inputs = []
    rs, gs, frs, fgs, after = forward(p, yy, yh, training, flaw, inputs)
    fm, gen = feature_loss(frs, fgs, ratios, flaw), generator_loss(gs, ratios, flaw)
    disc, r_l, g_l = discriminator_loss(rs, gs, ratios, flaw)
    (w_fm * fm + w_gen * gen + w_disc * disc).backward()
    grad = {k: v.grad.double().numpy() for k, v in p.items() if v.requires_grad and v.grad is not None}
    grad["y_hat"] = yh.grad.double().numpy()
    diffs = torch.cat([(r - g).detach().double().reshape(-1) for fr, fg in zip(frs, fgs) for r, g in zip(fr, fg)])
    return {"fm": float(fm.detach()), "gen": float(gen.detach()), "disc": float(disc.detach()), "r_losses": r_l.detach().double().numpy(),
            "g_losses": g_l.detach().double().numpy(), "grad": grad, "grad_y": yy.grad.double().numpy(),
            "out_r": [r.detach().double().numpy() for r in rs], "out_g": [g.detach().double().numpy() for g in gs],
            "after": {k: v.double().numpy() for k, v in after.items()}, "inputs": torch.cat(inputs), "diffs": diffs,
            "fmap_r": [[m.detach().double().numpy() for m in fr] for fr in frs]}


def kink_ratios(sd, y, y_hat, len_ratios=None, training=True):
    """(smallest |leaky-relu input| of the float64 run / largest |x32 - x64|, the same for r - g over the counted frames of
    every feature map): above KINK_FACTOR no kink decision differs between fp32 and float64"""
    got = {}
    for dt in (torch.float64, torch.float32):
        p = {k: torch.as_tensor(np.asarray(v)).to(dt) for k, v in sd.items()}
        inputs = []
        with torch.no_grad():
            _, _, frs, fgs, _ = forward(p, torch.as_tensor(np.asarray(y)).to(dt), torch.as_tensor(np.asarray(y_hat)).to(dt),
                                        training, None, inputs)
        diffs = []
        for fr, fg in zip(frs, fgs):
            for r, g in zip(fr, fg):
                d = (r - g).double()
                m = _mask(len_ratios, r.shape[2], d).bool()[:, None, :].expand_as(d)
                diffs.append(d[m].reshape(-1))
        got[dt] = (torch.cat(inputs), torch.cat(diffs))
    (i64, d64), (i32, d32) = got[torch.float64], got[torch.float32]
    return (float(i64.abs().min() / (i32 - i64).abs().max()), float(d64.abs().min() / (d32 - d64).abs().max()))


def fold_plain(sd):
    """the state dict with every norm folded (float64; spectral norm in EVAL mode: the vectors as they are) -> plain
    weight / bias entries"""
    p = {k: torch.as_tensor(np.asarray(v)).double() for k, v in sd.items()}
    n = 1 + max(int(k.split(".")[1]) for k in p)
    out = {}
    for i in range(n):
        sets, _ = _member_weights(p, i, False, 1)
        for name, (w, b) in zip(LAYERS, sets[0]):
            out[f"discriminators.{i}.{name}weight"], out[f"discriminators.{i}.{name}bias"] = w, b
    return out


def make_state(channels, groups, seed=0, gain=3.0):
    """a random state dict of the reference's structure at any widths: default-style init, weight_g times gain, biases
    U(-0.3, 0.3), unit power-iteration vectors"""
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    for i in range(3):
        cin = 1
        for l, name in enumerate(LAYERS):
            cout, g = (channels[l], groups[l]) if l < 7 else (1, 1)
            k = KERNELS[l]
            bound = 1.0 / np.sqrt(cin // g * k)
            w = (torch.rand(cout, cin // g, k, generator=gen) * 2 - 1) * bound
            pre = f"discriminators.{i}.{name}"
            sd[pre + "bias"] = (torch.rand(cout, generator=gen) * 2 - 1) * 0.3
            if i == 0:
                sd[pre + "weight_orig"] = w * gain
                sd[pre + "weight_u"] = _normalize(torch.randn(cout, generator=gen))
                sd[pre + "weight_v"] = _normalize(torch.randn(cin // g * k, generator=gen))
            else:
                sd[pre + "weight_g"] = w.flatten(1).norm(dim=1).reshape(-1, 1, 1) * gain
                sd[pre + "weight_v"] = w
            cin = cout
    return {k: v.numpy() for k, v in sd.items()}
