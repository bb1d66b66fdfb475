"""fp64 restatement of WaveGlow.infer with the operand rounding of its 16-bit GEMM modes (rad_mmm_amd/waveglow.py,
`precision`), for the tests of those modes.  Everything is _waveglow_ref.infer_ref, operation for operation, except the
three WN GEMM families cond_layer, in_layers and res_skip_layers, whose operands are rounded as the HIP path stores them:

    exact   no rounding: the same calls as infer_ref, so the same bits
    f16     each operand element x becomes fp16(s * x) / s; the products are summed in fp64 (the HIP path: in fp32)
    h3      each operand is the pair hi = fp16(s * x), lo = fp16(s * x - hi); the GEMM is hi.hi + hi.lo + lo.hi
            (the lo.lo term is dropped, as on the device)

s is a power of two per tensor class: W_SCALE for weights, 1 for activations.  fp16 rounding is tensor.to(torch.float16).
start, the gate, the residual stream, the skip sum, end, the coupling and the inverse mix stay exact."""
import torch
import torch.nn.functional as F

from _waveglow_ref import _w, group_cond_ref

MODES = ("exact", "f16", "h3")
W_SCALE = 256.0          # rad_mmm_amd.ops.W_SCALE (tests/test_waveglow_half_cpu.py checks that they agree)


def split_pair(x, s):
    """fp64 x -> (hi, lo) as fp64 values of the fp16 pair of s * x"""
    t = x * s
    hi = t.to(torch.float16).double()
    lo = (t - hi).to(torch.float16).double()
    return hi, lo


def conv_half(x, w, b, mode, **kw):
    """F.conv1d(x, w, b, **kw) with the operands of one of the three GEMM families rounded for `mode`"""
    if mode == "exact":
        return F.conv1d(x, w, b, **kw)
    xh, xl = split_pair(x, 1.0)
    wh, wl = split_pair(w, W_SCALE)
    y = F.conv1d(xh, wh, None, **kw)
    if mode == "h3":
        y = y + F.conv1d(xh, wl, None, **kw) + F.conv1d(xl, wh, None, **kw)
    return y / W_SCALE + b[None, :, None]


def wn_half_ref(sd, k, cfg, audio0, spect, mode):
    wn = cfg["WN_config"]
    C, L, ks = wn["n_channels"], wn["n_layers"], wn["kernel_size"]
    p = f"WN.{k}."
    b = lambda n: sd[p + n + ".bias"].double()
    audio = F.conv1d(audio0, _w(sd, p + "start"), b("start"))
    output = torch.zeros_like(audio)
    cond = conv_half(spect, _w(sd, p + "cond_layer"), b("cond_layer"), mode)
    for i in range(L):
        d = 2 ** i
        a = conv_half(audio, _w(sd, p + f"in_layers.{i}"), b(f"in_layers.{i}"), mode, dilation=d,
                      padding=(ks * d - d) // 2)
        a = a + cond[:, 2 * C * i:2 * C * (i + 1)]
        acts = torch.tanh(a[:, :C]) * torch.sigmoid(a[:, C:])
        rs = conv_half(acts, _w(sd, p + f"res_skip_layers.{i}"), b(f"res_skip_layers.{i}"), mode)
        if i < L - 1:
            audio = audio + rs[:, :C]
            output = output + rs[:, C:]
        else:
            output = output + rs
    return F.conv1d(output, sd[p + "end.weight"].double(), b("end"))


def infer_half_ref(sd, cfg, mel, sigma, noise, mode):
    """infer_ref with the GEMM operands of `mode`: mel [1, n_mel, T], noise: the draws [1, ch, Tg] -> audio [1, T*HOP]"""
    assert mode in MODES
    spect = group_cond_ref(sd, cfg, mel)
    noise = [z.double() for z in noise]
    audio = sigma * noise[0]
    zi = 1
    for k in reversed(range(cfg["n_flows"])):
        nh = audio.size(1) // 2
        a0, a1 = audio[:, :nh], audio[:, nh:]
        out = wn_half_ref(sd, k, cfg, a0, spect, mode)
        s, b = out[:, nh:], out[:, :nh]
        a1 = (a1 - b) / torch.exp(s)
        audio = torch.cat([a0, a1], 1)
        Winv = torch.linalg.inv(sd[f"convinv.{k}.conv.weight"][:, :, 0].double())
        audio = F.conv1d(audio, Winv[:, :, None])
        if k % cfg["n_early_every"] == 0 and k > 0:
            audio = torch.cat((sigma * noise[zi], audio), 1)
            zi += 1
    return audio.permute(0, 2, 1).contiguous().view(audio.size(0), -1)


def rel_l2(a, b):
    """||a - b|| / ||b|| in fp64"""
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return ((a - b).norm() / b.norm()).item()


def shipped_case():
    """the shipped-WN case of tests/test_waveglow_gpu.py: 2 flows, B = 2, T = 12, lens [12, 3], seeds 7 / 8 ->
    (cfg, sd, mel [B, 80, T], lens, noise [[B, 8, Tg]], sigma)"""
    from _waveglow_ref import HOP, SHIPPED_WN, random_state
    cfg = dict(n_mel_channels=80, n_flows=2, n_group=8, n_early_every=4, n_early_size=2, WN_config=SHIPPED_WN)
    sd = random_state(cfg, 7)
    g = torch.Generator().manual_seed(8)
    B, T, lens = 2, 12, [12, 3]
    mel = torch.randn(B, 80, T, generator=g) - 2.0
    noise = [torch.randn(B, 8, T * (HOP // 8), generator=g)]
    return cfg, sd, mel, lens, noise, 0.9


def item_refs(sd, cfg, mel, lens, noise, sigma, modes):
    """per item b, alone at its own length: {mode: audio [lens[b] * HOP] fp64}"""
    from _waveglow_ref import HOP
    per = HOP // cfg["n_group"]
    out = []
    for b, n in enumerate(lens):
        m1, z1 = mel[b:b + 1, :, :n], [z[b:b + 1, :, :n * per] for z in noise]
        out.append({mode: infer_half_ref(sd, cfg, m1, sigma, z1, mode)[0] for mode in modes})
    return out
