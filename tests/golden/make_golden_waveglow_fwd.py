#!/usr/bin/env python3
"""Generate tests/golden/waveglow_fwd_tiny.npz by RUNNING THE REFERENCE's WaveGlow.forward and WaveGlowLoss
(vocoders/waveglow_for_LIMMITS23/glow.py:43-59, 207-249) on the CPU:

    python tests/golden/make_golden_waveglow_fwd.py --ref <checkout of the reference>

It follows make_golden_waveglow.py: the TINY configuration, each WN.end re-initialised with N(0, 0.05) weights and
biases, every weight rounded to a float16 value before it is loaded and stored as float16, exactly.  The reference
initialises each convinv orthonormal, so every log-determinant would be 0 and a wrong log-det term would pass: each W is
multiplied by a random positive diagonal in [0.5, 1.5] and 0.05 * N(0, 1) is added before the rounding; the generator
asserts det > 0 (the reference's torch.logdet is NaN below 0) and |logdet| > 0.05 for every flow.

The fixture holds the config, the weight-normed state_dict, mel, lens and audio (noise plus a sine, |x| < 1, zero past
each length); per item, run alone at its own length: z, the per-flow sums of log_s, the per-flow log-determinant of one
group step and the reference's loss; one equal-length batch of two (the first `eq_T` frames of both items) with the
reference's batch loss; the reference's own float32-against-float64 deviation of z and of the loss; and roundtrip_f32,
the max-abs error of the reference's float32 infer fed the z of its own float32 forward.

One thread and a zip archive with fixed time stamps: two runs write the same bytes.
"""
import argparse
import copy
import json
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

TINY = dict(n_mel_channels=8, n_flows=6, n_group=8, n_early_every=2, n_early_size=2,
            WN_config=dict(n_layers=4, n_channels=32, kernel_size=3))
HOP = 256


class Replay:
    """stand-in for torch.cuda.FloatTensor in the reference's infer: FloatTensor(*shape).normal_() hands back the next
    prepared draw (the pieces of z)"""
    draws = []

    def __init__(self, *shape):
        self.shape = tuple(shape)

    def normal_(self):
        z = Replay.draws.pop(0)
        assert tuple(z.shape) == self.shape, (tuple(z.shape), self.shape)
        return z


def save(name, **arrs):
    """np.savez_compressed with fixed member time stamps, in the order given"""
    path = os.path.join(HERE, name)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key, val in arrs.items():
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with zf.open(info, "w", force_zip64=True) as fh:
                np.lib.format.write_array(fh, np.asanyarray(val), allow_pickle=False)
    print(f"wrote {name}: {os.path.getsize(path) / 1024:.1f} KiB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project")
    args = ap.parse_args()
    from make_golden import install_stubs
    install_stubs()
    wg_dir = os.path.join(args.ref, "vocoders", "waveglow_for_LIMMITS23")
    sys.path[:0] = [wg_dir, os.path.join(wg_dir, "tacotron2")]
    os.chdir("/tmp")
    import torch
    torch.set_num_threads(1)
    torch.cuda.FloatTensor = Replay
    from glow import WaveGlow, WaveGlowLoss
    torch.set_grad_enabled(False)

    torch.manual_seed(51)
    m = WaveGlow(**json.loads(json.dumps(TINY)))
    g = torch.Generator().manual_seed(52)
    for wn in m.WN:
        wn.end.weight.data = 0.05 * torch.randn(wn.end.weight.shape, generator=g)
        wn.end.bias.data = 0.05 * torch.randn(wn.end.bias.shape, generator=g)
    for inv in m.convinv:
        W = inv.conv.weight.data[:, :, 0]
        c = W.shape[0]
        d = 0.5 + torch.rand(c, generator=g)
        inv.conv.weight.data = (W * d[None, :] + 0.05 * torch.randn(c, c, generator=g))[:, :, None].contiguous()
    for p in m.parameters():
        p.data = p.data.half().float()
    for k, inv in enumerate(m.convinv):
        W = inv.conv.weight.data[:, :, 0].double()
        det = torch.det(W).item()
        assert det > 0 and abs(np.log(det)) > 0.05, (k, det)
        print(f"convinv.{k}: det {det:.4f}, logdet {np.log(det):+.4f}")
    sd = {k: v.clone() for k, v in m.state_dict().items()}              # weight-normed keys
    m64 = copy.deepcopy(m).double()                                     # weight norm folded in float64 below
    m, m64 = WaveGlow.remove_weightnorm(m).eval(), WaveGlow.remove_weightnorm(m64).eval()
    crit = WaveGlowLoss(sigma=1.0)

    lens, n_flows, ng = [7, 4], TINY["n_flows"], TINY["n_group"]
    T = max(lens)
    per = HOP // ng
    Tg = T * per
    g = torch.Generator().manual_seed(53)
    mel = torch.randn(len(lens), 8, T, generator=g) - 2.0
    audio = torch.zeros(len(lens), T * HOP)
    for b, n in enumerate(lens):
        t = torch.arange(n * HOP)
        audio[b, :n * HOP] = 0.1 * torch.randn(n * HOP, generator=g).clamp(-3, 3) + 0.5 * torch.sin(t * (0.05 + 0.02 * b))
    assert audio.abs().max() < 1

    def detached(out):
        z, log_s_list, log_det_W_list = out
        return z, log_s_list, [x.clone() for x in log_det_W_list]       # WaveGlowLoss adds into the first entry

    z_all = np.zeros((len(lens), ng, Tg), np.float32)
    log_s_sums = np.zeros((len(lens), n_flows), np.float64)
    logdet = np.zeros((len(lens), n_flows), np.float64)
    loss_item = np.zeros(len(lens), np.float64)
    dz = dl = rt = 0.0
    for b, n in enumerate(lens):
        mb, ab = mel[b:b + 1, :, :n], audio[b:b + 1, :n * HOP]
        z, ls_list, ld_list = detached(m((mb, ab)))
        z64, ls64, ld64 = detached(m64((mb.double(), ab.double())))
        loss = crit((z, ls_list, [x.clone() for x in ld_list])).item()
        loss64 = crit((z64, ls64, ld64)).item()
        dz = max(dz, (z.double() - z64).abs().max().item())
        dl = max(dl, abs(loss - loss64))
        z_all[b, :, :n * per] = z[0].numpy()
        log_s_sums[b] = [x.double().sum().item() for x in ls_list]
        logdet[b] = [x.item() / (n * per) for x in ld_list]
        loss_item[b] = loss
        # the reference's own inverse on its own z: the last channels first, then the early blocks, latest exit first
        lo = ng - m.n_remaining_channels
        Replay.draws = [z[:, lo:].clone()]
        while lo > 0:
            Replay.draws.append(z[:, lo - TINY["n_early_size"]:lo].clone())
            lo -= TINY["n_early_size"]
        back = m.infer(mb, sigma=1.0)
        assert not Replay.draws
        rt = max(rt, (back - ab).abs().max().item())
    assert np.abs(logdet[0] - logdet[1]).max() < 1e-6
    eq_T = min(lens)
    eq = (mel[:, :, :eq_T], audio[:, :eq_T * HOP])
    eq_loss = crit(detached(m(eq))).item()
    eq_loss64 = crit(detached(m64((eq[0].double(), eq[1].double())))).item()
    dl = max(dl, abs(eq_loss - eq_loss64))
    print(f"waveglow_fwd_tiny: float32 vs float64 z {dz:.3e} (|z| max {np.abs(z_all).max():.3f}), loss {dl:.3e} "
          f"(losses {loss_item.tolist()}, batch {eq_loss:.6f}); float32 round trip {rt:.3e}")
    arrs = {}
    for k, v in sd.items():
        h = v.numpy().astype(np.float16)
        assert np.array_equal(h.astype(np.float32), v.numpy()), k
        arrs["sd/" + k] = h
    save("waveglow_fwd_tiny.npz", config=np.array(json.dumps(TINY)), mel=mel.numpy(), lens=np.array(lens),
         audio=audio.numpy(), z=z_all, log_s_sums=log_s_sums, logdet=logdet[0], loss_item=loss_item,
         eq_T=np.array(eq_T), eq_loss=np.array(eq_loss), f32_vs_f64_z=np.array(dz), f32_vs_f64_loss=np.array(dl),
         roundtrip_f32=np.array(rt), **arrs)


if __name__ == "__main__":
    main()
