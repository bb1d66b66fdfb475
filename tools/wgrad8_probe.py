#!/usr/bin/env python3
"""radmmm_wgrad_rm8 (--products 2, the default) or radmmm_wgrad_rmh (--products 1: the hi planes alone) at the benchmark shapes
(12 800 frames, 1024 x 1024; 5 taps dil 2 = the in_layer conv, 1 tap = res_skip): launch time, and -- for A/B builds of the
library (RADMMM_LIB_PATH) -- a dump / bit comparison of the results.  --lstm: the context LSTM's weight-gradient shapes instead
(4192 x 1048, and 2096 x 524 with the frame shift -1 / +1, on three products and on one; lstm_shapes).  --group: a flow step's
four res_skip weight gradients with their weight-norm backward, grouped (radmmm_wgrad_rmh_group + radmmm_weightnorm_bwd_multi)
against four single launches each (group_row).
    python tools/wgrad8_probe.py [--products 1] [--dump FILE | --compare FILE] [--reps 30] [--loop N]   (--loop: launches only, for rocprofv3 --pmc)
    python tools/wgrad8_probe.py --lstm [--reps 30]
    python tools/wgrad8_probe.py --group"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def lstm_shapes(args, ops, dev, B, T, I=1048, H=524):
    """The context LSTM's three weight gradients (12 800 frames): dW_ih 4192 x 1048 and the two dW_hh 2096 x 524 read out of y
    through the frame shift -1 / +1, on three products (radmmm_wgrad_rm / _rm_shift) and on one (radmmm_wgrad_rmh_shift), with
    the split passes that feed them (y's grouped planes) -- and what the recurrent pair cost before: h_prev as a tensor (zero
    fill, two strided copies, two .contiguous(), two split passes) and two radmmm_wgrad_rm launches on it."""
    g = torch.Generator().manual_seed(1)
    R = B * T
    dG = (torch.randn(R, 8 * H, generator=g) * 3e-3).to(dev)
    x = torch.randn(R, I, generator=g).to(dev)
    y = torch.tanh(torch.randn(R, 2 * H, generator=g)).to(dev)
    SG = 2048.0
    gh, gl = ops.split_f16(dG, 8 * H, SG, 8 * H)
    xh, xl = ops.split_f16(x, I, 1.0, ops.round_up(I, 32))
    yh, yl = ops.split_f16_groups(y, H, 2)
    Hg = yh.shape[1] // 2

    def h_prev_path():
        y3 = y.view(B, T, 2 * H)
        hp = torch.zeros(B, T, 2 * H, device=dev, dtype=torch.float32)
        hp[:, 1:, :H] = y3[:, :-1, :H]
        hp[:, :-1, H:] = y3[:, 1:, H:]
        hp = hp.view(R, 2 * H)
        Hq = ops.round_up(H, 8)
        hpf = ops.split_f16(hp[:, :H].contiguous(), H, 1.0, Hq)
        hpr = ops.split_f16(hp[:, H:].contiguous(), H, 1.0, Hq)
        return (ops.wgrad_rm_slabs((gh[:, :4 * H], gl[:, :4 * H]), hpf, B, T, 4 * H, H, 1, 1, 1.0 / SG),
                ops.wgrad_rm_slabs((gh[:, 4 * H:], gl[:, 4 * H:]), hpr, B, T, 4 * H, H, 1, 1, 1.0 / SG))

    def shifted3():
        pair = ops.split_f16_groups(y, H, 2)
        return (ops.wgrad_rm_shift_slabs((gh, gl), 0, pair, 0, -1, B, T, 4 * H, H, 1.0 / SG),
                ops.wgrad_rm_shift_slabs((gh, gl), 4 * H, pair, Hg, 1, B, T, 4 * H, H, 1.0 / SG))

    def shifted1():
        hi, _ = ops.split_f16_groups(y, H, 2, with_lo=False)
        return (ops.wgrad_rmh_shift_slabs(gh, 0, hi, 0, -1, B, T, 4 * H, H, 1.0 / SG),
                ops.wgrad_rmh_shift_slabs(gh, 4 * H, hi, Hg, 1, B, T, 4 * H, H, 1.0 / SG))

    cases = [("dW_ih 4192 x 1048, three products", 8 * H * I, lambda: ops.wgrad_rm_slabs((gh, gl), (xh, xl), B, T, 8 * H, I, 1, 1, 1.0 / SG)),
             ("dW_ih 4192 x 1048, one product", 8 * H * I, lambda: ops.wgrad_rmh_shift_slabs(gh, 0, xh, 0, 0, B, T, 8 * H, I, 1.0 / SG)),
             ("dW_hh 2096 x 524, shift -1, three products", 4 * H * H, lambda: ops.wgrad_rm_shift_slabs((gh, gl), 0, (yh, yl), 0, -1, B, T, 4 * H, H, 1.0 / SG)),
             ("dW_hh 2096 x 524, shift +1, three products", 4 * H * H, lambda: ops.wgrad_rm_shift_slabs((gh, gl), 4 * H, (yh, yl), Hg, 1, B, T, 4 * H, H, 1.0 / SG)),
             ("dW_hh 2096 x 524, shift -1, one product", 4 * H * H, lambda: ops.wgrad_rmh_shift_slabs(gh, 0, yh, 0, -1, B, T, 4 * H, H, 1.0 / SG)),
             ("dW_hh 2096 x 524, shift +1, one product", 4 * H * H, lambda: ops.wgrad_rmh_shift_slabs(gh, 4 * H, yh, Hg, 1, B, T, 4 * H, H, 1.0 / SG)),
             ("both dW_hh with their operands: h_prev tensor + 2 x wgrad_rm (before)", 8 * H * H, h_prev_path),
             ("both dW_hh with their operands: grouped split of y + 2 x shifted, three products", 8 * H * H, shifted3),
             ("both dW_hh with their operands: grouped hi plane of y + 2 x shifted, one product", 8 * H * H, shifted1)]
    a, b = h_prev_path(), shifted3()
    print("shifted three-product slabs vs the h_prev path:", "bit-identical" if all(torch.equal(p, q) for p, q in zip(a, b)) else "DIFFERENT")
    for name, mn, fn in cases:
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / args.reps
        print(json.dumps({"case": name, "us": round(us, 1), "fp32_equiv_tflops": round(2.0 * R * mn / us / 1e6, 1)}), flush=True)


def group_row(ops, dev, B, T, C, SG, gh, xh, reps=50):
    """A flow step's four res/skip weight gradients (1 tap, 1024 x 1024, 12 800 rows, four operand pairs): four
    radmmm_wgrad_rmh launches + four radmmm_weightnorm_bwd against one radmmm_wgrad_rmh_group + one
    radmmm_weightnorm_bwd_multi, event-timed over 50 repetitions; the grouped slabs against single launches at the grouped
    split factor (bit for bit) and the summed gradients against the per-conv split factor."""
    g = torch.Generator().manual_seed(2)
    pairs = [(gh, xh)] + [((torch.randn(B * T, C, generator=g) * 3e-3 * SG).half().to(dev),
                           torch.nn.functional.softplus(torch.randn(B * T, C, generator=g) * 2).half().to(dev)) for _ in range(3)]
    vs = [torch.randn(C, C, 1, generator=g).to(dev) for _ in range(4)]
    gs = [torch.randn(C, 1, 1, generator=g).to(dev) for _ in range(4)]
    invs = [(1.0 / v.flatten(1).norm(dim=1)).contiguous() for v in vs]
    jobs = [(a, b, C, C) for a, b in pairs]

    def singles():
        return [ops.wgrad_rmh_slabs(a, b, B, T, C, C, 1, 1, 1.0 / SG) for a, b in pairs]

    def grouped():
        return ops.wgrad_rmh_group_slabs(jobs, B, T, 1, 1, 1.0 / SG)

    Ps, Pg = singles(), grouped()
    Sg = int(Pg[0].shape[0])
    at_sg = [ops.wgrad_rmh_group_slabs([j], B, T, 1, 1, 1.0 / SG, splits=Sg)[0] for j in jobs]
    same = all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(Pg, at_sg))
    rel = max(float((p.sum(0) - q.sum(0)).abs().max() / q.sum(0).abs().max()) for p, q in zip(Pg, Ps))
    print(f"grouped slabs vs single launches at S = {Sg}: {'bit-identical' if same else 'DIFFERENT'}; summed gradient vs S = "
          f"{int(Ps[0].shape[0])}: max rel diff {rel:.2e}")
    cases = [("4 x wgrad_rmh", singles), ("wgrad_rmh_group", grouped),
             ("4 x weightnorm_bwd", lambda: [ops.weightnorm_bwd(v, gg, inv, P, C) for v, gg, inv, P in zip(vs, gs, invs, Ps)]),
             ("weightnorm_bwd_multi", lambda: ops.weightnorm_bwd_multi(vs, gs, invs, Pg, C)),
             ("4 x (wgrad_rmh + weightnorm_bwd)", lambda: [ops.weightnorm_bwd(v, gg, inv, P, C) for v, gg, inv, P in zip(vs, gs, invs, singles())]),
             ("wgrad_rmh_group + weightnorm_bwd_multi", lambda: ops.weightnorm_bwd_multi(vs, gs, invs, grouped(), C))]
    for name, fn in cases:
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        splits = Sg if "group" in name or "multi" in name else int(Ps[0].shape[0])
        print(json.dumps({"case": name, "splits": splits, "us": round(e0.elapsed_time(e1) * 1e3 / reps, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lstm", action="store_true", help="the context LSTM's weight-gradient shapes instead of the WN convs'")
    ap.add_argument("--group", action="store_true", help="four res_skip jobs: one grouped launch against four single launches")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--dump")
    ap.add_argument("--compare")
    ap.add_argument("--loop", type=int, default=0)
    ap.add_argument("--products", type=int, choices=(1, 2), default=2)
    args = ap.parse_args()
    import rad_mmm_amd  # noqa: F401
    from rad_mmm_amd import ops
    dev = torch.device("cuda:0")
    B, T, C = 32, 400, 1024
    g = torch.Generator().manual_seed(0)
    lens = torch.tensor([T - (7 * b) % 90 for b in range(B)], dtype=torch.int32, device=dev)
    x = torch.nn.functional.softplus(torch.randn(B * T, C, generator=g) * 2).to(dev)
    gy = (torch.randn(B * T, C, generator=g) * 3e-3).to(dev)
    SG = 2048.0
    gh, gx = ops.split_f16(gy, C, SG, C, 2, ops.X8_GRAD_EXP)
    xh, xx = ops.split_f16(x, C, 1.0, C, 2, ops.X8_ACT_EXP)
    if args.lstm:
        lstm_shapes(args, ops, dev, B, T)
        return
    if args.group:
        group_row(ops, dev, B, T, C, SG, gh, xh)
        return
    cases = [("in_layer (5 taps, dil 2, masked)", 5, 2, lens), ("res_skip (1 tap)", 1, 1, None), ("5 taps, dil 1, masked", 5, 1, lens)]
    outs = {}
    for name, taps, dil, ln in cases:
        if args.products == 1:
            fn = lambda: ops.wgrad_rmh_slabs(gh, xh, B, T, C, C, taps, dil, 1.0 / SG, ln)
        else:
            fn = lambda: ops.wgrad_rm8_slabs((gh, gx), ops.X8_GRAD_EXP, (xh, xx), ops.X8_ACT_EXP, B, T, C, C, taps, dil, 1.0 / SG, ln)
        if args.loop:
            if taps == 5 and dil == 2:
                for _ in range(args.loop):
                    fn()
                torch.cuda.synchronize()
            continue
        P = fn()
        torch.cuda.synchronize()
        outs[name] = P.sum(0).cpu()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / args.reps
        print(json.dumps({"products": args.products, "case": name, "splits": int(P.shape[0]), "us": round(us, 1),
                          "fp32_equiv_tflops": round(2.0 * B * T * C * C * taps / us / 1e6, 1)}), flush=True)
    if args.dump:
        torch.save(outs, args.dump)
    if args.compare:
        ref = torch.load(args.compare)
        for k, v in outs.items():
            same = torch.equal(v.view(torch.int32), ref[k].view(torch.int32))
            d = float((v - ref[k]).abs().max() / ref[k].abs().max())
            print(f"compare {k}: {'bit-identical' if same else 'DIFFERENT'} (max rel diff {d:.2e})")


if __name__ == "__main__":
    main()
