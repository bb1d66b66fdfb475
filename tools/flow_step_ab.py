"""A/B record of the affine flow step for a refactor of its autograd nodes: run it in a checkout of the parent commit and in the
new tree and compare the two JSON files (tools/flow_step_ab.py --compare a.json b.json; profiles/flow_step_plan_ab.json#parent_1
names one run of the committed collection).

Per scenario: sha256 of every output, every gradient and (training run) the final parameters; the ordered list of C-ABI calls
that rad_mmm_amd.ops issued -- (entry point, every non-pointer argument, which pointer arguments are null), taken by recording
wrappers over ops.lib, ops.rowgemm, ops.rowgemm_h3 and ops.wgrad -- as a count and a sha256 (--dump-calls DIR writes the lists
themselves); torch.cuda.max_memory_allocated.  Only the public API and radmmm_synth are used, so the same file runs in both trees.

Scenarios: one flow step (WN width 64, B = 2, ragged) per path of AffineFlowStepH3Fn / AffineFlowStepFn and per switch, a
two-flow decoder (the context-gradient accumulator) and the six-step 12 x 800 training run of tests/test_hip_round5.py.
"""
import argparse
import ctypes as C
import gc
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = torch.device("cuda:0")
SWITCHES = ("RADMMM_WGRAD_PRODUCTS", "RADMMM_RES_SRC", "RADMMM_DACT_MULTI", "RADMMM_WGRAD_GROUP", "RADMMM_RES_STREAM")
QUERIES = {"radmmm_last_error", "radmmm_gemm_cu_slots", "radmmm_abi_version", "radmmm_rowgemm_h3_colsum_rows"}
QUERY_SUFFIXES = ("_tiles", "_scratch_floats", "_plan", "_last_kernel")

# name: (precision, T, n_layers, frozen parameters, environment)
STEPS = {
    "f8x_one_product": ("f8x", 40, 4, False, {}),
    "f8x_two_products": ("f8x", 40, 4, False, {"RADMMM_WGRAD_PRODUCTS": "2"}),
    "f8x_T64": ("f8x", 64, 4, False, {}),
    "h3_pairs": ("h3", 40, 4, False, {}),
    "h3_pairs_T64": ("h3", 64, 4, False, {}),
    "f16_transposed": ("f16", 40, 4, False, {}),
    "h3_T24_transposed": ("h3", 24, 4, False, {}),
    "f8x_T24_transposed": ("f8x", 24, 4, False, {}),
    "f16_wide_taps_fp32_fallback": ("f16", 40, 5, False, {}),
    "h3_T24_wide_taps_fp32_fallback": ("h3", 24, 5, False, {}),
    "f8x_one_layer": ("f8x", 40, 1, False, {}),
    "f8x_five_layers": ("f8x", 40, 5, False, {}),
    "h3_one_layer": ("h3", 40, 1, False, {}),
    "h3_five_layers": ("h3", 40, 5, False, {}),
    "f16_one_layer": ("f16", 40, 1, False, {}),
    "f8x_frozen": ("f8x", 40, 4, True, {}),
    "h3_frozen": ("h3", 40, 4, True, {}),
    "f16_frozen": ("f16", 40, 4, True, {}),
    "f8x_res_src_0": ("f8x", 40, 4, False, {"RADMMM_RES_SRC": "0"}),
    "h3_res_src_0": ("h3", 40, 4, False, {"RADMMM_RES_SRC": "0"}),
    "f8x_dact_multi_0": ("f8x", 40, 4, False, {"RADMMM_DACT_MULTI": "0"}),
    "h3_dact_multi_0": ("h3", 40, 4, False, {"RADMMM_DACT_MULTI": "0"}),
    "f8x_wgrad_group_0": ("f8x", 40, 4, False, {"RADMMM_WGRAD_GROUP": "0"}),
    "f8x_res_stream_1": ("f8x", 40, 4, False, {"RADMMM_RES_STREAM": "1"}),
    "fp32": ("fp32", 40, 4, False, {}),
    "fp32_frozen": ("fp32", 40, 4, True, {}),
}
KW = dict(n_speaker_dim=16, use_accent_emb_for_decoder=True, n_accent_dim=8, n_text_dim=512, n_f0_dims=1,
          n_energy_avg_dims=1, n_mel_channels=80, n_early_size=2, n_early_every=2, n_group_size=2,
          scaling_fn="tanh", affine_activation="softplus", use_partial_padding=True, n_conv_layers_per_step=4, n_flows=2)


def digest(t) -> str:
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


# ---------------------------------------------------------------------------------------------------------------------
# recording wrappers
# ---------------------------------------------------------------------------------------------------------------------
def _enc_struct(s):
    out = []
    for name, typ in s._fields_:
        v = getattr(s, name)
        if typ is C.c_void_p:
            out.append((name, "ptr" if v else "null"))
        elif isinstance(v, C.Structure):
            out.append((name, _enc_struct(v)))
        elif isinstance(v, C.Array):
            out.append((name, ["ptr" if e else "null" for e in v]))
        else:
            out.append((name, v))
    return out


def _enc_arg(a, typ):
    if typ is C.c_void_p:
        return "ptr" if a else "null"
    if a is None:
        return "null"
    if isinstance(a, C.Array):
        return [_enc_struct(e) for e in a]
    if hasattr(a, "_obj"):                                   # ctypes.byref(struct)
        return _enc_struct(a._obj)
    return a


class LibRecorder:
    """ops.lib with every launching entry point recorded (queries -- tile counts, scratch sizes, plans -- pass through)"""

    def __init__(self, lib, calls):
        self.__dict__["_lib"], self.__dict__["_calls"] = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("radmmm_") or name in QUERIES or name.endswith(QUERY_SUFFIXES):
            return fn
        types = fn.argtypes

        def call(*args):
            assert types is not None and len(types) == len(args), name
            self._calls.append((name, [_enc_arg(a, t) for a, t in zip(args, types)]))
            return fn(*args)
        return call


def _record_kw(name, fn, calls):
    def call(**kw):
        enc = []
        for k, v in kw.items():
            if isinstance(v, torch.Tensor):
                v = "ptr"
            elif v is None:
                v = "null"
            elif isinstance(v, (list, tuple)):
                v = ["ptr" if t is not None else "null" for t in v]
            enc.append((k, v))
        calls.append((name, enc, "stream" if torch.cuda.current_stream().cuda_stream else "stream0"))
        return fn(**kw)
    return call


def install(calls):
    from rad_mmm_amd import ops
    ops.lib = LibRecorder(ops.lib, calls)
    for name in ("rowgemm", "rowgemm_h3", "wgrad"):
        setattr(ops, name, _record_kw(name, getattr(ops, name), calls))


# ---------------------------------------------------------------------------------------------------------------------
# scenarios
# ---------------------------------------------------------------------------------------------------------------------
def flow_step(precision, T, n_layers, frozen):
    """one AffineTransformationLayer.run: WN width 64, 8 flow channels, 12 context channels, B = 2, ragged lengths"""
    from rad_mmm_amd.common import AffineTransformationLayer
    from rad_mmm_amd.ops import ZLD
    B, Cz, D, Wc = 2, 8, 12, 64
    g = torch.Generator().manual_seed(1000 * T + 10 * n_layers + len(precision))
    layer = AffineTransformationLayer(Cz, D, n_layers, affine_model="wavenet", scaling_fn="tanh", affine_activation="softplus",
                                      n_channels=Wc, use_partial_padding=True)
    with torch.no_grad():
        for n, p in layer.named_parameters():
            p.copy_(torch.rand(p.shape, generator=g) + 0.5 if n.endswith("weight_g") else torch.randn(p.shape, generator=g) * 0.1)
    layer = layer.to(DEV)
    for p in layer.parameters():
        p.requires_grad_(not frozen)
    z = torch.zeros(B * T, ZLD)
    z[:, :Cz] = torch.randn(B * T, Cz, generator=g)
    z = z.to(DEV).requires_grad_(True)
    cond = torch.randn(B * T, D, generator=g).to(DEV).requires_grad_(True)
    W = torch.eye(ZLD)
    W[:Cz, :Cz] += 0.1 * torch.randn(Cz, Cz, generator=g)
    W = W.to(DEV).requires_grad_(True)
    b_eff = torch.zeros(ZLD, device=DEV)
    lens = torch.tensor([T, T - 14], dtype=torch.int32, device=DEV)
    gz = torch.zeros(B * T, ZLD)
    gz[:, :Cz] = torch.randn(B * T, Cz, generator=g)
    gl = torch.randn(B * T, Cz // 2, generator=g)
    zo, log_s = layer.run(z, cond, lens, W, b_eff, B, T, precision, {})
    ((zo * gz.to(DEV)).sum() + (log_s * gl.to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    out = {"z_out": digest(zo), "log_s": digest(log_s), "grad.z": digest(z.grad), "grad.cond": digest(cond.grad),
           "grad.W_eff": digest(W.grad)}
    for n, p in layer.named_parameters():
        assert (p.grad is None) == frozen, n
        if p.grad is not None:
            out["grad." + n] = digest(p.grad)
    return out


def _T(d):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()}


def decoder_two_affine_steps(precision):
    """two-flow decoder, forward + NLL + backward: the affine steps share one context-gradient buffer"""
    import radmmm_synth as S
    from rad_mmm_amd.common import SequenceLength
    from rad_mmm_amd.decoders import RADMMMFlow
    from rad_mmm_amd.loss import RADMMMLoss
    kw = dict(KW, n_text_dim=64)
    cfg = S.DecoderConfig(**kw)
    dec = RADMMMFlow(use_accent=True, **kw)
    dec.load_state_dict(_T(S.procedural_decoder_state(S.decoder_state_shapes(cfg))))
    dec.gemm_precision = precision
    dec = dec.to(DEV).train()
    b = {k: v.to(DEV) for k, v in _T(S.synthetic_batch(2, 80, cfg, 7, ragged=True)).items()}
    ctx = b["context"].clone().requires_grad_(True)
    sl = SequenceLength(b["lengths"])
    out = dec(b["mel"], b["spk"], ctx, sl, b["f0"], b["energy"], b["accent"])
    loss = RADMMMLoss(sigma=1.0, n_group_size=2)(out, None, sl, 0)["loss_mel"][0]
    loss.backward()
    torch.cuda.synchronize()
    res = {"z_mel": digest(out["z_mel"]), "loss": digest(loss), "grad.context": digest(ctx.grad)}
    res.update({"grad." + n: digest(p.grad) for n, p in dec.named_parameters() if p.grad is not None})
    return res


def training_run(steps=6):
    """the run of tests/test_hip_round5.py::test_training_run_is_bitwise_repeatable (free-running host)"""
    import radmmm_synth as S
    from rad_mmm_amd.common import SequenceLength
    from rad_mmm_amd.ddp import BucketedGradReducer
    from rad_mmm_amd.decoders import RADMMMFlow
    from rad_mmm_amd.loss import RADMMMLoss
    from rad_mmm_amd.optim import FlatRAdam
    cfg = S.DecoderConfig(**KW)
    dec = RADMMMFlow(use_accent=True, **KW)
    dec.load_state_dict(_T(S.procedural_decoder_state(S.decoder_state_shapes(cfg))))
    dec = dec.to(DEV).train()
    red = BucketedGradReducer(dec)
    opt = FlatRAdam(dec.named_parameters(), lr=2e-4, weight_decay=1e-6, reducer=red)
    crit = RADMMMLoss(sigma=1.0, n_group_size=2)
    res = {}
    for k in range(steps):
        b = {kk: vv.to(DEV) for kk, vv in _T(S.synthetic_batch(12, 800, cfg, 500 + k, ragged=True)).items()}
        if k >= 2:
            b["mel"] = (b["mel"] - 2.5) * 3.0 + 2.5
        sl = SequenceLength(b["lengths"])
        red.prepare()
        out = dec(b["mel"], b["spk"], b["context"], sl, b["f0"], b["energy"], b["accent"])
        loss = crit(out, None, sl, 0)["loss_mel"][0]
        loss.backward()
        red.finish()
        res[f"step{k}.z_mel"], res[f"step{k}.loss"] = digest(out["z_mel"]), digest(loss)
        for n, p in dec.named_parameters():
            if p.grad is not None:
                res[f"step{k}.grad.{n}"] = digest(p.grad)
        opt.clip_grad_norm(1.0)
        opt.step()
    torch.cuda.synchronize()
    res.update({"param." + n: digest(p) for n, p in dec.named_parameters()})
    return res


def run_scenario(name, fn, env, calls, dump_dir):
    for k in SWITCHES + ("RADMMM_PRECISION", "RADMMM_CHECK_SATURATION"):
        os.environ.pop(k, None)
    os.environ.update(RADMMM_DEBUG="1", RADMMM_F8X_MIN_ROWS="0", **env)
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    del calls[:]
    digests = fn()
    text = json.dumps(calls)
    if dump_dir:
        os.makedirs(dump_dir, exist_ok=True)
        with open(os.path.join(dump_dir, name + ".txt"), "w") as f:
            f.write("\n".join(json.dumps(c) for c in calls) + "\n")
    return {"digests": digests, "digest_of_digests": hashlib.sha256(json.dumps(digests, sort_keys=True).encode()).hexdigest(),
            "calls": len(calls), "calls_sha256": hashlib.sha256(text.encode()).hexdigest(),
            "max_memory_allocated": int(torch.cuda.max_memory_allocated())}


def _load(path):
    """the scenarios of a record of this tool, or of run R of a collection of them (profiles/flow_step_plan_ab.json) as PATH#R"""
    path, _, run = path.partition("#")
    d = json.load(open(path))
    return d["runs"][run] if run else d["scenarios"]


def compare(a_path, b_path) -> int:
    a, b = _load(a_path), _load(b_path)
    bad = 0
    for name in sorted(set(a) | set(b)):
        ra, rb = a.get(name), b.get(name)
        if ra is None or rb is None:
            print(f"{name}: only in {'first' if rb is None else 'second'}")
            bad += 1
            continue
        da, db = ra.get("digests") or {}, rb.get("digests") or {}       # (a collection keeps digest_of_digests only)
        diff = sorted(k for k in set(da) | set(db) if da.get(k) != db.get(k)) or (
            ["digest_of_digests"] if ra["digest_of_digests"] != rb["digest_of_digests"] else [])
        same_calls = ra["calls_sha256"] == rb["calls_sha256"]
        mem = rb["max_memory_allocated"] - ra["max_memory_allocated"]
        print(f"{name}: digests {'equal' if not diff else 'DIFFER ' + str(diff[:4])}, calls {ra['calls']} / {rb['calls']} "
              f"{'equal' if same_calls else 'DIFFER'}, peak memory {ra['max_memory_allocated']} / {rb['max_memory_allocated']} ({mem:+d})")
        bad += bool(diff) + (not same_calls)
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="flow_step_ab.json")
    ap.add_argument("--dump-calls", default=None, metavar="DIR")
    ap.add_argument("--only", default=None, help="comma-separated scenario names")
    ap.add_argument("--no-training-run", action="store_true")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    calls = []
    install(calls)
    todo = {name: ((lambda s=spec: flow_step(*s[:4])), spec[4]) for name, spec in STEPS.items()}
    for prec in ("f8x", "h3", "f16"):
        todo["decoder_two_affine_steps_" + prec] = ((lambda p=prec: decoder_two_affine_steps(p)), {})
    if not args.no_training_run:
        todo["training_run_12x800"] = (training_run, {"RADMMM_PRECISION": "f8x"})
    only = set(args.only.split(",")) if args.only else None
    res = {}
    for name, (fn, env) in todo.items():
        if only is None or name in only:
            res[name] = run_scenario(name, fn, env, calls, args.dump_calls)
            print(name, res[name]["calls"], res[name]["calls_sha256"][:12], res[name]["digest_of_digests"][:12],
                  res[name]["max_memory_allocated"], flush=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "scenarios": res}, f, indent=1)


if __name__ == "__main__":
    main()
