"""ops.flow_plan: the host-only plan of an AffineFlowStepH3Fn node, held to a table of decisions.

The table (`expected` below) is derived from the lines of the node the plan replaced -- AffineFlowStepH3Fn.forward / .backward
of the commit before the plan, quoted here with the names they had there (NPR = nprod, nl = n_layers):

  forward   use_rm    = bool(NPR in (2, 3) and T >= 32 and B <= 1024 and any(ctx.needs_input_grad))
  forward   pair_only = use_rm and NPR == 2
  forward   res_src   = bool(2 <= nl <= 4 and debug_env("RADMMM_RES_SRC", "1") != "0")
  forward   OUT       = None if (res_src and use_rm) else _empty(N, Wc, like=z_in)           -> out_f32
  forward   pair_res  = bool(res_src and NPR == 2 and nl >= 2 and z_in.is_cuda and debug_env("RADMMM_RES_STREAM", "0") == "1")
  forward   ctx.plan  = FlowPlan(use_rm, pair_only, wgrad_products_env() if pair_only else NPR, layout)
  backward  multi     = bool(use_rm and 2 <= nl <= 4 and act and debug_env("RADMMM_DACT_MULTI", "1") != "0")
  backward  grouped   = bool(multi and pair_only and plan.wgrad_products == 1 and debug_env("RADMMM_WGRAD_GROUP", "1") != "0")
  backward  `if use_rm: ... wg_rm(...)  else: ... transpose_split_act / wgrad_h3_slabs / wgrad_slabs`   -> wgrad strategy
  backward  `if use_rm and T % 16 != 0:` (the channel mix's weight gradient from split pairs)           -> mix_split

debug_env honours a switch only under RADMMM_DEBUG=1; RADMMM_WGRAD_PRODUCTS is read with os.environ directly, takes "1" or "2"
and is read only where pair_only holds.  The one intended difference from those lines: RADMMM_DACT_MULTI and RADMMM_WGRAD_GROUP
are read when the plan is made (forward), like the others.
"""
import itertools
import sys

import pytest

SWITCHES = {"RADMMM_WGRAD_PRODUCTS": ("1", "2"), "RADMMM_RES_SRC": ("1", "0"), "RADMMM_DACT_MULTI": ("1", "0"),
            "RADMMM_WGRAD_GROUP": ("1", "0"), "RADMMM_RES_STREAM": ("0", "1")}
SHAPES = list(itertools.product((1, 2, 3), (24, 32, 40), (2, 1025), (1, 2, 4, 5), (0, 1), (False, True)))


def expected(nprod, B, T, nl, act, needs_grad, is_cuda, env, debug=True):
    sw = lambda name, default: env.get(name, default) if debug else default
    use_rm = nprod in (2, 3) and T >= 32 and B <= 1024 and needs_grad
    pair_only = use_rm and nprod == 2
    products = int(env.get("RADMMM_WGRAD_PRODUCTS", "1")) if pair_only else nprod
    res_src = 2 <= nl <= 4 and sw("RADMMM_RES_SRC", "1") != "0"
    multi = use_rm and 2 <= nl <= 4 and bool(act) and sw("RADMMM_DACT_MULTI", "1") != "0"
    return dict(use_rm=use_rm, pair_only=pair_only, wgrad_products=products, res_src=res_src, out_f32=not (res_src and use_rm),
                pair_res=res_src and nprod == 2 and nl >= 2 and is_cuda and sw("RADMMM_RES_STREAM", "0") == "1",
                multi=multi, grouped=multi and pair_only and products == 1 and sw("RADMMM_WGRAD_GROUP", "1") != "0",
                wgrad="pairs" if use_rm else "transposed", mix_split=use_rm and T % 16 != 0)


def _set(monkeypatch, env, debug="1"):
    monkeypatch.setenv("RADMMM_DEBUG", debug)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("values", list(itertools.product(*SWITCHES.values())), ids="".join)
def test_plan_follows_the_table_under_every_switch_setting(values, monkeypatch):
    from rad_mmm_amd.ops import flow_plan
    env = dict(zip(SWITCHES, values))
    _set(monkeypatch, env)
    for nprod, T, B, nl, act, needs_grad in SHAPES:
        for is_cuda in (True, False):
            plan = flow_plan(nprod, B, T, nl, act, needs_grad, is_cuda)
            assert plan._asdict() == expected(nprod, B, T, nl, act, needs_grad, is_cuda, env), (nprod, B, T, nl, act, needs_grad)
            assert all(type(v) in (bool, int, str) for v in plan)


def test_defaults_and_the_benchmark_shape(monkeypatch):
    from rad_mmm_amd.ops import FlowPlan, flow_plan
    _set(monkeypatch, {})
    for nprod, T, B, nl, act, needs_grad in SHAPES:
        assert flow_plan(nprod, B, T, nl, act, needs_grad)._asdict() == expected(nprod, B, T, nl, act, needs_grad, True, {})
    # f8x, four WN layers, softplus: pair-only on one product, skip sum formed once, no fp32 OUT, one gQ pass, grouped
    assert flow_plan(2, 32, 400, 4, 1, True) == FlowPlan(True, True, 1, True, False, False, True, True, "pairs", False)
    assert flow_plan(3, 32, 400, 4, 1, True) == FlowPlan(True, False, 3, True, False, False, True, False, "pairs", False)
    assert flow_plan(1, 32, 400, 4, 1, True) == FlowPlan(False, False, 1, True, True, False, False, False, "transposed", False)
    assert flow_plan(2, 2, 1000, 8, 1, True) == FlowPlan(True, True, 1, False, True, False, False, False, "pairs", True)


def test_rows_written_by_hand(monkeypatch):
    """(use_rm, pair_only, wgrad_products, res_src, out_f32, pair_res, multi, grouped, wgrad, mix_split) worked out from the rules,
    not computed: each row moves one input or one switch away from f8x / B 2 / T 40 / four layers / softplus / gradients needed"""
    from rad_mmm_amd.ops import FlowPlan, flow_plan
    rows = [
        ({}, (2, 2, 40, 4, 1, True), (True, True, 1, True, False, False, True, True, "pairs", True)),
        ({}, (2, 2, 24, 4, 1, True), (False, False, 2, True, True, False, False, False, "transposed", False)),      # T < 32
        ({}, (2, 1025, 40, 4, 1, True), (False, False, 2, True, True, False, False, False, "transposed", False)),   # B > 1024
        ({}, (2, 2, 40, 1, 1, True), (True, True, 1, False, True, False, False, False, "pairs", True)),             # one layer
        ({}, (2, 2, 40, 5, 1, True), (True, True, 1, False, True, False, False, False, "pairs", True)),             # five layers
        ({}, (2, 2, 40, 4, 0, True), (True, True, 1, True, False, False, False, False, "pairs", True)),             # no activation
        ({}, (2, 2, 40, 4, 1, False), (False, False, 2, True, True, False, False, False, "transposed", False)),     # no gradient
        ({}, (3, 2, 32, 4, 1, True), (True, False, 3, True, False, False, True, False, "pairs", False)),            # h3, T % 16 == 0
        ({}, (1, 2, 40, 4, 1, True), (False, False, 1, True, True, False, False, False, "transposed", False)),      # f16
        ({"RADMMM_WGRAD_PRODUCTS": "2"}, (2, 2, 40, 4, 1, True), (True, True, 2, True, False, False, True, False, "pairs", True)),
        ({"RADMMM_RES_SRC": "0"}, (2, 2, 40, 4, 1, True), (True, True, 1, False, True, False, True, True, "pairs", True)),
        ({"RADMMM_DACT_MULTI": "0"}, (2, 2, 40, 4, 1, True), (True, True, 1, True, False, False, False, False, "pairs", True)),
        ({"RADMMM_WGRAD_GROUP": "0"}, (2, 2, 40, 4, 1, True), (True, True, 1, True, False, False, True, False, "pairs", True)),
        ({"RADMMM_RES_STREAM": "1"}, (2, 2, 40, 4, 1, True), (True, True, 1, True, False, True, True, True, "pairs", True)),
        ({"RADMMM_RES_STREAM": "1"}, (3, 2, 40, 4, 1, True), (True, False, 3, True, False, False, True, False, "pairs", True)),   # f8x only
        ({"RADMMM_RES_STREAM": "1", "RADMMM_RES_SRC": "0"}, (2, 2, 40, 4, 1, True), (True, True, 1, False, True, False, True, True, "pairs", True)),
    ]
    for env, args, want in rows:
        _set(monkeypatch, env)
        assert flow_plan(*args) == FlowPlan(*want), (env, args)
    _set(monkeypatch, {"RADMMM_RES_STREAM": "1"})
    assert not flow_plan(2, 2, 40, 4, 1, True, is_cuda=False).pair_res


def test_debug_switches_need_radmmm_debug(monkeypatch):
    """without RADMMM_DEBUG=1 the four A/B switches are ignored; RADMMM_WGRAD_PRODUCTS (a supported switch) is not"""
    from rad_mmm_amd.ops import flow_plan
    env = {"RADMMM_WGRAD_PRODUCTS": "2", "RADMMM_RES_SRC": "0", "RADMMM_DACT_MULTI": "0", "RADMMM_WGRAD_GROUP": "0",
           "RADMMM_RES_STREAM": "1"}
    _set(monkeypatch, env, debug="0")
    for nprod, T, B, nl, act, needs_grad in SHAPES:
        assert flow_plan(nprod, B, T, nl, act, needs_grad)._asdict() == expected(nprod, B, T, nl, act, needs_grad, True, env, debug=False)


def test_wgrad_products_is_validated_only_where_it_is_read(monkeypatch):
    from rad_mmm_amd.ops import flow_plan
    _set(monkeypatch, {"RADMMM_WGRAD_PRODUCTS": "3"})
    with pytest.raises(ValueError):
        flow_plan(2, 2, 40, 4, 1, True)
    assert flow_plan(3, 2, 40, 4, 1, True).wgrad_products == 3
    assert flow_plan(2, 2, 24, 4, 1, True).wgrad_products == 2          # not pair-only (T < 32): the product scheme itself


def test_the_plan_call_needs_no_gpu(monkeypatch):
    import torch
    from rad_mmm_amd.ops import flow_plan
    _set(monkeypatch, {})
    was_initialised = torch.cuda.is_initialized()
    before = set(sys.modules)
    calls = []
    monkeypatch.setattr(torch.cuda, "_lazy_init", lambda *a, **k: calls.append("cuda"))
    for nprod, T, B, nl, act, needs_grad in SHAPES:
        flow_plan(nprod, B, T, nl, act, needs_grad)
    assert not calls and torch.cuda.is_initialized() == was_initialised
    assert set(sys.modules) == before                                    # nothing imported by the call
