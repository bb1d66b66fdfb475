"""CPU checks of the fused Adam / AdamW step (rad_mmm_amd/csrc/optim.hip radmmm_adam_step, rad_mmm_amd.optim.FlatAdam):
the float64 restatement tests/_adam_ref.py is held to torch.optim.Adam and torch.optim.AdamW, the bar of the GPU tests
rejects planted wrong variants, and the entry points refuse bad arguments before any HIP call."""
import numpy as np
import pytest
import torch

import _adam_ref as R
from rad_mmm_amd.optim import FlatAdam

STEPS = 5


def _problem(seed, n=257):
    g = np.random.default_rng(seed)
    p0 = g.standard_normal(n)
    grads = [g.standard_normal(n) * 10.0 ** g.uniform(-3, 1, n) for _ in range(STEPS)]
    return p0, grads


@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.8, 0.99)])
def test_restatement_matches_torch_in_float64(decoupled, weight_decay, betas):
    p0, grads = _problem(3)
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([p], lr=1e-3, betas=betas, eps=1e-8, weight_decay=weight_decay)
    want = []
    for g in grads:
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        want.append(p.detach().numpy().copy())
    got, m, v, t = R.run(p0, grads, lr=1e-3, betas=betas, eps=1e-8, weight_decay=weight_decay, decoupled=decoupled)
    assert t == STEPS
    for k in range(STEPS):
        assert np.abs(got[k] - want[k]).max() <= 1e-12, k
    st = opt.state[p]
    assert np.abs(m - st["exp_avg"].numpy()).max() <= 1e-12 and np.abs(v - st["exp_avg_sq"].numpy()).max() <= 1e-12


@pytest.mark.parametrize("flaw,kw", [
    ("decay_swapped", dict(weight_decay=0.01, decoupled=True)),
    ("decay_swapped", dict(weight_decay=0.01, decoupled=False)),
    ("eps_in_sqrt", dict(eps=1e-8)),
    ("bias_t_minus_1", dict()),
])
def test_bar_rejects_planted_variants(flaw, kw):
    """the GPU tests' bar (tests/test_hip_adam_direct.py) against the float64 restatement separates each planted variant
    from the right rule, over the 5 steps and after a single one where the variant differs there.  The problem is that of
    the GPU tests: parameters of order 1, lr 1e-2, gradients over four decades with a few tiny ones (where eps matters)."""
    p0, grads = _problem(5)
    grads[0][:8] = 1e-9                                       # sqrt(v) ~ eps: eps inside the root is visible here
    for g in grads[1:]:
        g[:8] *= 1e-9
    base = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8)
    base.update(kw)
    want, *_ = R.run(p0, grads, **base)
    bad, *_ = R.run(p0, grads, flaw=flaw, **base)
    assert R.within_bar(want[-1], want[-1], STEPS)
    assert not R.within_bar(bad[-1], want[-1], STEPS), R.worst_over_bar(bad[-1], want[-1], STEPS)
    assert R.worst_over_bar(bad[-1], want[-1], STEPS) > 10.0


def test_bar_rejects_a_counter_that_advances_on_a_skipped_step():
    p0, grads = _problem(7)
    skip = [False, True, False, False, False]
    kw = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, skip=skip)
    want, _, _, t = R.run(p0, grads, **kw)
    bad, _, _, tb = R.run(p0, grads, flaw="count_skipped", **kw)
    assert (t, tb) == (4, 5)
    assert np.array_equal(want[0], want[1])                   # the skipped step changed nothing
    assert not R.within_bar(bad[-1], want[-1], STEPS) and R.worst_over_bar(bad[-1], want[-1], STEPS) > 10.0


def test_entry_points_refuse_bad_arguments_without_gpu():
    """null pointers, pointers off a 16-byte boundary and n <= 0 return -1 before any HIP call (the stand-in addresses are
    never dereferenced)"""
    import rad_mmm_amd._lib as L
    lib = L.lib
    a = 0x10000
    ok = dict(p=a, g=2 * a, m=3 * a, v=4 * a, n=1024, clip=None, step=5 * a, skip=None)

    def call(**over):
        k = dict(ok, **over)
        return lib.radmmm_adam_step(k["p"], k["g"], k["m"], k["v"], k["n"], k["clip"], k["step"], k["skip"], 1e-3, 0.9, 0.999,
                                    1e-8, 0.0, 0, None)
    for name in ("p", "g", "m", "v", "step"):
        assert call(**{name: None}) == -1, name
        assert lib.radmmm_last_error() == b"adam_step: bad arguments"
    for name in ("p", "g", "m", "v"):
        for off in (4, 8, 12, 1):
            assert call(**{name: ok[name] + off}) == -1, (name, off)
            assert lib.radmmm_last_error() == b"adam_step: the flat buffers must be 16B aligned"
    for n in (0, -1, -2 ** 40):
        assert call(n=n) == -1
        assert lib.radmmm_last_error() == b"adam_step: bad arguments"
    assert lib.radmmm_adam_advance(None, None, None) == -1 and lib.radmmm_last_error() == b"adam_advance: bad arguments"
    assert lib.radmmm_abi_version() == 4                      # the entry points are additive


def test_flat_adam_needs_gpu_parameters():
    with pytest.raises(ValueError, match="on the GPU"):
        FlatAdam([("w", torch.nn.Parameter(torch.zeros(3)))])
    with pytest.raises(ValueError, match="betas"):
        FlatAdam([("w", torch.nn.Parameter(torch.zeros(3)))], betas=(1.0, 0.999))
