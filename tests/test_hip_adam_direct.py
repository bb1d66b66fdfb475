"""radmmm_adam_advance / radmmm_adam_step through the C ABI against the float64 restatement tests/_adam_ref.py: every tail
length, more than one workgroup, the size where the grid-stride loop wraps (the launch is capped at 4096 workgroups of 256
lanes with 4 elements each), both decay modes, with and without a clip coefficient; the skip word; memory outside [0, n);
determinism.

Bars (tests/test_radam.py:55): rtol 2e-6, atol 2e-7 after the 5 steps, rtol 1e-6, atol 1e-7 after the first.  Why they
hold for a right kernel: a step rounds p twice (the decay, the subtraction), 2^-24 = 6e-8 relative each, so 5 steps stay
below 10 * 6e-8 = 6e-7 in the worst case; the update itself is lr = 1e-2 times a quotient of a few fp32 roundings
(relative 1e-6 at most), 1e-8 absolute.  Both are inside the bars with room, and far from the planted variants of
tests/test_adam_cpu.py, which miss by more than 10 bars on this problem."""
import numpy as np
import pytest
import torch

import _adam_ref as R
from rad_mmm_amd._lib import check, lib, ptr, stream

ADAM_STEP, ADAM_ADVANCE = lib.radmmm_adam_step, lib.radmmm_adam_advance

pytestmark = pytest.mark.gpu

STEPS = 5
PAD = 8                                                        # floats of NaN on either side of every array (32 bytes)
WRAP = 4 * (4096 * 256 + 1) + 3
SIZES = (1, 3, 4, 5, 1023, 1024, 1025, WRAP)
HYPER = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
CLIP = 0.37

_problems = {}


def _keep_coupled_gradient_conditioned(gr, p0):
    """Adam's update is lr * g / (|g| + eps)-like: where the coupled gradient c g + wd p cancels to about eps, the fp32
    rounding of that sum (2^-24 of its larger term) moves the update by a large part of lr, for ANY fp32 implementation,
    and among 4 M elements a few always land there.  Those elements test the conditioning of the problem, not the kernel,
    so the data keeps |c g + wd p| above a quarter of its larger term for c in {CLIP, 1} and for every p within 0.06 of p0
    (5 steps move p by at most 5 lr = 0.05): a gradient inside the band where the two terms can cancel gets p0's sign, or,
    where p may change sign (|p0| <= 0.06), the magnitude 0.05, which is above the band."""
    wd, drift = HYPER["weight_decay"], 0.06
    a, ap = np.abs(gr), np.abs(p0)
    band = (a >= wd * np.maximum(ap - drift, 0.0) / 4) & (a <= 4 * wd * (ap + drift) / CLIP)
    keeps_sign = ap > drift
    gr[band & keeps_sign] = (a * np.sign(p0))[band & keeps_sign]
    gr[band & ~keeps_sign] = (np.float32(0.05) * np.where(gr < 0, -1, 1))[band & ~keeps_sign]


def _problem(n):
    """(p0, grads) as float32 numpy arrays, made once per size and never written to"""
    if n not in _problems:
        g = np.random.default_rng(n)
        p0 = g.standard_normal(n).astype(np.float32)
        grads = [(g.standard_normal(n) * 10.0 ** g.uniform(-3, 1, n)).astype(np.float32) for _ in range(STEPS)]
        for gr in grads:
            _keep_coupled_gradient_conditioned(gr, p0)
        for k, gr in enumerate(grads):                         # a few gradients where sqrt(v) is of eps' size
            gr[:: 97] = 1e-9 * (k + 1)
        for a in [p0] + grads:
            a.setflags(write=False)
        _problems[n] = (p0, grads)
    return _problems[n]


class _Arrays:
    """p, g, m, v of n elements, each 16-byte aligned inside a buffer whose pads hold NaN; the counter; the skip word"""

    def __init__(self, n, p0, dev="cuda:0"):
        self.n = n
        self.bufs = {k: torch.full((n + 2 * PAD,), float("nan"), device=dev) for k in "pgmv"}
        for k in "pgmv":
            setattr(self, k, self.bufs[k][PAD: PAD + n])
            assert getattr(self, k).data_ptr() % 16 == 0
        self.p.copy_(torch.from_numpy(p0))
        self.m.zero_()
        self.v.zero_()
        self.step = torch.zeros(1, device=dev, dtype=torch.int32)
        self.skip = torch.zeros(1, device=dev, dtype=torch.int32)
        self.clip = torch.full((1,), CLIP, device=dev)

    def update(self, g, decoupled, clip, skip=False):
        self.g.copy_(torch.from_numpy(g) if isinstance(g, np.ndarray) else g)
        self.skip.fill_(1 if skip else 0)
        b1, b2 = HYPER["betas"]
        check(ADAM_ADVANCE(ptr(self.step), ptr(self.skip), stream()), "adam_advance")
        check(ADAM_STEP(ptr(self.p), ptr(self.g), ptr(self.m), ptr(self.v), self.n, ptr(self.clip) if clip else None,
                                   ptr(self.step), ptr(self.skip), HYPER["lr"], b1, b2, HYPER["eps"], HYPER["weight_decay"],
                                   1 if decoupled else 0, stream()), "adam_step")

    def bits(self):
        return [self.bufs[k].clone().view(torch.int32) for k in "pmv"] + [self.step.clone()]

    def pads_untouched(self):
        return all(bool(torch.isnan(b[:PAD]).all()) and bool(torch.isnan(b[PAD + self.n:]).all()) for b in self.bufs.values())


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("decoupled,clip", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("n", SIZES)
def test_five_steps_against_float64(n, decoupled, clip):
    p0, grads = _problem(n)
    clip64 = float(np.float32(CLIP))
    want, m64, v64, _ = R.run(p0, grads, clips=[clip64] * STEPS if clip else None, decoupled=decoupled, **HYPER)
    a = _Arrays(n, p0)
    for k in range(STEPS):
        a.update(grads[k], decoupled, clip)
        if k == 0:
            got = a.p.cpu().numpy()
            print(f"n={n} step 1: {R.worst_over_bar(got, want[0], 1):.3g} of the bar")
            assert R.within_bar(got, want[0], 1)
    got = a.p.cpu().numpy()
    print(f"n={n} step {STEPS}: {R.worst_over_bar(got, want[-1], STEPS):.3g} of the bar")
    assert R.within_bar(got, want[-1], STEPS)
    # the moments: v is a sum of non-negative terms (relative bar); m can cancel, so its bar is relative to the largest
    # gradient the element saw (in coupled mode the gradient includes weight_decay * p, and |p| stays below |p0| + 1)
    gmax = np.max(np.abs(np.stack(grads)), axis=0).astype(np.float64) + HYPER["weight_decay"] * (np.abs(p0) + 1.0)
    assert np.all(np.abs(a.m.cpu().numpy() - m64) <= 2e-6 * gmax)
    assert np.allclose(a.v.cpu().numpy(), v64, rtol=2e-6, atol=0.0)
    assert int(a.step.item()) == STEPS
    assert a.pads_untouched()


@pytest.mark.parametrize("n", (5, 1025, WRAP))
def test_skip_keeps_every_bit_and_the_next_step_is_step_one(n):
    p0, grads = _problem(n)
    poison = torch.from_numpy(grads[1].copy())
    poison[0] = float("nan")
    poison[n // 2] = float("inf")
    poison[n - 1] = float("-inf")
    for decoupled in (False, True):
        a = _Arrays(n, p0)
        before = a.bits()
        a.update(poison, decoupled, clip=True, skip=True)
        assert _same(a.bits(), before) and int(a.step.item()) == 0 and a.pads_untouched()
        a.update(grads[0], decoupled, clip=True)
        fresh = _Arrays(n, p0)
        fresh.update(grads[0], decoupled, clip=True)
        assert _same(a.bits(), fresh.bits()) and int(a.step.item()) == 1
        # a skip in mid-run: the moments and the count of step 1 stay, poisoned gradient or not
        mid = a.bits()
        a.update(poison, decoupled, clip=False, skip=True)
        assert _same(a.bits(), mid)


@pytest.mark.parametrize("n", (1023, WRAP))
def test_two_identical_runs_give_identical_bits(n):
    p0, grads = _problem(n)
    runs = []
    for _ in range(2):
        a = _Arrays(n, p0)
        for k in range(3):
            a.update(grads[k], True, clip=True)
        runs.append(a.bits())
    assert _same(*runs)
