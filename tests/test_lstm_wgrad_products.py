"""bilstm(..., wgrad_products=1): the context LSTM's three weight-gradient GEMMs (dW_ih and the two dW_hh) on ONE f16 product
from the hi planes (radmmm_wgrad_rmh_shift), at the smallest shapes that take the split-f16 path (B * T >= 4096, the shapes of
test_hip_lstm.py).  Nothing but the four weight gradients may move, they move within the one-product bound, and the choice is
made in forward."""
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(16, 256, 64, 36, None), (18, 230, 52, 40, [230] * 9 + [100, 64, 7] * 3)]
WEIGHTS = ("weight_ih_l0", "weight_hh_l0", "weight_ih_l0_reverse", "weight_hh_l0_reverse")
BIASES = ("bias_ih_l0", "bias_hh_l0", "bias_ih_l0_reverse", "bias_hh_l0_reverse")


def _run(B, T, I, H, lens, products, between=None, x_grad=True):
    """forward + backward of one fresh module (same parameters, inputs and output gradient every time: the module's gradient
    scale starts from the same state) -> y, dx, parameter gradients, and the backward's own operands dG, x, y (rows)."""
    from rad_mmm_amd.lstm import bilstm
    g = torch.Generator().manual_seed(B * 100 + H)
    lstm = nn.LSTM(I, H, num_layers=1, batch_first=True, bidirectional=True)
    with torch.no_grad():
        for p in lstm.parameters():
            p.copy_((torch.rand(p.shape, generator=g) - 0.5) * 0.6)
    lstm = lstm.to(DEV)
    x = torch.randn(B, T, I, generator=g).to(DEV).requires_grad_(x_grad)
    gy = (torch.randn(B, T, 2 * H, generator=g) * 1e-3).to(DEV)
    lens_d = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    y = bilstm(lstm, x, lens_d) if products is None else bilstm(lstm, x, lens_d, wgrad_products=products)
    fn = y.grad_fn
    if between is not None:
        between()
    (y * gy).sum().backward(retain_graph=True)                   # (kept only to read the node's saved tensors below)
    saved = fn.saved_tensors
    ops_ = {"x": saved[0].clone(), "dG": saved[1].clone(), "y": saved[3].clone()}      # G holds the pre-activation gradients now
    return y.detach(), x.grad, {n: p.grad for n, p in lstm.named_parameters()}, ops_


@pytest.fixture(scope="module")
def runs():
    cache = {}

    def get(shape_id, products):
        if (shape_id, products) not in cache:
            cache[(shape_id, products)] = _run(*SHAPES[shape_id], products)
        return cache[(shape_id, products)]
    return get


@pytest.mark.parametrize("shape_id", [0, 1])
def test_one_product_moves_only_the_weight_gradients(shape_id, runs):
    """wgrad_products = 1 against 3 (and 3 is the default): y, dx and the four bias gradients are bit-equal; each of the four
    weight gradients differs, elementwise by at most 2^-10 * |dG|^T |operand| + 3e-6 * max |g3| -- two round-to-nearest fp16
    operands per product and the fp32 accumulation, the bound of test_wgrad_one_pass.py's kernel test -- with dG, x and
    h_prev (y moved by one frame inside each utterance) the backward's own fp32 tensors."""
    B, T, I, H, lens = SHAPES[shape_id]
    y3, dx3, g3, o3 = runs(shape_id, 3)
    y1, dx1, g1, o1 = runs(shape_id, 1)
    yd, dxd, gd, _ = runs(shape_id, None)
    assert torch.equal(y1, y3) and torch.equal(dx1, dx3) and torch.equal(yd, y3) and torch.equal(dxd, dx3)
    for n in BIASES + WEIGHTS:
        assert torch.equal(gd[n], g3[n]), n
    for n in BIASES:
        assert torch.equal(g1[n], g3[n]), n
    for k in o3:
        assert torch.equal(o1[k], o3[k]), k
    dG, x2, yr = o3["dG"].double().abs(), o3["x"].double().abs(), o3["y"].double().abs().view(B, T, 2 * H)
    hp = torch.zeros_like(yr)
    hp[:, 1:, :H] = yr[:, :-1, :H]
    hp[:, :-1, H:] = yr[:, 1:, H:]
    hp = hp.view(B * T, 2 * H)
    mag = {"weight_ih_l0": dG[:, :4 * H].t() @ x2, "weight_ih_l0_reverse": dG[:, 4 * H:].t() @ x2,
           "weight_hh_l0": dG[:, :4 * H].t() @ hp[:, :H], "weight_hh_l0_reverse": dG[:, 4 * H:].t() @ hp[:, H:]}
    for n in WEIGHTS:
        assert not torch.equal(g1[n], g3[n]), n
        bound = 2.0 ** -10 * mag[n] + 3e-6 * g3[n].double().abs().max()
        used = float(((g1[n].double() - g3[n].double()).abs() / bound).max())
        l2 = float((g1[n].double() - g3[n].double()).norm() / g3[n].double().norm())
        print(f"lstm {SHAPES[shape_id][:4]} {n}: largest |g1 - g3| / bound {used:.3f}, L2 rel {l2:.2e}")
        assert used <= 1.0, (n, used)


def test_product_count_is_fixed_in_forward(runs, monkeypatch):
    """The count travels from forward to backward on the autograd node: RADMMM_WGRAD_PRODUCTS (what RADMMMFlow derives its
    argument from) flipped between the two changes nothing, for either count."""
    for products, other in ((1, "2"), (3, "1")):
        _, dx, g, _ = runs(1, products)
        _, dxf, gf, _ = _run(*SHAPES[1], products, between=lambda: monkeypatch.setenv("RADMMM_WGRAD_PRODUCTS", other))
        assert torch.equal(dx, dxf)
        for n in g:
            assert torch.equal(g[n], gf[n]), n


def test_one_product_without_an_input_gradient(runs):
    """x needs no gradient: dG's lo plane is not produced at all (nobody reads it), and the hi plane the weight gradients
    contract has the same bits -- every parameter gradient equals the run that also computed dx."""
    _, dx, g, _ = _run(*SHAPES[0], 1, x_grad=False)
    assert dx is None
    for n, v in runs(0, 1)[2].items():
        assert torch.equal(g[n], v), n


def test_wgrad_products_is_validated():
    from rad_mmm_amd.lstm import bilstm
    lstm = nn.LSTM(6, 5, num_layers=1, batch_first=True, bidirectional=True).to(DEV)
    with pytest.raises(ValueError, match="wgrad_products"):
        bilstm(lstm, torch.randn(2, 4, 6, device=DEV), None, wgrad_products=2)
