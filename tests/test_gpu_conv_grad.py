"""Kernel E's second-order launch with its incoming gradient in two terms (bh_bn_eval_bwd_bwd2), and the wiring that feeds it:
the convolution gradient node leaves the second term of d_gy on the BatchNorm gradient node behind it (victim_layers)."""

import copy
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


# (B, C, HW), the smallest that reach each code path: scalar (HW % 4 != 0), narrow float4 (one wavefront per channel), wide with one
# slab, and slab-split with the combine launch (B * HW >= 12288)
KERNEL_SHAPES = [(1, 3, 49), (2, 5, 16), (1, 4, 2048), (1, 2, 12288)]


@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=["scalar", "narrow", "wide", "slabs"])
def test_two_term_launch_is_bit_identical_to_adding_the_terms_first(shape, hip_lib):
    """bh_bn_eval_bwd_bwd2(ggx=a, ggx2=b) against bh_bn_eval_bwd_bwd(ggx=a+b), the sum taken by torch on the GPU: d_gy, d_x and
    d_w bit for bit, with and without the ReLU mask and the residual's term, with and without ggw / ggb, and with no ggx at all."""
    from breaching_amd import _lib

    B, C, HW = shape
    slabs = hip_lib.bh_bn_eval_slabs(B, C, HW)
    assert (slabs > 1) == (shape == KERNEL_SHAPES[3])
    gen = torch.Generator().manual_seed(B * 1000 + C * 100 + HW)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(_dev())  # noqa: E731
    a, b, gy, x, y, ggr = (rnd(B, C, HW) for _ in range(6))
    b[0, 0, :3] = -a[0, 0, :3]  # exact cancellation: the sum is +0, whatever the signs
    weight, ggw, ggb = rnd(C), rnd(C), rnd(C)
    inv_std, mean_inv = rnd(C).abs() + 0.5, rnd(C)
    total = a + b
    ptr = _lib.ptr

    def launch(two_terms, ggx, ggx2, masked, affine):
        d_gy, d_x = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
        d_w = torch.full((C,), float("nan"), device=_dev())
        ws = torch.empty(C * slabs, dtype=torch.float64, device=_dev()) if slabs > 1 else None
        head = (ptr(ggx), ptr(ggx2)) if two_terms else (ptr(ggx),)
        fn = hip_lib.bh_bn_eval_bwd_bwd2 if two_terms else hip_lib.bh_bn_eval_bwd_bwd
        status = fn(*head, ptr(ggw if affine else None), ptr(ggb if affine else None), ptr(gy), ptr(x), ptr(weight), ptr(inv_std),
                    ptr(mean_inv), ptr(d_gy), ptr(d_x), ptr(d_w), ptr(ws), ptr(y if masked else None), ptr(ggr if masked else None),
                    B, C, HW, _lib.current_stream_handle(_dev()))
        assert status == 0
        return d_gy, d_x, d_w

    for masked, affine in itertools.product((False, True), (False, True)):
        want = launch(False, total, None, masked, affine)
        got = launch(True, a, b, masked, affine)
        assert not any(torch.isnan(t).any() for t in want)
        for name, g, w in zip(("d_gy", "d_x", "d_w"), got, want):
            assert torch.equal(g, w), (name, masked, affine, float((g - w).abs().max()))
        lone = launch(True, total, None, masked, affine)  # ggx2 = NULL is the old entry point
        assert all(torch.equal(g, w) for g, w in zip(lone, want))
        none_want, none_got = launch(False, None, None, masked, affine), launch(True, None, None, masked, affine)
        assert all(torch.equal(g, w) for g, w in zip(none_got, none_want))


class _Block(torch.nn.Module):
    def __init__(self, c_in, c_out, stride):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(c_in, c_out, 3, stride, 1, bias=False)
        self.bn1 = torch.nn.BatchNorm2d(c_out)
        self.conv2 = torch.nn.Conv2d(c_out, c_out, 3, 1, 1, bias=False)
        self.bn2 = torch.nn.BatchNorm2d(c_out)
        self.relu = torch.nn.ReLU(inplace=True)
        self.downsample = None
        if stride != 1 or c_in != c_out:
            self.downsample = torch.nn.Sequential(torch.nn.Conv2d(c_in, c_out, 1, stride, bias=False), torch.nn.BatchNorm2d(c_out))

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        out += identity
        return self.relu(out)


def _toy_resnet():
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, 1, 1, bias=False), torch.nn.BatchNorm2d(8), torch.nn.ReLU(inplace=True),
                                _Block(8, 8, 1), _Block(8, 8, 2), torch.nn.AdaptiveAvgPool2d(1), torch.nn.Flatten(), torch.nn.Linear(8, 5))
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.3)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.2)
    return model.eval()


def test_conv_node_hands_its_second_term_to_the_batchnorm_launch(hip_lib):
    """A two-block toy ResNet (8 channels, 16 x 16, one stride-2 block with a 1 x 1 downsample) with the BatchNorm and the
    convolution swaps together: the second-order input gradient against the same model in fp64 on the CPU, next to the stock fp32
    modules on the GPU (referee and yardstick of test_resnet_blocks_run_fused_and_match_the_stock_modules, same factor); the
    second-order launch sees a second term once per conv -> BatchNorm pair whose convolution has both (all six but the stem, which
    has no first-order input gradient); and a second outer pass over the retained graph gives the same bits (nothing stale)."""
    import breaching_amd.victim_layers as V

    base = _toy_resnet()
    stock = copy.deepcopy(base).to(_dev())
    owned = V.use_owned_conv_gradient(V.use_affine_eval_batchnorm(copy.deepcopy(base).to(_dev()), "hip"))
    exact = copy.deepcopy(base).double()
    x = torch.randn(2, 3, 16, 16)

    second_terms = []
    inner = hip_lib.bh_bn_eval_bwd_bwd2

    def spy(*args):
        second_terms.append(bool(args[1].value))
        return inner(*args)

    def evaluate(model, xin, passes=1):
        xq = xin.clone().requires_grad_(True)
        grads = torch.autograd.grad(model(xq).logsumexp(1).sum(), list(model.parameters()), create_graph=True)
        objective = sum((g * g).sum() for g in grads)
        outs = [torch.autograd.grad(objective, xq, retain_graph=True)[0] for _ in range(passes)]
        return [t.detach().double().cpu() for t in outs]

    hip_lib.bh_bn_eval_bwd_bwd2 = spy
    try:
        with torch.backends.cudnn.flags(deterministic=True):  # two passes are compared bit for bit: no atomically accumulating solver
            got, again = evaluate(owned, x.to(_dev()), passes=2)
    finally:
        hip_lib.bh_bn_eval_bwd_bwd2 = inner
    assert len(second_terms) == 12 and sum(second_terms[:6]) == 5 and sum(second_terms[6:]) == 5, second_terms
    assert torch.equal(got, again)
    (plain,), (want,) = evaluate(stock, x.to(_dev())), evaluate(exact, x.double())
    err_owned = float((got - want).norm() / want.norm())
    err_stock = float((plain - want).norm() / want.norm())
    print(f"  toy resnet second-order input gradient, relative error vs fp64: owned {err_owned:.2e}, stock torch modules {err_stock:.2e}")
    assert err_owned <= max(10.0 * err_stock, 2e-2), (err_owned, err_stock)
