"""The convolution gradient node of the victim copy (`victim_layers._ConvFunction` / `_ConvGradFunction`) against the stock
torch.nn.Conv2d through the two autograd orders the attack uses.  ATen ops only: runs without a GPU.

What must hold: everything the attack reads -- the first-order parameter gradients and the outer pass's gradient with respect to
the candidate -- comes from the same ATen calls as before and is bitwise equal; the outer pass's weight gradient, computed only
when the engine will use it, now comes from a weight-gradient call and agrees with fp64 as well as the stock path does; and an
outer pass with respect to the candidate alone launches no weight-gradient convolution at all."""

import copy

import pytest
import torch

import breaching_amd.victim_layers as V

# (C_in of the case conv is 4; input is [2, 3, size, size]) kernel, stride, padding, dilation, groups, K, size
CASES = {
    "3x3_s1_p1": dict(kernel_size=3, stride=1, padding=1, size=9),
    "3x3_s2_p1_even": dict(kernel_size=3, stride=2, padding=1, size=8),
    "3x3_s2_p1_odd": dict(kernel_size=3, stride=2, padding=1, size=9),
    "1x1_s2": dict(kernel_size=1, stride=2, padding=0, size=9),
    "7x7_s2_p3": dict(kernel_size=7, stride=2, padding=3, size=13),
    "dilation2": dict(kernel_size=3, stride=1, padding=2, dilation=2, size=9),
    "groups2": dict(kernel_size=3, stride=1, padding=1, groups=2, out_channels=4, size=8),
}


def _net(case, bias, dtype):
    spec = dict(CASES[case])
    spec.pop("size")
    torch.manual_seed(11)
    layers = [torch.nn.Conv2d(3, 4, 3, padding=1, bias=bias), torch.nn.Tanh(),
              torch.nn.Conv2d(4, spec.pop("out_channels", 5), bias=bias, **spec), torch.nn.Tanh()]
    return torch.nn.Sequential(*layers).to(dtype)


def _input(case, dtype):
    torch.manual_seed(5)
    size = CASES[case]["size"]
    return torch.randn(2, 3, size, size).to(dtype)


def _two_orders(model, x0, wrt_params=True):
    """(first-order parameter gradients, d objective / d x, d objective / d parameters or None) of a gradient-matching objective."""
    x = x0.clone().requires_grad_(True)
    params = list(model.parameters())
    first = torch.autograd.grad(model(x).square().mean(), params, create_graph=True)
    torch.manual_seed(3)
    objective = sum(((g - torch.randn(g.shape).to(g.dtype)) ** 2).sum() for g in first)  # the same fp32 targets in either precision
    (dx,) = torch.autograd.grad(objective, x, retain_graph=wrt_params)
    dw = torch.autograd.grad(objective, params) if wrt_params else None
    return [g.detach() for g in first], dx, dw


def _relative(a_list, ref_list):
    """One figure per comparison: relative L2 deviation over all tensors together (a per-tensor maximum of a handful of
    elements is decided by single roundings and says nothing about a factor of two)."""
    a = torch.cat([t.double().flatten() for t in a_list])
    ref = torch.cat([t.double().flatten() for t in ref_list])
    return float((a - ref).norm() / ref.norm())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("case", list(CASES))
def test_what_the_attack_reads_is_bitwise_what_the_stock_modules_give(case, bias, dtype):
    """(a) first-order parameter gradients and the outer pass's d/dx: the same ATen calls in the same order, difference 0."""
    stock = _net(case, bias, dtype)
    owned = V.use_owned_conv_gradient(copy.deepcopy(stock))
    assert all(type(m) is V._HipConv2d for m in owned if isinstance(m, torch.nn.Conv2d))
    x = _input(case, dtype)
    assert torch.equal(owned(x), stock(x))
    first_s, dx_s, _ = _two_orders(stock, x, wrt_params=False)
    first_o, dx_o, _ = _two_orders(owned, x, wrt_params=False)
    for a, b in zip(first_o, first_s):
        assert torch.equal(a, b)
    assert torch.equal(dx_o, dx_s)


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("case", list(CASES))
def test_weight_gradient_of_the_outer_pass_is_as_close_to_fp64_as_the_stock_path(case, bias):
    """(b) d objective / d parameters, through autograd.grad with the parameters among the inputs and through .backward():
    against the stock modules in fp64; the fp32 node may deviate at most twice as much as the stock fp32 modules do (its weight
    gradient is a weight-gradient call, ATen's a forward convolution of transposed operands: other summation order)."""
    exact = _net(case, bias, torch.float64)
    stock = _net(case, bias, torch.float32)
    owned = V.use_owned_conv_gradient(copy.deepcopy(stock))
    x = _input(case, torch.float32)
    _, dx_e, dw_e = _two_orders(exact, x.double())
    _, dx_s, dw_s = _two_orders(stock, x)
    _, dx_o, dw_o = _two_orders(owned, x)
    assert torch.equal(dx_o, dx_s)
    err_owned, err_stock = _relative(dw_o, dw_e), _relative(dw_s, dw_e)
    print(f"  {case} bias={bias}: d/dw relative deviation from fp64: owned {err_owned:.3e}, stock {err_stock:.3e}")
    assert err_owned <= 2.0 * err_stock, (err_owned, err_stock)

    def by_backward(model, xin):
        model.zero_grad()
        xq = xin.clone().requires_grad_(True)
        params = list(model.parameters())
        first = torch.autograd.grad(model(xq).square().mean(), params, create_graph=True)
        torch.manual_seed(3)
        sum(((g - torch.randn(g.shape).to(g.dtype)) ** 2).sum() for g in first).backward()
        assert xq.grad is not None and all(p.grad is not None for p in params)  # no `inputs`: every leaf is filled
        return [xq.grad] + [p.grad for p in params]

    want, plain, got = by_backward(exact, x.double()), by_backward(stock, x), by_backward(owned, x)
    err_owned, err_stock = _relative(got, want), _relative(plain, want)
    print(f"  {case} bias={bias}: .backward() relative deviation from fp64: owned {err_owned:.3e}, stock {err_stock:.3e}")
    assert err_owned <= 2.0 * err_stock, (err_owned, err_stock)


def _conv_events(event):
    """aten::convolution / aten::convolution_backward events below `event` in the profiler's tree."""
    found = []
    for child in event.cpu_children:
        if child.name in ("aten::convolution", "aten::convolution_backward"):
            found.append(child)
        else:
            found.extend(_conv_events(child))
    return found


def test_outer_pass_wrt_the_input_launches_no_weight_gradient_convolution():
    """(c) torch.profiler over the outer backward with respect to the input only: no aten::convolution whose "input" is the
    [C, B, H, W] transpose ATen's double backward builds for gW; every `_ConvGradFunction` node runs exactly two convolutions
    and one convolution_backward (one and one for the stem, whose first-order input gradient was never computed: no ggx)."""
    from torch.profiler import ProfilerActivity, profile

    torch.manual_seed(0)
    B, C = 2, 6  # B != every channel count: a [C, B, H, W] operand cannot be mistaken for an activation
    model = torch.nn.Sequential(torch.nn.Conv2d(3, C, 3, padding=1), torch.nn.Tanh(), torch.nn.Conv2d(C, C, 3, stride=2, padding=1),
                                torch.nn.Tanh(), torch.nn.Conv2d(C, 5, 1, bias=False))
    x0 = torch.randn(B, 3, 10, 10)

    def trace(net):
        x = x0.clone().requires_grad_(True)
        first = torch.autograd.grad(net(x).square().mean(), list(net.parameters()), create_graph=True)
        objective = sum((g * g).sum() for g in first)
        with profile(activities=[ProfilerActivity.CPU], record_shapes=True) as prof:
            torch.autograd.grad(objective, x)
        return prof.events()

    def transposed_operand(events):
        return [e for e in events if e.name == "aten::convolution" and e.input_shapes[0][:2] in ([3, B], [C, B], [5, B])]

    assert len(transposed_operand(trace(model))) == 2  # the stock modules: gW of the two convolutions that have a ggI
    events = trace(V.use_owned_conv_gradient(copy.deepcopy(model)))
    assert transposed_operand(events) == []
    nodes = [e for e in events if e.name == "_ConvGradFunctionBackward"]
    assert len(nodes) == 3
    counts = sorted(tuple(sum(c.name == n for c in _conv_events(node)) for n in ("aten::convolution", "aten::convolution_backward"))
                    for node in nodes)
    assert counts == [(1, 1), (2, 1), (2, 1)], counts
    # the whole pass: those, and one input-gradient call per convolution of the forward graph the objective also flows through
    assert sum(e.name == "aten::convolution" for e in events) == 5 and sum(e.name == "aten::convolution_backward" for e in events) == 6


class _Scale(torch.autograd.Function):
    """A custom node directly behind a convolution, differentiable twice."""

    @staticmethod
    def forward(ctx, x, k):
        ctx.k = k
        return x * k

    @staticmethod
    def backward(ctx, g):
        return _Scale.apply(g, ctx.k), None


def test_a_custom_node_directly_behind_the_convolution():
    torch.manual_seed(1)
    conv_a, conv_b = torch.nn.Conv2d(3, 4, 3, padding=1), torch.nn.Conv2d(4, 4, 3, padding=1, bias=False)

    def build(swap):
        a, b = copy.deepcopy(conv_a), copy.deepcopy(conv_b)
        net = torch.nn.Sequential(a, torch.nn.Tanh(), b)
        if swap:
            V.use_owned_conv_gradient(net)

        class Wrapped(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.net = net

            def forward(self, x):
                return torch.tanh(_Scale.apply(self.net(x), 0.5))

        return Wrapped()

    x = torch.randn(2, 3, 8, 8)
    first_s, dx_s, dw_s = _two_orders(build(False), x)
    first_o, dx_o, dw_o = _two_orders(build(True), x)
    assert all(torch.equal(a, b) for a, b in zip(first_o, first_s)) and torch.equal(dx_o, dx_s)
    for a, b in zip(dw_o, dw_s):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_weights_that_depend_on_the_input_get_their_gradient(dtype):
    """FedAvg's multi-step update (gm.py): the second local step runs on weights that are a function of the candidate, so the
    outer pass with respect to the candidate alone needs d/dw of the second step's convolutions -- the engine query says so."""
    from torch.func import functional_call

    torch.manual_seed(2)
    stock = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3, padding=1), torch.nn.Tanh(), torch.nn.Conv2d(4, 4, 3, stride=2, padding=1)).to(dtype)
    owned = V.use_owned_conv_gradient(copy.deepcopy(stock))
    exact = copy.deepcopy(stock).double()
    x0 = torch.randn(2, 3, 8, 8).to(dtype)

    def local_update(model, x0):
        x = x0.clone().requires_grad_(True)
        names = [n for n, _ in model.named_parameters()]
        server = [p for _, p in model.named_parameters()]
        params = server
        for _ in range(2):
            loss = functional_call(model, dict(zip(names, params)), (x,)).square().mean()
            grads = torch.autograd.grad(loss, params, create_graph=True)
            params = [p - 0.1 * g for p, g in zip(params, grads)]
        objective = sum(((p - s) ** 2).sum() for p, s in zip(params, server))
        (dx,) = torch.autograd.grad(objective, x)
        return dx

    want, plain, got = local_update(exact, x0.double()), local_update(stock, x0), local_update(owned, x0)
    err_owned, err_stock = _relative([got], [want]), _relative([plain], [want])
    print(f"  two local steps, {dtype}: d/dx relative deviation from fp64: owned {err_owned:.3e}, stock {err_stock:.3e}")
    assert err_owned <= 2.0 * err_stock if dtype == torch.float32 else err_owned <= 1e-13, (err_owned, err_stock)


def test_a_third_differentiation_raises():
    """`_ConvGradFunction.backward` is once_differentiable, like kernel E's second order: a pass that reaches it again raises."""
    torch.manual_seed(4)
    model = V.use_owned_conv_gradient(torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3, padding=1), torch.nn.Tanh(), torch.nn.Conv2d(4, 2, 3)))
    x = torch.randn(1, 3, 6, 6, requires_grad=True)
    first = torch.autograd.grad(model(x).square().mean(), list(model.parameters()), create_graph=True)
    (second,) = torch.autograd.grad(sum((g * g).sum() for g in first), x, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        second.square().sum().backward()


def test_swap_and_fall_through_rules():
    """(d) the class swap keeps parameters, hooks and isinstance, is idempotent and survives deepcopy; padding modes other than
    zeros, string padding, integer inputs and torch.func transforms take the stock forward."""
    torch.manual_seed(6)
    model = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3, padding=1), torch.nn.Conv2d(4, 4, 3, padding=1, padding_mode="reflect"),
                                torch.nn.Conv2d(4, 4, 3, padding="same"), torch.nn.ConvTranspose2d(4, 2, 2))
    weights = [m.weight for m in model]
    seen = []
    model[0].register_forward_hook(lambda mod, args, out: seen.append(type(mod)))
    V.use_owned_conv_gradient(model)
    V.use_owned_conv_gradient(model)
    assert [type(m) for m in model] == [V._HipConv2d, V._HipConv2d, V._HipConv2d, torch.nn.ConvTranspose2d]
    assert all(isinstance(m, torch.nn.Conv2d) for m in model[:3]) and all(m.weight is w for m, w in zip(model, weights))
    clone = copy.deepcopy(model)
    assert type(clone[0]) is V._HipConv2d and clone[0].weight is not model[0].weight
    assert torch.nn.Sequential(*model).state_dict().keys() == torch.nn.Sequential(*clone).state_dict().keys()

    x = torch.randn(2, 3, 8, 8, requires_grad=True)
    names = []
    h = x
    for m in clone:
        h = m(h)
        names.append(type(h.grad_fn).__name__)
    assert names[0] == "_ConvFunctionBackward" and names[1] == names[2] == "ConvolutionBackward0", names
    assert seen == [V._HipConv2d]  # the hook came along, through the swap and the deepcopy

    conv = clone[0]
    stock = torch.nn.Conv2d(3, 4, 3, padding=1)
    stock.load_state_dict(conv.state_dict())
    x = torch.randn(2, 3, 8, 8)
    got = torch.func.grad(lambda t: conv(t).square().sum())(x)  # under a transform: the stock forward, which functorch can differentiate
    assert torch.equal(got, torch.func.grad(lambda t: stock(t).square().sum())(x))
    assert torch.equal(torch.func.vmap(lambda t: conv(t[None])[0])(x), torch.func.vmap(lambda t: stock(t[None])[0])(x))
    assert torch.equal(conv(x[0]), stock(x[0]))  # unbatched
    with torch.no_grad():
        assert torch.equal(conv(x), stock(x))
    with pytest.raises(RuntimeError):
        conv(torch.ones(1, 3, 8, 8, dtype=torch.int64))  # the stock forward's own error, not ours


def test_switch_reads_config_and_environment(monkeypatch):
    from breaching_amd import get_attack_config

    monkeypatch.delenv("BREACH_HIP_CONV_GRAD", raising=False)
    assert V.owned_conv_grad_enabled(get_attack_config("invertinggradients", []))
    assert not V.owned_conv_grad_enabled(get_attack_config("invertinggradients", ["impl.owned_conv_grad=False"]))
    monkeypatch.setenv("BREACH_HIP_CONV_GRAD", "0")
    assert not V.owned_conv_grad_enabled(get_attack_config("invertinggradients", []))
    monkeypatch.setenv("BREACH_HIP_CONV_GRAD", "1")
    assert V.owned_conv_grad_enabled(get_attack_config("invertinggradients", ["impl.owned_conv_grad=False"]))


def test_two_term_second_order_launch_rejects_bad_arguments_before_launching(hip_lib):
    """bh_bn_eval_bwd_bwd2 on the host (no launch, no GPU): a second term without a first is BH_EINVAL (a lone term is passed as
    ggx), and the second term obeys the 16-byte alignment rule of the first when H * W is a multiple of four."""
    lib = hip_lib
    ok = 16  # a non-null, 16-byte aligned fake address: validation never dereferences
    tail = (None, None, ok, ok, None, ok, ok, ok, ok, None, None, None, None)  # ggw, ggb, gy, x, weight, inv_std, mean_inv, d_gy, d_x, ...
    assert lib.bh_bn_eval_bwd_bwd2(None, ok, *tail, 1, 4, 16, None) == -1          # ggx2 without ggx
    assert lib.bh_bn_eval_bwd_bwd2(ok, ok + 4, *tail, 1, 4, 16, None) == -1        # misaligned for 16-byte access
    assert lib.bh_bn_eval_bwd_bwd2(ok + 4, ok, *tail, 1, 4, 16, None) == -1
    assert lib.bh_bn_eval_bwd_bwd2(ok, ok, *tail, 8, 4, 112 * 112, None) == -1     # S > 1 needs a workspace
    assert lib.bh_bn_eval_bwd_bwd2(ok, ok, None, None, None, ok, None, ok, ok, ok, ok, None, None, None, None, 1, 4, 16, None) == -1  # gy missing
    assert lib.bh_bn_eval_bwd_bwd2(ok, ok, *tail, 0, 4, 16, None) == -1            # B = 0
