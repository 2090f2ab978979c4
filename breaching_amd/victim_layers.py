"""Layers of the attacker's PRIVATE copy of the victim model that run on HIP kernels: eval-mode BatchNorm2d (+ the residual add and
the ReLU behind it) on kernel E and LayerNorm on kernel F, through both autograd orders the attack differentiates them in -- and the
autograd node of Conv2d, which launches no kernel of ours.

This module is the whole of the victim-model surface (SURVEY.md section 8 row a6 "stays PyTorch by design"):
the convolutions themselves in all three autograd orders, GEMMs, pooling, attention, softmax and the loss of the victim model stay
PyTorch-ROCm / MIOpen / rocBLAS.  What is here exists because PyTorch's DECOMPOSITION of the derivative of the backward pass was most
of an attack iteration -- for BatchNorm and LayerNorm most of the LAUNCH COUNT (about 700 of the 1 170 launches of a ResNet-18
iteration, more than half of a BERT-base iteration's), for Conv2d a quarter of the KERNEL TIME, spent on a weight gradient that
nothing reads -- not because the arithmetic is the attack's.

  * `use_affine_eval_batchnorm(model, mode, fuse_epilogue)`  -- class swap BatchNorm2d -> `_EvalAffineBatchNorm2d` (same parameters,
    buffers, hooks); `_EvalBNFunction` / `_EvalBNGradFunction` = kernel E's three launches as two chained autograd.Functions;
    `_PendingBatchNorm` = the lazy output that lets `+ identity` and `relu` ride in the BatchNorm's launches for ANY forward code;
    `FusedEpilogueError` + `fuse_bn_relu_policy` = the fail-open policy of that fusion (the attacker switches it off on a model it
    cannot serve, attacker.HipOptimizationAttacker._autograd_objective).
  * `use_hip_layernorm(model)`  -- LayerNorm -> `_HipLayerNorm` (kernel F).
  * `use_owned_conv_gradient(model)`  -- Conv2d -> `_HipConv2d`: `_ConvFunction` / `_ConvGradFunction` call the same ATen
    convolution ops as before (MIOpen's kernels, unchanged); what changed is which of them the outer pass calls.  ATen's
    double backward computes the objective's gradient with respect to the victim's WEIGHTS whenever the first-order input gradient
    exists, although the attack differentiates with respect to the candidate only; the node asks the engine and skips it.  It also
    hands the second of the two convolution outputs that make up the BatchNorm's incoming gradient to kernel E's second-order
    launch (bh_bn_eval_bwd_bwd2) instead of adding them with an elementwise launch.  What did not change: every convolution
    that is needed, its arguments, their order, and therefore every value the attack reads.

reference: none of this exists there -- the reference runs the victim model as it is (objectives.py:36-46); PyTorch's own eval-mode
batch_norm / layer_norm arithmetic through both orders, run in fp64, is the oracle (tests/test_gpu_kernels.py), and the stock Conv2d
the convolution node's (tests/test_conv_grad.py).
"""

import torch

from . import _lib
from .config import cfg_get as _cfg_get

def _vector_ready(t, hw):
    """Contiguous fp32, and 16-byte aligned when the kernels will use 16-byte accesses (H*W % 4 == 0)."""
    if not t.is_contiguous():
        t = t.contiguous()
    if hw % 4 == 0 and t.data_ptr() % 16:
        t = t.clone()
    return t


def _under_functorch(x):
    """True while a torch.func transform (vmap / grad / jvp ...) is active or `x` is one of its wrapper tensors.  The custom
    autograd Functions of kernels E / F carry no functorch rules (no setup_context / vmap staticmethods) and support exactly
    the two autograd orders the attack uses: under a transform the modules take the torch formulation instead."""
    try:
        from torch._C._functorch import is_functorch_wrapped_tensor, peek_interpreter_stack

        return bool(is_functorch_wrapped_tensor(x)) or peek_interpreter_stack() is not None
    except Exception:  # private API moved: be conservative only about what we can see
        return False


class _EvalBNFunction(torch.autograd.Function):
    """y = x * s_c + t_c of an eval-mode BatchNorm2d as ONE launch (bh_bn_eval_fwd); its backward is `_EvalBNGradFunction`, one
    launch again and itself differentiable -- the attack needs the derivative of the first-order pass (objectives.py:40-46
    under create_graph=True, then optimization_based_attack.py:160).

    Epilogue: with `residual` and / or `relu` the launch computes y = relu(x * s_c + t_c + residual) -- the tail of a ResNet
    block (`_PendingBatchNorm` decides when) -- and the two backward orders carry the ReLU mask (read back from y) and the
    residual's gradient.

    Outputs: y, an alias `xp` of the input, and -- with `tap` (a DeepInversion tap of this layer, priors._BnInputTap) -- a 0-dim
    token.  Both extras exist to let autograd hand this node EVERYTHING that flows back to this BatchNorm input in one call, so
    that one launch writes the sum and the engine has nothing left to accumulate:
      * `xp` is what the first-order backward differentiates with respect to (instead of x itself): in the attack's outer pass
        the derivative of that backward sends its d_x to `xp`, i.e. to this node, which adds it to gy * s_c inside
        bh_bn_eval_bwd (`gx_add`) -- otherwise two nodes each send a gradient to x's producer and autograd adds them with an
        ATen launch per layer;
      * the token is how the prior's statistic node sends back d objective / d total: the launch adds gout * (A_c + B_c * x)
        (it reads x anyway): the prior's backward costs no launch and no traffic of its own (regularizers.py:222-227 /
        deepinversion.py:93-103, math only).
    The engine calls a node only when the gradients of all its used outputs have arrived: correct by construction, no
    assumption about execution order."""

    @staticmethod
    def forward(ctx, x, weight, bias, inv_std, mean_inv, stats=None, tap=None, residual=None, relu=False):
        """`stats`: fp64 view of 2 * C * S words that receives sum(x), sum(x^2) per (channel, slab) -- kernel D's input."""
        lib = _lib.load()
        B, C = x.shape[0], x.shape[1]
        hw = x[0, 0].numel()
        xk = _vector_ready(x.detach(), hw)
        rk = None if residual is None else _vector_ready(residual.detach().to(torch.float32), hw)
        y = torch.empty_like(xk)
        with torch.cuda.device(x.device):
            _lib.check(lib.bh_bn_eval_fwd(_lib.ptr(xk), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(inv_std), _lib.ptr(mean_inv),
                                          _lib.ptr(y), _lib.ptr(stats), _lib.ptr(rk), int(bool(relu)), B, C, hw,
                                          _lib.current_stream_handle(x.device)), "bh_bn_eval_fwd")
        xp = x.view_as(x)
        # the alias of the INPUT is saved (not the detached kernel view): the backward below is differentiable with respect to
        # it; with a ReLU the OUTPUT is saved too -- its sign is the mask of both backward orders
        ctx.save_for_backward(xp, weight, inv_std, mean_inv, *([y] if relu else []))
        ctx.has_bias, ctx.relu, ctx.has_residual = bias is not None, bool(relu), residual is not None
        ctx.tap = None if tap is None else (tap.record, tap.layer)  # the record of THIS pass: its coefficients are what the backward applies
        ctx.set_materialize_grads(False)
        return (y, xp) if tap is None else (y, xp, x.new_empty(()))

    @staticmethod
    def backward(ctx, gy, g_xp=None, g_token=None):
        xp, weight, inv_std, mean_inv, *rest = ctx.saved_tensors
        mask = rest[0].detach() if ctx.relu else None  # a constant of every order (ReLU'' = 0 almost everywhere)
        none = (None,) * 9
        if g_token is None or ctx.tap is None:
            if gy is None:
                return (g_xp,) + none[1:]
            tap = None
        else:
            if torch.is_grad_enabled():
                raise NotImplementedError("The DeepInversion term fused into the BatchNorm backward supports no create_graph "
                                          "pass through it (set BREACH_HIP_BN_FUSED_TAP=0).")
            record, layer = ctx.tap
            _, coef_ptr = record.layer_coefficients(layer)
            if gy is None:
                gy = torch.zeros_like(xp)
            tap = (coef_ptr, g_token.detach().reshape(1).to(torch.float32), record.coef)
        fold = g_xp is not None and not torch.is_grad_enabled()  # the launch adds it; under create_graph a differentiable add does
        gx, gw, gb, gr = _EvalBNGradFunction.apply(gy, xp, weight, inv_std, mean_inv, mask, tap, ctx.has_residual, g_xp if fold else None)
        if g_xp is not None and not fold:
            gx = gx + g_xp
        return gx, (gw if weight is not None else None), (gb if ctx.has_bias else None), None, None, None, None, gr, None


class _EvalBNGradFunction(torch.autograd.Function):
    """(gy, x, weight) -> (gx, gw, gb, g_residual) in one launch (bh_bn_eval_bwd); backward = the derivative of that map in one
    launch (bh_bn_eval_bwd_bwd).  PyTorch's decomposition of the same three orders is ~35 launches per layer (+ 6 for a ReLU).
    `mask`: the forward output when the forward applied a ReLU (gy is masked by [y > 0] first); `tap` = (address of the layer's
    (A_c, B_c) pairs, gout, owner of that memory): gx additionally receives gout * (A_c + B_c * x); `want_residual`: also
    return the masked gradient itself, the gradient of the forward's residual input; `gx_add`: a constant added to gx."""

    @staticmethod
    def forward(ctx, gy, x, weight, inv_std, mean_inv, mask=None, tap=None, want_residual=False, gx_add=None):
        lib = _lib.load()
        B, C = x.shape[0], x.shape[1]
        hw = x[0, 0].numel()
        gyk = _vector_ready(gy.detach().to(torch.float32), hw)
        xk = _vector_ready(x.detach(), hw)
        mk = None if mask is None else _vector_ready(mask.detach(), hw)
        ak = None if gx_add is None else _vector_ready(gx_add.detach().to(torch.float32), hw)
        gx = torch.empty_like(xk)
        gr = torch.empty_like(xk) if want_residual else None
        gw = torch.empty(C, dtype=torch.float32, device=x.device)
        gb = torch.empty(C, dtype=torch.float32, device=x.device)
        slabs = lib.bh_bn_eval_slabs(B, C, hw)
        ws = torch.empty(2 * C * slabs, dtype=torch.float64, device=x.device) if slabs > 1 else None
        coef_ptr, gout = (tap[0], _lib.ptr(tap[1])) if tap is not None else (_lib.ptr(None), _lib.ptr(None))
        with torch.cuda.device(x.device):
            _lib.check(lib.bh_bn_eval_bwd(_lib.ptr(gyk), _lib.ptr(xk), _lib.ptr(weight), _lib.ptr(inv_std), _lib.ptr(mean_inv),
                                          _lib.ptr(gx), _lib.ptr(gw), _lib.ptr(gb), _lib.ptr(ws), coef_ptr, gout, _lib.ptr(mk), _lib.ptr(gr),
                                          _lib.ptr(ak), B, C, hw, _lib.current_stream_handle(x.device)), "bh_bn_eval_bwd")
        ctx.save_for_backward(gyk, xk, weight, inv_std, mean_inv, *([mk] if mk is not None else []))
        ctx.set_materialize_grads(False)
        ctx.extra_terms, ctx.masked = (tap is not None or gx_add is not None), mk is not None
        return gx, gw, gb, gr

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, ggx, ggw, ggb, ggr):
        lib = _lib.load()
        gy, x, weight, inv_std, mean_inv, *rest = ctx.saved_tensors
        mask = rest[0] if ctx.masked else None
        none = (None,) * 9
        ggx2 = _take_conv_term(ctx)  # the second term of ggx, left here by the convolution that consumed gx (`_ConvGradFunction`)
        if ggx is None:
            ggx, ggx2 = ggx2, None
        if ggx is None and ggw is None and ggb is None and ggr is None:
            return none
        if ctx.extra_terms:
            raise NotImplementedError("No derivative of the BatchNorm backward with the DeepInversion term / another gradient folded in.")
        B, C = x.shape[0], x.shape[1]
        hw = x[0, 0].numel()
        ggx = None if ggx is None else _vector_ready(ggx.to(torch.float32), hw)
        ggx2 = None if ggx2 is None else _vector_ready(ggx2.to(torch.float32), hw)
        ggr = None if ggr is None else _vector_ready(ggr.to(torch.float32), hw)
        ggw = None if ggw is None else ggw.to(torch.float32).contiguous()
        ggb = None if ggb is None else ggb.to(torch.float32).contiguous()
        d_gy = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        d_x = torch.empty_like(x) if (ctx.needs_input_grad[1] and ggw is not None) else None
        d_w = torch.empty(C, dtype=torch.float32, device=x.device) if (weight is not None and ctx.needs_input_grad[2] and ggx is not None) else None
        if d_gy is None and d_x is None and d_w is None:
            return none
        slabs = lib.bh_bn_eval_slabs(B, C, hw)
        ws = torch.empty(C * slabs, dtype=torch.float64, device=x.device) if slabs > 1 else None
        with torch.cuda.device(x.device):
            _lib.check(lib.bh_bn_eval_bwd_bwd2(_lib.ptr(ggx), _lib.ptr(ggx2), _lib.ptr(ggw), _lib.ptr(ggb), _lib.ptr(gy), _lib.ptr(x),
                                               _lib.ptr(weight), _lib.ptr(inv_std), _lib.ptr(mean_inv), _lib.ptr(d_gy), _lib.ptr(d_x),
                                               _lib.ptr(d_w), _lib.ptr(ws), _lib.ptr(mask), _lib.ptr(ggr), B, C, hw,
                                               _lib.current_stream_handle(x.device)), "bh_bn_eval_bwd_bwd2")
        return d_gy, d_x, d_w, None, None, None, None, None, None


def _take_conv_term(node):
    """Pop what `_ConvGradFunction.backward` left on this `_EvalBNGradFunction` node: (graph task id, tensor).  Only an entry of
    the backward pass that is running now counts; anything else is a leftover of a pass that ended early and is dropped."""
    entry = getattr(node, "_conv_term", None)
    if entry is None:
        return None
    node._conv_term = None
    return entry[1] if entry[0] == torch._C._current_graph_task_id() else None


def _engine_wants(edge):
    """Will the backward pass that is running now use the gradient sent along `edge` (an entry of a node's `next_functions`)?
    `ctx.needs_input_grad` only says `requires_grad`; the engine knows which nodes lie on a path to the `inputs` of this
    autograd.grad call.  No node: nobody.  The query raises for a leaf that is itself one of those inputs (and outside a backward
    pass): then the answer is yes -- computing too much is always correct."""
    node = edge[0] if edge is not None else None
    if node is None:
        return False
    try:
        return bool(torch._C._will_engine_execute_node(node))
    except RuntimeError:
        return True


_aten = torch.ops.aten


class _ConvFunction(torch.autograd.Function):
    """y = convolution(x, w, b) -- MIOpen's, through ATen, as before; its backward is `_ConvGradFunction`, one
    aten.convolution_backward and itself differentiable.  What is owned here is only how the derivative of that backward is
    decomposed (`_ConvGradFunction.backward`)."""

    @staticmethod
    def forward(ctx, x, w, b, stride, padding, dilation, groups):
        ctx.geometry = (list(stride), list(padding), list(dilation), int(groups))
        ctx.bias_sizes = None if b is None else [w.shape[0]]
        ctx.save_for_backward(x, w)
        return _aten.convolution(x, w, b, ctx.geometry[0], ctx.geometry[1], ctx.geometry[2], False, [0] * len(ctx.geometry[0]), groups)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        none = (None,) * 7
        # the stem's input gradient is not on the way to the parameters: skipped in the first-order pass (ATen's output mask did that)
        mask = tuple(bool(ctx.needs_input_grad[i]) and _engine_wants(ctx.next_functions[i]) for i in range(3))
        if not any(mask):
            return none
        producer = gy.grad_fn if gy.output_nr == 0 and getattr(gy.grad_fn, "_forward_cls", None) is _EvalBNGradFunction else None
        gx, gw, gb = _ConvGradFunction.apply(gy, x, w, ctx.geometry, mask, ctx.bias_sizes, producer)
        return (gx, gw, gb) + none[3:]


class _ConvGradFunction(torch.autograd.Function):
    """(gy, x, w) -> (gx, gw, gb): one aten.convolution_backward with the output mask of what the running pass uses.

    backward = the derivative of that map for incoming (ggx, ggw, ggb), each possibly absent:
        d_gy = conv(ggx, w) + conv(x, ggw) + ggb          d_x = conv_backward_input(gy, ggw)          d_w = conv_backward_weight(gy, ggx)
    ATen's `_convolution_double_backward` computes the same three, but d_w whenever ggx is defined -- also when the pass
    differentiates with respect to the candidate only and the engine has masked that output off, which is every iteration of
    the attack.  d_w is a convolution of a [C, B, H, W] "input" with a [K, B, H, W] "filter", the shape MIOpen serves worst:
    about a quarter of a ResNet-18 iteration's kernel time went into a result nobody read.  Here it is launched only when the
    engine will use it (FedAvg's multi-step updates, whose weights depend on the candidate: gm.py), as a real weight-gradient
    call.

    `producer`: the `_EvalBNGradFunction` node whose output gy is, when it is one.  In the outer pass d_gy is that node's
    incoming ggx; instead of adding the two convolution outputs with an elementwise launch, the first is returned and the
    second is left on the node, whose one launch reads both (bh_bn_eval_bwd_bwd2: the same fp32 add, no launch)."""

    @staticmethod
    def forward(ctx, gy, x, w, geometry, mask, bias_sizes, producer):
        stride, padding, dilation, groups = geometry
        ctx.geometry, ctx.producer = geometry, producer
        ctx.save_for_backward(gy, x, w)
        ctx.set_materialize_grads(False)
        return _aten.convolution_backward(gy, x, w, bias_sizes, stride, padding, dilation, False, [0] * len(stride), groups, list(mask))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, ggx, ggw, ggb):
        gy, x, w = ctx.saved_tensors
        stride, padding, dilation, groups = ctx.geometry
        zeros = [0] * len(stride)
        want = [bool(ctx.needs_input_grad[i]) and _engine_wants(ctx.next_functions[i]) for i in range(3)]
        d_gy = d_x = d_w = None
        if want[0]:
            t1 = None if ggx is None else _aten.convolution(ggx, w, None, stride, padding, dilation, False, zeros, groups)
            t2 = None if ggw is None else _aten.convolution(x, ggw, None, stride, padding, dilation, False, zeros, groups)
            if t1 is not None and t2 is not None:
                d_gy = t1 if ggb is None and _leave_on_producer(ctx, t2) else t1 + t2
            else:
                d_gy = t1 if t2 is None else t2
            if ggb is not None:
                bias = ggb.reshape(1, -1, *([1] * (gy.dim() - 2)))
                d_gy = bias.expand_as(gy) if d_gy is None else d_gy + bias
        if want[1] and ggw is not None:
            d_x = _aten.convolution_backward(gy, x, ggw, None, stride, padding, dilation, False, zeros, groups, [True, False, False])[0]
        if want[2] and ggx is not None:
            d_w = _aten.convolution_backward(gy, ggx, w, None, stride, padding, dilation, False, zeros, groups, [False, True, False])[1]
        return d_gy, d_x, d_w, None, None, None, None


def _leave_on_producer(ctx, term):
    """Hand `term`, the second summand of d_gy, to the `_EvalBNGradFunction` node that produced gy, if the running pass will run
    that node (it then receives the first summand as its ggx from the engine, after this node: it depends on it)."""
    producer = ctx.producer
    if producer is None or ctx.next_functions[0] != (producer, 0):
        return False
    try:
        if not torch._C._will_engine_execute_node(producer):
            return False
    except RuntimeError:
        return False
    task = torch._C._current_graph_task_id()
    entry = getattr(producer, "_conv_term", None)
    if entry is not None and entry[0] == task:
        term = entry[1] + term
    producer._conv_term = (task, term)
    return True


class _HipConv2d(torch.nn.Conv2d):
    """torch.nn.Conv2d (same parameters, hooks, `isinstance`; instances converted by swapping ``__class__``) whose forward goes
    through `_ConvFunction`.  The convolutions of every autograd order are still ATen's / MIOpen's; see `_ConvGradFunction`.
    Not tied to a device.  Non-zero padding modes, string padding, non-floating or unbatched inputs and torch.func transforms
    take the stock forward."""

    def forward(self, x):
        if isinstance(x, _PendingBatchNorm):
            x = x.value()
        if (self.padding_mode != "zeros" or isinstance(self.padding, str) or x.dim() != 4 or not x.is_floating_point()
                or x.dtype != self.weight.dtype or torch.is_autocast_enabled(x.device.type) or _under_functorch(x)):
            return super().forward(x)
        return _ConvFunction.apply(x, self.weight, self.bias, self.stride, self.padding, self.dilation, self.groups)


def use_owned_conv_gradient(model):
    """Convert every plain Conv2d of `model` in place (idempotent).  On by default; cfg.impl.owned_conv_grad=False or
    BREACH_HIP_CONV_GRAD=0 keeps the stock modules."""
    for module in model.modules():
        if type(module) is torch.nn.Conv2d:
            module.__class__ = _HipConv2d
    return model


def owned_conv_grad_enabled(cfg):
    import os

    env = os.environ.get("BREACH_HIP_CONV_GRAD")
    if env is not None:
        return env.strip().lower() not in ("0", "false", "off", "no")
    flag = _cfg_get(cfg.impl, "owned_conv_grad", True)
    return True if flag is None else bool(flag)


def _launch_eval_bn(module, x, sink, tap, residual, relu):
    """One kernel E forward launch of `module` on `x` (+ residual, ReLU); hands the DeepInversion tap its token."""
    inv_std, mean_inv = module._frozen_statistics()
    out = _EvalBNFunction.apply(x, module.weight, module.bias, inv_std, mean_inv, sink, tap, residual, relu)
    if tap is not None:
        tap.token = out[2]
    return out[0]  # out[1], the input's alias, lives on only as the node's saved tensor


_RELU_OUT_OF_PLACE = (torch.relu, torch.nn.functional.relu, torch.Tensor.relu)
_RELU_IN_PLACE = (torch.relu_, torch.Tensor.relu_, torch.nn.functional.relu_)
_ADD_OUT_OF_PLACE = (torch.add, torch.Tensor.add, torch.Tensor.__add__, torch.Tensor.__radd__)
_ADD_IN_PLACE = (torch.Tensor.add_, torch.Tensor.__iadd__)


class FusedEpilogueError(RuntimeError):
    """The deferred BatchNorm launch (`_PendingBatchNorm`) met a consumer it cannot serve.  With cfg.impl.fuse_bn_relu = "auto" (the
    default) the attacker catches it on the model copy it happened on, switches the epilogue fusion off there and repeats the
    evaluation; "required" lets it through."""


class _PendingBatchNorm(torch.Tensor):
    """The not-yet-launched output of an eval-mode BatchNorm on kernel E: a metadata-only tensor that waits for its first
    consumer.  `+ identity` / `+= identity` is absorbed as the launch's residual, `relu` / `relu_` launches
    y = relu(x * s + t + residual) in one kernel; any other use launches the plain affine map (then the residual add, if one
    was absorbed) and carries on with an ordinary tensor.  Works on arbitrary Python `forward` code (torchvision-style
    BasicBlock / Bottleneck included) without tracing or rewriting the victim model; in-place forms update this object, so
    code that does not rebind the result (`self.relu(out)` with inplace=True, `out.add_(identity)`) sees the right values.

    reference: none -- the reference runs the victim model as it is (objectives.py:36-46); this is launch-count reduction for
    the attacker's private model copy (~110 of ~717 launches per ResNet-18 iteration, profiles/r4_op_attribution.txt)."""

    @staticmethod
    def __new__(cls, module, x, sink, tap):
        self = torch.Tensor._make_wrapper_subclass(cls, x.shape, dtype=x.dtype, device=x.device, requires_grad=False)
        self._module, self._x, self._sink, self._tap = module, x, sink, tap
        self._residual, self._value = None, None
        self._graph_expected = torch.is_grad_enabled() and x.requires_grad
        if tap is not None:
            tap.pending = self  # the DeepInversion prior launches whatever is still waiting when it is evaluated
        return self

    def launch(self, relu=False):
        """Run the kernel now (the only place this object's computation happens)."""
        if self._graph_expected and not torch.is_grad_enabled():
            # Created where autograd was recording, consumed where it is not: the consumer is almost certainly the forward of a
            # custom autograd.Function, which received this metadata-only wrapper as an input and therefore has no autograd
            # edge to the BatchNorm input -- its gradient would silently stop here.  Fail loudly instead.
            raise FusedEpilogueError("An eval-mode BatchNorm output was handed to a custom autograd.Function (or consumed inside a "
                                     "no_grad block) before any ordinary operation used it; the deferred BatchNorm launch cannot "
                                     "carry an autograd edge there.  cfg.impl.fuse_bn_relu='auto' (the default) falls back to "
                                     "un-fused launches on this model; False (or BREACH_HIP_FUSE_BN_RELU=0) never defers.")
        return _launch_eval_bn(self._module, self._x, self._sink, self._tap, self._residual, relu)

    def value(self):
        """The plain (un-fused) result, computed once: affine map, plus the absorbed residual if there is one."""
        if self._value is None:
            residual, self._residual = self._residual, None
            y = self.launch(relu=False)
            self._value = y if residual is None else y + residual
        return self._value

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        first = args[0] if args else None
        fresh = isinstance(first, cls) and first._value is None
        if fresh and len(args) == 1 and func in _RELU_OUT_OF_PLACE and not kwargs.get("inplace", False):
            out = first.launch(relu=True)  # `first` itself stays pending: a second consumer still gets the un-clamped values --
            first._sink = first._tap = None  # -- but the statistics sink and the DeepInversion tap belong to this first launch only
            return out
        if fresh and len(args) == 1 and (func in _RELU_IN_PLACE or (func is torch.nn.functional.relu and kwargs.get("inplace", False))):
            first._value = first.launch(relu=True)
            return first._value
        if func in _ADD_OUT_OF_PLACE or func in _ADD_IN_PLACE:
            plain_alpha = kwargs.get("alpha", 1) == 1 and set(kwargs) <= {"alpha"} and len(args) == 2
            if plain_alpha and torch.is_tensor(args[1]) and torch.is_tensor(first):
                a, b = args
                if func in _ADD_OUT_OF_PLACE and not (isinstance(a, cls) and a._value is None and a._residual is None):
                    a, b = b, a  # identity + bn(...)
                if (isinstance(a, cls) and a._value is None and a._residual is None and b is not a and b.shape == a.shape
                        and b.dtype == a.dtype and b.device == a.device):
                    other = b.value() if isinstance(b, cls) else b
                    if func in _ADD_IN_PLACE:
                        if a is args[0]:
                            a._residual = other
                            return a
                    else:
                        merged = cls(a._module, a._x, a._sink, a._tap)
                        merged._residual = other
                        a._sink = a._tap = None  # handed on to `merged`: a later use of `a` itself launches without them
                        return merged
        name = getattr(func, "__name__", "")
        if name == "__get__" and args and isinstance(first, cls) and getattr(getattr(func, "__self__", None), "__name__", "") in (
                "shape", "dtype", "device", "ndim", "is_cuda", "layout"):
            with torch._C.DisableTorchFunctionSubclass():  # metadata of the wrapper itself: no launch
                return func(*args, **kwargs)

        def real(obj):
            if isinstance(obj, cls):
                return obj.value()
            if isinstance(obj, (list, tuple)):
                return type(obj)(real(o) for o in obj)
            return obj

        with torch._C.DisableTorchFunctionSubclass():
            return func(*[real(a) for a in args], **{k: real(v) for k, v in kwargs.items()})

    @classmethod
    def __torch_dispatch__(cls, func, types, args=(), kwargs=None):  # reached only by callers that bypass __torch_function__
        def real(obj):
            if isinstance(obj, cls):
                return obj.value()
            if isinstance(obj, (list, tuple)):
                return type(obj)(real(o) for o in obj)
            return obj

        return func(*[real(a) for a in args], **{k: real(v) for k, v in (kwargs or {}).items()})

    def __repr__(self):
        return f"_PendingBatchNorm(shape={tuple(self.shape)}, residual={self._residual is not None}, launched={self._value is not None})"


def fuse_bn_relu_policy(cfg=None):
    """BatchNorm -> (+ residual) -> ReLU in kernel E's launches: "auto" (default: on; a victim model whose forward hands a BatchNorm
    output straight to a custom autograd.Function or a no_grad consumer -- the one thing the deferred launch cannot serve -- gets
    the fusion switched off on its copy at the first evaluation, with a warning and a note in stats["execution"]), "required" (that
    case raises) or "off".  cfg.impl.fuse_bn_relu = True / "auto" / "required" / False, or BREACH_HIP_FUSE_BN_RELU = 1 / auto /
    required / 0.  The reference attacks arbitrary models (objectives.py:36-46): the default must never be the reason one cannot be."""
    import os

    flag = os.environ.get("BREACH_HIP_FUSE_BN_RELU")
    if flag is None:
        flag = _cfg_get(cfg.impl, "fuse_bn_relu", True) if cfg is not None else True
    if flag is None:
        return "auto"
    if isinstance(flag, str):
        flag = flag.strip().lower()
        if flag in ("required", "require", "strict"):
            return "required"
        return "off" if flag in ("0", "false", "off", "no") else "auto"
    return "auto" if bool(flag) else "off"


def fuse_bn_relu_enabled(cfg=None):
    return fuse_bn_relu_policy(cfg) != "off"


class _EvalAffineBatchNorm2d(torch.nn.BatchNorm2d):
    """BatchNorm2d whose inference-mode forward is the per-channel affine map it is: ``y = x * s + t`` with
    ``s = w / sqrt(var + eps)``, ``t = b - mean * s``.

    Same parameters, buffers, hooks and ``isinstance`` behaviour as ``torch.nn.BatchNorm2d`` (instances are converted by
    swapping ``__class__``); only the op sequence differs.  PyTorch's double backward of ``F.batch_norm`` in eval mode
    decomposes into dozens of small kernels per layer per iteration.  Mode "hip" (default): one HIP launch per autograd order
    (`_EvalBNFunction`); mode "addcmul" (round 2): one broadcast multiply-add in torch ops, autograd decomposes the rest.
    Training-mode batches, non-4-D, non-fp32 or non-ROCm inputs fall through to the stock / torch path."""

    eval_mode = "hip"
    fuse_epilogue = True  # let the residual add and the ReLU that follow ride in this layer's launches (`_PendingBatchNorm`)

    def _runs_on_hip(self, x):
        """Kernel E takes fp32 [B, C, H, W] ROCm activations within its index range (B * HW < 2^31, numel < 2^40), outside
        torch.func transforms; everything else runs the torch formulation below (same values, more launches)."""
        if not (not self.training and self.running_mean is not None and self.running_var is not None and x.dim() == 4
                and self.eval_mode == "hip" and x.is_cuda and x.dtype == torch.float32 and x.numel() > 0):
            return False
        if x.shape[0] * x.shape[2] * x.shape[3] >= 2 ** 31 or x.numel() >= 2 ** 40:
            return False
        return not _under_functorch(x)

    def accepts_stats_sink(self, x):
        """True when the coming forward of `x` will go through kernel E and can fill a per-(channel, slab) statistics buffer
        (the DeepInversion prior's taps ask, priors._BnInputTap)."""
        return self._runs_on_hip(x)

    def forward(self, x):
        if isinstance(x, _PendingBatchNorm):  # BatchNorm fed directly by a BatchNorm: an autograd.Function must never see the
            x = x.value()                      # metadata-only wrapper as an input (it carries no autograd edge)
        sink = self.__dict__.pop("_bn_stats_sink", None)  # set by a DeepInversion tap for this one call
        tap = self.__dict__.pop("_bn_tap", None)           # likewise: the tap whose token this forward has to emit
        if tap is not None and not self._runs_on_hip(x):   # (the tap asked `accepts_stats_sink` on the same x: not reached)
            from .priors import _BnTap

            x, tap.token = _BnTap.apply(x, tap.record, tap.layer)
            tap.x, tap.live, tap.in_producer, tap = x.detach(), x, False, None
        if self.training or self.running_mean is None or self.running_var is None or x.dim() != 4:
            return super().forward(x)
        inv_std, mean_inv = self._frozen_statistics()
        if self._runs_on_hip(x):
            if self.fuse_epilogue and fuse_bn_relu_enabled():
                return _PendingBatchNorm(self, x, sink, tap)  # launched by its first consumer (relu / + identity / anything)
            return _launch_eval_bn(self, x, sink, tap, None, False)
        if self.weight is not None:
            scale = self.weight * inv_std
            shift = -(self.weight * mean_inv)
        else:
            scale, shift = inv_std, -mean_inv
        if self.bias is not None:
            shift = shift + self.bias
        return torch.addcmul(shift.view(1, -1, 1, 1), x, scale.view(1, -1, 1, 1))

    def _frozen_statistics(self):
        """1/sqrt(var+eps) and mean/sqrt(var+eps): constants of the attack (the buffers are fixed once the model is
        rebuilt from the payload), recomputed only if a buffer is written to."""
        key = (self.running_mean._version, self.running_var._version, self.running_var.data_ptr(), self.running_var.device)
        cached = getattr(self, "_frozen", None)
        if cached is None or cached[0] != key:
            with torch.no_grad():
                inv_std = torch.rsqrt(self.running_var + self.eps).to(torch.float32).contiguous()
                cached = (key, inv_std, (self.running_mean * inv_std).to(torch.float32).contiguous())
            self._frozen = cached
        return cached[1], cached[2]


def use_affine_eval_batchnorm(model, mode="hip", fuse_epilogue=True):
    """Convert every plain BatchNorm2d of `model` in place (idempotent).  On by default; cfg.impl.fast_eval_bn (True / "hip" /
    "addcmul" / False) or BREACH_HIP_FAST_BN (1 / hip / addcmul / 0) choose the formulation or keep the stock modules;
    `fuse_epilogue` (cfg.impl.fuse_bn_relu / BREACH_HIP_FUSE_BN_RELU): the following residual add and ReLU ride in the launch."""
    for module in model.modules():
        if type(module) is torch.nn.BatchNorm2d:
            module.__class__ = _EvalAffineBatchNorm2d
        if type(module) is _EvalAffineBatchNorm2d:
            module.eval_mode = mode
            module.fuse_epilogue = bool(fuse_epilogue)
    return model


def fast_eval_bn_mode(cfg):
    """"hip" (default), "addcmul" or None (stock modules)."""
    import os

    flag = os.environ.get("BREACH_HIP_FAST_BN")
    if flag is None:
        flag = _cfg_get(cfg.impl, "fast_eval_bn", True)
    if flag is None or flag is True:
        return "hip"
    if flag is False:
        return None
    flag = str(flag).strip().lower()
    if flag in ("0", "false", "off", "no", "stock"):
        return None
    return "addcmul" if flag == "addcmul" else "hip"


def fast_eval_bn_enabled(cfg):
    return fast_eval_bn_mode(cfg) is not None


class _LayerNormFunction(torch.autograd.Function):
    """LayerNorm over the last dimension as ONE launch (bh_ln_fwd); its backward is `_LayerNormGradFunction`, itself
    differentiable -- the text attacks need the derivative of the first-order pass (objectives.py:40-46 under
    create_graph=True, then optimization_with_label_attack.py:168-174)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        lib = _lib.load()
        D = x.shape[-1]
        xk = x.detach().contiguous()
        R = xk.numel() // D
        y = torch.empty_like(xk)
        mean = torch.empty(R, dtype=torch.float32, device=x.device)
        rstd = torch.empty(R, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.bh_ln_fwd(_lib.ptr(xk), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(y), _lib.ptr(mean), _lib.ptr(rstd), R, D,
                                     float(eps), _lib.current_stream_handle(x.device)), "bh_ln_fwd")
        ctx.save_for_backward(x, weight, mean, rstd)  # the input itself: the backward below is differentiable in it
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, mean, rstd = ctx.saved_tensors
        gx, gw, gb = _LayerNormGradFunction.apply(gy, x, weight, mean, rstd)
        return gx, (gw if weight is not None else None), (gb if ctx.has_bias else None), None


class _LayerNormGradFunction(torch.autograd.Function):
    """(gy, x, weight) -> (gx, gweight, gbias) in two launches (bh_ln_bwd: rows, then columns); backward = the derivative of
    that map (bh_ln_bwd_bwd: rows, then columns for d_weight).  `mean` / `rstd` are cached functions of x: the derivative
    with respect to x accounts for them.  PyTorch's decomposition of the same orders is ~83 launches per layer."""

    @staticmethod
    def forward(ctx, gy, x, weight, mean, rstd):
        lib = _lib.load()
        D = x.shape[-1]
        xk = x.detach().contiguous()
        gyk = gy.detach().to(torch.float32).contiguous()
        R = xk.numel() // D
        gx = torch.empty_like(xk)
        gw = torch.empty(D, dtype=torch.float32, device=x.device)
        gb = torch.empty(D, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.bh_ln_bwd(_lib.ptr(gyk), _lib.ptr(xk), _lib.ptr(weight), _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(gx),
                                     _lib.ptr(gw), _lib.ptr(gb), R, D, _lib.current_stream_handle(x.device)), "bh_ln_bwd")
        ctx.save_for_backward(gyk, xk, weight, mean, rstd)
        ctx.set_materialize_grads(False)
        return gx, gw, gb

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, u, s, t):
        lib = _lib.load()
        gy, x, weight, mean, rstd = ctx.saved_tensors
        if u is None and s is None and t is None:
            return None, None, None, None, None
        D = x.shape[-1]
        R = x.numel() // D
        u = None if u is None else u.to(torch.float32).contiguous()
        s = None if s is None else s.to(torch.float32).contiguous()
        t = None if t is None else t.to(torch.float32).contiguous()
        d_gy = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        d_x = torch.empty_like(x) if ctx.needs_input_grad[1] else None
        want_dw = weight is not None and ctx.needs_input_grad[2] and u is not None
        d_w = torch.empty(D, dtype=torch.float32, device=x.device) if want_dw else None
        rows = torch.empty(2 * R, dtype=torch.float32, device=x.device) if want_dw else None
        if d_gy is None and d_x is None and d_w is None:
            return None, None, None, None, None
        with torch.cuda.device(x.device):
            _lib.check(lib.bh_ln_bwd_bwd(_lib.ptr(u), _lib.ptr(s), _lib.ptr(t), _lib.ptr(gy), _lib.ptr(x), _lib.ptr(weight),
                                         _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(d_gy), _lib.ptr(d_x), _lib.ptr(d_w), _lib.ptr(rows), R, D,
                                         _lib.current_stream_handle(x.device)), "bh_ln_bwd_bwd")
        return d_gy, d_x, d_w, None, None


class _HipLayerNorm(torch.nn.LayerNorm):
    """torch.nn.LayerNorm (same parameters, hooks, `isinstance`; instances converted by swapping ``__class__``) whose forward is
    kernel F when it normalises the last dimension of an fp32 ROCm tensor; anything else takes the stock path."""

    def forward(self, x):
        if isinstance(x, _PendingBatchNorm):
            x = x.value()
        if (len(self.normalized_shape) == 1 and x.is_cuda and x.dtype == torch.float32 and x.numel() > 0
                and x.shape[-1] == self.normalized_shape[0] and x.numel() < 2 ** 31 and not _under_functorch(x)):
            return _LayerNormFunction.apply(x, self.weight, self.bias, self.eps)
        return super().forward(x)


def use_hip_layernorm(model):
    """Convert every plain LayerNorm of `model` in place (idempotent).  On by default; cfg.impl.fast_layer_norm=False or
    BREACH_HIP_FAST_LN=0 keeps the stock modules."""
    for module in model.modules():
        if type(module) is torch.nn.LayerNorm:
            module.__class__ = _HipLayerNorm
    return model


def fast_layer_norm_enabled(cfg):
    import os

    env = os.environ.get("BREACH_HIP_FAST_LN")
    if env is not None:
        return env.strip().lower() not in ("0", "false", "off", "no")
    flag = _cfg_get(cfg.impl, "fast_layer_norm", True)
    return True if flag is None else bool(flag)
