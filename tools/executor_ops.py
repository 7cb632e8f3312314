"""Op-level graphs for the executor arms no model's graph produces: small nn.Modules that drive the executor entry points
(adamml_amd/runtime.py) directly.  Plain module (it never touches torch.cuda), loaded by path as `executor_ops`: tests/test_executor_gpu.py runs them on the GPU against the
forced float64 replay, tests/test_executor_ref_cpu.py anchors the replay of the same graphs to torch autograd, tools/launch_trace.py
traces them -- one definition, so the traced row and the checked row cannot drift.

Every graph: G = 2 BatchNorm groups, 2 images of 12 x 12 (or 11 x 11) per group, 8 input channels.  `_run` has the models' signature; the
Lazy it returns the data of is kept in `.out_lazy` (Replay.output_of designates it), and the tape's first closure hands it the output gradient.
The entry points are looked up in this module's namespace at call time, so executor_ref.Recorder wraps them here as it does in the models."""
import torch
import torch.nn as nn

from adamml_amd.runtime import (ACT_NONE, ACT_RELU, ConvState, Lazy, NetRT, add_act, conv_bn, conv_bn_add, conv_bn_add_supported,  # noqa: F401
                                materialize, maxpool3x3s2)

GROUPS = 2


class OpsNet(nn.Module):
    hw = 12

    def __init__(self):
        super().__init__()
        self.rt = NetRT()
        self.out_lazy = None
        self.states = {}

    def cs(self, conv):
        s = self.states.get(id(conv))
        if s is None:
            s = self.states[id(conv)] = ConvState(conv.weight, conv.stride[0], conv.padding[0], depthwise=conv.groups > 1)
        return s

    def make_input(self, seed=5):
        x = torch.randn(GROUPS * 2, self.hw, self.hw, 8, generator=torch.Generator().manual_seed(seed))
        return x.to(torch.bfloat16)

    def out_shape(self, x):
        raise NotImplementedError

    def graph(self, rt, x):
        raise NotImplementedError

    def _run(self, x, groups, need_grad):
        rt = self.rt
        tape = rt.begin_forward(x.device, self.training, need_grad, groups)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                self.cs(m).repack(need_grad)
        out = self.out_lazy = self.graph(rt, Lazy(x, requires_grad=False))
        rt.end_forward()
        tape.record(lambda: setattr(out, "grad", tape.grad_out.to(torch.bfloat16).contiguous()))
        return out.data, tape


class SharedDepthwiseInput(OpsNet):
    """A depthwise conv that is not the sole consumer of its input (unfused weight gradient, accumulating data gradient) and an
    activated add of two plain tensors (adamml_act_bwd_from_output: neither operand has BatchNorm vectors to take sums for).
    The depthwise conv's BatchNorm is linear: were both operands of the add outputs of a ReLU, the add's own mask would only close
    positions whose gradient the operands' ReLUs close anyway, and a backward that skipped it would compute the same gradients."""

    def __init__(self):
        super().__init__()
        self.pw, self.dw = nn.Conv2d(8, 16, 1, bias=False), nn.Conv2d(16, 16, 3, padding=1, groups=16, bias=False)
        self.bn1, self.bn2 = nn.BatchNorm2d(16), nn.BatchNorm2d(16)

    def out_shape(self, x):
        return (x.shape[0], self.hw, self.hw, 16)

    def graph(self, rt, x):
        h = conv_bn(rt, x, self.cs(self.pw), self.bn1, ACT_RELU)
        a = conv_bn(rt, h, self.cs(self.dw), self.bn2, ACT_NONE)
        return add_act(rt, materialize(rt, a), materialize(rt, h), ACT_RELU)

    def torch_forward(self, xg):
        h = torch.relu(self.bn1(self.pw(xg)))
        return torch.relu(self.bn2(self.dw(h)) + h)


class AlgGemmArm(OpsNet):
    """conv_bn(8 -> 256, ReLU) -> conv_bn(256 -> 512, 1x1, linear BatchNorm) -> materialize: the 256 -> 512 conv meets _alg_supported
    with Cin = ALG_GEMM_CIN, so its backward forms W^T diag(B_g) W and W G_g for both groups through adamml_gemm_f32.
    fused=True: the same conv as conv_bn_add (no identity), which computes G in the forward pass and hands it to the backward."""

    def __init__(self, fused=False):
        super().__init__()
        self.fused = fused
        self.c1, self.c2 = nn.Conv2d(8, 256, 1, bias=False), nn.Conv2d(256, 512, 1, bias=False)
        self.bn1, self.bn2 = nn.BatchNorm2d(256), nn.BatchNorm2d(512)

    def out_shape(self, x):
        return (x.shape[0], self.hw, self.hw, 512)

    def graph(self, rt, x):
        h = conv_bn(rt, x, self.cs(self.c1), self.bn1, ACT_RELU)
        if self.fused:
            if not conv_bn_add_supported(rt, h, self.cs(self.c2), rt.tape.need_grad):
                raise RuntimeError("AlgGemmArm: conv_bn_add refuses the 256 -> 512 conv")
            return conv_bn_add(rt, h, self.cs(self.c2), self.bn2, None, ACT_NONE)
        z = conv_bn(rt, h, self.cs(self.c2), self.bn2, ACT_NONE, sole_consumer=True)
        return materialize(rt, z)

    def torch_forward(self, xg):
        return self.bn2(self.c2(torch.relu(self.bn1(self.c1(xg)))))


class UnfusedMaxpool(OpsNet):
    """h = conv_bn(ReLU); p = maxpool3x3s2(h) (NOT the sole consumer); q = conv_bn(h, 1x1 stride 2, linear); out = relu(q + p).
    The tape runs in reverse, so the consumer issued LAST finds h.grad unclaimed: pool_first=True -> the conv's data gradient writes and
    adamml_maxpool2d_bwd accumulates (acc = 1); pool_first=False -> the pool's backward writes (acc = 0) and the data gradient accumulates.
    Either way h's gradient arrives as that of its activated value: h's own backward (the plain arm) applies the ReLU mask itself."""
    hw = 11

    def __init__(self, pool_first=True):
        super().__init__()
        self.pool_first = pool_first
        self.c1, self.c2 = nn.Conv2d(8, 16, 1, bias=False), nn.Conv2d(16, 16, 1, stride=2, bias=False)
        self.bn1, self.bn2 = nn.BatchNorm2d(16), nn.BatchNorm2d(16)

    def out_shape(self, x):
        return (x.shape[0], (self.hw + 1) // 2, (self.hw + 1) // 2, 16)

    def graph(self, rt, x):
        h = conv_bn(rt, x, self.cs(self.c1), self.bn1, ACT_RELU)
        if self.pool_first:
            p = maxpool3x3s2(rt, h)
            q = conv_bn(rt, h, self.cs(self.c2), self.bn2, ACT_NONE)
        else:
            q = conv_bn(rt, h, self.cs(self.c2), self.bn2, ACT_NONE)
            p = maxpool3x3s2(rt, h)
        return add_act(rt, q, p, ACT_RELU)

    def torch_forward(self, xg):
        h = torch.relu(self.bn1(self.c1(xg)))
        return torch.relu(self.bn2(self.c2(h)) + torch.nn.functional.max_pool2d(h, 3, 2, 1))


class AccumulatingAdd(OpsNet):
    """t = materialize(conv_bn(ReLU)) is the identity operand of two adds: u = relu(BN(conv(t)) + t), out = relu(BN(conv(u)) + t).
    In the reversed tape t.grad is set by the second add and ADDED to by the first one's backward (_accum_grad: adamml_bn_act_add
    with null scale and shift), and once more by the data gradient of the conv that reads t."""

    def __init__(self):
        super().__init__()
        self.c0, self.c1, self.c2 = nn.Conv2d(8, 16, 1, bias=False), nn.Conv2d(16, 16, 1, bias=False), nn.Conv2d(16, 16, 1, bias=False)
        self.bn0, self.bn1, self.bn2 = nn.BatchNorm2d(16), nn.BatchNorm2d(16), nn.BatchNorm2d(16)

    def out_shape(self, x):
        return (x.shape[0], self.hw, self.hw, 16)

    def graph(self, rt, x):
        t = materialize(rt, conv_bn(rt, x, self.cs(self.c0), self.bn0, ACT_RELU))
        u = add_act(rt, conv_bn(rt, t, self.cs(self.c1), self.bn1, ACT_NONE), t, ACT_RELU)
        return add_act(rt, conv_bn(rt, u, self.cs(self.c2), self.bn2, ACT_NONE), t, ACT_RELU)

    def torch_forward(self, xg):
        t = torch.relu(self.bn0(self.c0(xg)))
        u = torch.relu(self.bn1(self.c1(t)) + t)
        return torch.relu(self.bn2(self.c2(u)) + t)


# label -> constructor; the rows of tests/test_executor_gpu.py, tests/test_launch_trace_cpu.py and tools/launch_trace.py
ROWS = (
    ("ops-shared-depthwise-input", SharedDepthwiseInput),
    ("ops-alg-gemm-arm", AlgGemmArm),
    ("ops-alg-gemm-arm-fused", lambda: AlgGemmArm(fused=True)),
    ("ops-unfused-maxpool-pool-first", lambda: UnfusedMaxpool(True)),
    ("ops-unfused-maxpool-conv-first", lambda: UnfusedMaxpool(False)),
    ("ops-accumulating-add", AccumulatingAdd),
)


def make(label):
    torch.manual_seed(0)
    return dict(ROWS)[label]()
