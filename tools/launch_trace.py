"""Host-only launch trace of the executor (adamml_amd/runtime.py): every model row runs its own `_run` and its reverse tape on CPU
tensors with `call` replaced by a logger -- the host logic never reads a tensor value, and the *_supported / *_streams / *_workspace
probes answer without a GPU.  One line per launch: entry point, every argument (a ConvDesc by its sixteen fields, a pointer by the
ordinal of its first appearance, None for a null pointer) and hip.next_meta; a marker line where the weight-gradient stream context
is entered / left.  Two trees issue the same launches exactly when their traces are byte-identical.
Usage: python tools/launch_trace.py [--package DIR] [--out FILE]     (DIR: the tree whose adamml_amd is traced, default: this one)"""
import collections
import contextlib
import hashlib
import os
import sys

import torch


def _resnet(frames, frozen=None, depth=50, **kw):
    from adamml_amd.resnet import ResNet
    net = ResNet(depth, num_frames=frames, num_classes=11, dropout=0.0, **kw)
    return net, ([p for m in frozen(net) for p in m.parameters()] if frozen else [])


def _frames(net, n, hw):
    return torch.zeros(n, hw, hw, net.input_cpad(hw, hw), dtype=torch.bfloat16)


def _mobilenet(which, frozen=None):
    if which == "sound":
        from adamml_amd.sound_mobilenet_v2 import MobileNetV2
        net, x = MobileNetV2(num_classes=11, input_channels=1, dropout=0.0), torch.zeros(4, 2, 64, 64)
    else:
        from adamml_amd.policy_net import MobileNetV2
        net, x = MobileNetV2(num_frames=4, input_channels=3), torch.zeros(2 * 4 * 4, 64, 64, 8, dtype=torch.bfloat16)
    return net, x, (frozen(net) if frozen else [])


def _depthwise_weights(net):
    return [m.weight for m in net.modules() if isinstance(m, torch.nn.Conv2d) and m.groups > 1]


def _all_but(net, params):
    return [p for p in net.parameters() if id(p) not in {id(q) for q in params}]


def _resnet_row(frames, hw, clips, groups, mode="grad", frozen=None, **kw):
    def make():
        net, fz = _resnet(frames, frozen, **kw)
        return net, _frames(net, groups * clips * frames, hw), groups, mode, fz
    return make


def _mobilenet_row(which, mode="grad", frozen=None):
    def make():
        net, x, fz = _mobilenet(which, frozen)
        return net, x, 2, mode, fz
    return make


# the op-level graphs of tools/executor_ops.py (the forms no model's graph produces), defined there once for the GPU test, the CPU test and
# this trace: a depthwise conv sharing its input, the adamml_gemm_f32 arm of the algebraic backward (conv_bn and conv_bn_add), the unfused
# max-pool backward writing / accumulating, the accumulating _accum_grad
_OPS_ROWS = ("ops-shared-depthwise-input", "ops-alg-gemm-arm", "ops-alg-gemm-arm-fused", "ops-unfused-maxpool-pool-first",
             "ops-unfused-maxpool-conv-first", "ops-accumulating-add")


def _executor_ops():
    """tools/executor_ops.py as the module `executor_ops` (loaded from this directory once; the tests load the same file under the same name,
    so the graphs they record and the ones traced here are one module)"""
    mod = sys.modules.get("executor_ops")
    if mod is None:
        import importlib.util
        spec = importlib.util.spec_from_file_location("executor_ops", os.path.join(os.path.dirname(os.path.abspath(__file__)), "executor_ops.py"))
        mod = sys.modules["executor_ops"] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    return mod


def _ops_row(label):
    def make():
        executor_ops = _executor_ops()
        net = executor_ops.make(label)
        return net, torch.zeros_like(net.make_input()), executor_ops.GROUPS, "grad", []
    return make


# label -> () -> (net, input, BatchNorm groups, "grad" | "train-nograd" | "eval", frozen parameters).  Every row is a row of
# tests/test_executor_gpu.py too (same shapes, groups and frozen sets; resnet50-eval is its eval-vector-cache test), where what the launches
# compute is checked; tests/test_launch_trace_cpu.py asserts the same entry-point expectations for both.
ROWS = (
    ("resnet50-streaming", _resnet_row(8, 92, 8, 1)),
    ("resnet50-tile-g3", _resnet_row(4, 44, 2, 3)),
    ("resnet50-without-t-stride", _resnet_row(4, 44, 2, 1, without_t_stride=True)),
    ("resnet50-avg", _resnet_row(12, 44, 1, 1, pooling_method="avg")),
    ("resnet50-frozen-stem-layer1", _resnet_row(4, 44, 2, 3, frozen=lambda n: [n.conv1, n.bn1, n.layer1])),
    ("sound-mobilenetv2-g2", _mobilenet_row("sound")),
    ("policy-mobilenetv2-g2", _mobilenet_row("policy")),
    ("resnet50-train-nograd", _resnet_row(4, 44, 2, 3, mode="train-nograd")),
    ("resnet50-eval", _resnet_row(4, 44, 2, 3, mode="eval")),
    ("policy-mobilenetv2-train-nograd", _mobilenet_row("policy", mode="train-nograd")),
    ("sound-mobilenetv2-eval", _mobilenet_row("sound", mode="eval")),
    ("policy-mobilenetv2-frozen-depthwise", _mobilenet_row("policy", frozen=_depthwise_weights)),
    # only the depthwise weights train: their inputs take no gradient, the unfused depthwise weight gradient runs
    ("policy-mobilenetv2-depthwise-only", _mobilenet_row("policy", frozen=lambda n: _all_but(n, _depthwise_weights(n)))),
    # no BatchNorm trains: its producers' data gradients need no sums, the bare data gradients and the unfused activation mask run
    ("sound-mobilenetv2-frozen-batchnorm", _mobilenet_row("sound", frozen=lambda n: [p for p in n.parameters() if p.dim() == 1])),
    ("resnet50-frozen-conv-weights", _resnet_row(4, 44, 2, 1, frozen=lambda n: [_W([p for p in n.parameters() if p.dim() == 4])])),
    ("policy-mobilenetv2-eval", _mobilenet_row("policy", mode="eval")),
) + tuple((label, _ops_row(label)) for label in _OPS_ROWS) + (
    # the BasicBlock arm of ResNet._run (appended: a pointer's ordinal counts from the first row, so the lines of the rows above stay as they
    # were).  ResNet-18 at 44 x 44 has spatial sizes 11, 6, 3, 2: the 64-channel 3x3 residual data gradient is the resident-weight kernel
    ("resnet18-c64-g3", _resnet_row(4, 44, 2, 3, depth=18)),
    # 28 x 28: 7, 4, 2, 1 -- 64 channels at W = 7 stay with the tile kernel; layer 4 runs its 3x3 convs on 1 x 1 images
    ("resnet18-tile-7x7-no-t-stride", _resnet_row(4, 28, 2, 2, depth=18, without_t_stride=True)),
    ("resnet18-avg", _resnet_row(12, 44, 1, 1, depth=18, pooling_method="avg")),
    # 92 x 92: layer 1 is 23 x 23 (a 20-row strip and a ragged 3-row strip per image, odd width), pools over 8, 4 and 2 frames
    ("resnet18-t8-23x23", _resnet_row(8, 92, 2, 1, depth=18)),
    ("resnet34-g1", _resnet_row(4, 44, 2, 1, depth=34)),
    ("resnet18-frozen-stem-layer1", _resnet_row(4, 44, 2, 3, depth=18, frozen=lambda n: [n.conv1, n.bn1, n.layer1])),
    ("resnet18-frozen-batchnorm", _resnet_row(4, 44, 2, 3, depth=18, frozen=lambda n: [_W([p for m in n.modules() if isinstance(m, torch.nn.BatchNorm2d)
                                                                                           for p in m.parameters()])])),
    ("resnet18-frozen-conv-weights", _resnet_row(4, 44, 2, 3, depth=18, frozen=lambda n: [_W([p for p in n.parameters() if p.dim() == 4])])),
    ("resnet18-train-nograd", _resnet_row(4, 44, 2, 3, depth=18, mode="train-nograd")),
    ("resnet18-eval", _resnet_row(4, 44, 2, 3, depth=18, mode="eval")),
)


class _W:
    def __init__(self, params):
        self.params = params

    def parameters(self):
        return self.params


SITES = None        # --sites: a set collecting (file, line) of every statement that launched


class _Ptr(int):
    """what the replaced `ptr` returns: an address the logger turns into an ordinal"""


class Row:
    __slots__ = ("label", "net", "log", "lines", "counts")


@contextlib.contextmanager
def _patched(log):
    """`call`, `ptr` and hip._stream replaced in every loaded adamml_amd module; the weight-gradient stream context writes markers"""
    from adamml_amd import hip, runtime
    ids, keep = {}, []                  # ordinal by first appearance in a launch; every tensor stays alive, so no address is reused

    def ptr(t):
        keep.append(t)
        return None if t is None else _Ptr(t.data_ptr())

    def norm(a):
        if isinstance(a, _Ptr):
            return "p%d" % ids.setdefault(int(a), len(ids))
        d = getattr(a, "_obj", None)
        return tuple(getattr(d, f[0]) for f in d._fields_) if isinstance(d, hip.ConvDesc) else a

    def call(name, *args):
        if SITES is not None:
            SITES.add((os.path.basename(sys._getframe(1).f_code.co_filename), sys._getframe(1).f_lineno))
        log.append((name, tuple(norm(a) for a in args), hip.next_meta))
        hip.next_meta = (0.0, 0.0)              # (as under hip.LaunchProfiler: a launch shows the meta written FOR it)

    def marker(name, real):
        def method(self, *a):
            log.append((name, tuple(norm(ptr(t)) for t in self.tensors), None))
            return real(self, *a)
        return method

    mods = [m for n, m in list(sys.modules.items()) if m is not None and (n == "adamml_amd" or n.startswith("adamml_amd."))]
    saved = [(m, n, getattr(m, n)) for m in mods for n, real in (("call", hip.call), ("ptr", hip.ptr)) if getattr(m, n, None) is real]
    ws = runtime._on_wgrad_stream
    saved += [(hip, "_stream", hip._stream), (ws, "__enter__", ws.__enter__), (ws, "__exit__", ws.__exit__), (hip, "_wgrad_ws", hip._wgrad_ws)]
    try:
        for m, n, _ in saved[:-4]:
            setattr(m, n, call if n == "call" else ptr)
        hip._stream = lambda: 0
        hip._wgrad_ws = {}                      # (a scratch buffer grown by an earlier run would change the workspace sizes passed)
        hip.next_meta = (0.0, 0.0)              # (the meta an earlier, unprofiled launch of the process left behind would show on the first line)
        ws.__enter__, ws.__exit__ = marker("wgrad_stream_enter", ws.__enter__), marker("wgrad_stream_exit", ws.__exit__)
        yield
    finally:
        for m, n, v in saved:
            setattr(m, n, v)


def trace(rows=ROWS):
    """-> [Row]: the launches of every row, in order"""
    import adamml_amd.resnet, adamml_amd.sound_mobilenet_v2, adamml_amd.policy_net  # noqa: F401,E401  (loaded before `call` is replaced)
    log, out = [], []
    with _patched(log):
        for label, make in rows:
            torch.manual_seed(0)
            net, x, groups, mode, frozen = make()
            for p in frozen:
                p.requires_grad_(False)
            n0 = len(log)
            net.train(mode != "eval")
            if mode == "grad":
                for p in net.parameters():
                    p.grad = torch.zeros_like(p) if p.requires_grad else None
                y, tape = net._run(x, groups, True)
                net.rt.bwd_arena.reset(x.device)
                tape.grad_out = torch.zeros(tuple(y.shape))
                tape.backward()
            else:
                with torch.no_grad():
                    net._run(x, groups, False)
            r = Row()
            r.label, r.net, r.log = label, net, log[n0:]
            r.lines = ["%s %r %r" % e for e in r.log]
            r.counts = collections.Counter(e[0] for e in r.log if e[2] is not None)
            out.append(r)
    return out


def digest(rows):
    return hashlib.sha256("".join(ln + "\n" for r in rows for ln in ["# " + r.label] + r.lines).encode()).hexdigest()


def main(argv):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if "--package" in argv:
        root = os.path.abspath(argv[argv.index("--package") + 1])
    sys.path.insert(0, root)
    if "--sites" in argv:
        globals()["SITES"] = set()
    rows = trace()
    if SITES is not None:
        # the `call(...)` statements of runtime.py no row reached (a launch is reported at a line of the statement's own span)
        import ast
        src = open(os.path.join(root, "adamml_amd", "runtime.py")).read()
        hit = {ln for f, ln in SITES if f == "runtime.py"}
        for node in sorted((n for n in ast.walk(ast.parse(src)) if isinstance(n, ast.Call)), key=lambda n: n.lineno):
            if isinstance(node, ast.Call) and getattr(node.func, "id", None) == "call" and not hit & set(range(node.lineno, node.end_lineno + 1)):
                print("unreached runtime.py:%d %s" % (node.lineno, src.split("\n")[node.lineno - 1].strip()[:100]))
    for r in rows:
        print("%-40s %5d launches, %2d entry points, %s" % (r.label, sum(r.counts.values()), len(r.counts), digest([r])[:16]))
    total = collections.Counter()
    for r in rows:
        total += r.counts
    print("all rows: %d launches, %d entry points" % (sum(total.values()), len(total)))
    print("sha256 %s" % digest(rows))
    if "--out" in argv:
        with open(argv[argv.index("--out") + 1], "w") as f:
            f.writelines(ln + "\n" for r in rows for ln in ["# " + r.label] + r.lines)


if __name__ == "__main__":
    main(sys.argv[1:])
