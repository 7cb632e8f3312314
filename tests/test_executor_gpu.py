"""The host executor's fused training paths (adamml_amd/runtime.py) against a forced float64 replay of the forward that ran
(tests/executor_ref.py; tests/test_executor_ref_cpu.py shows on the CPU that the bound used here catches seven kinds of executor defect).

Every row drives one forward and one backward of a real model through its own `_run` with the executor entry points recorded, then
  * checks the forward op by op, teacher-forced (each op's float64 result from the recorded inputs against the recorded output),
  * checks every BatchNorm's vectors, running statistics and num_batches_tracked,
  * checks every parameter gradient against  K e_emu + alg_term  (K = 4, shared with the CPU test),
  * asserts a written expectation of the entry points that ran (hip.LaunchProfiler).
Shapes are the smallest that reach the branch (the host-side *_supported / *_streams probes answer without a GPU).
Partial freezes run in two variants (the frozen parameters' gradient buffers kept, or none at all); the forward-only rows (train mode
under no_grad, eval mode) replay the forward alone; the op-level rows drive the graphs of tools/executor_ops.py through the same run_row.
The BasicBlock arm (ResNet-18 / -34: the fused 3x3 residual data gradient and the host decisions around it) has its rows at the end."""
import collections
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from adamml_amd import hip  # noqa: E402
from adamml_amd import runtime  # noqa: E402
from adamml_amd.backbone import run_tape  # noqa: E402
from tests import executor_ref as X  # noqa: E402
from tests import elementwise_ref as E  # noqa: E402
from tests import fused_ref as FR  # noqa: E402
from tests.test_blocks_gpu import randomize  # noqa: E402

DEV = "cuda"


def gen(seed):
    return torch.Generator().manual_seed(seed)


def frames_input(n, hw, c, cpad, seed):
    x = torch.zeros(n, hw, hw, cpad)
    x[..., :c] = torch.randn(n, hw, hw, c, generator=gen(seed))
    return x.to(torch.bfloat16)


def randomize_convs(net, seed):
    """He-scaled weights everywhere (the policy net's own initialisation is fan-out scaled and leaves tiny activations)"""
    g = gen(seed)
    for m in net.modules():
        if isinstance(m, torch.nn.Conv2d):
            fan = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
            m.weight.data = torch.randn(m.weight.shape, generator=g) * (2.0 / fan) ** 0.5
        elif isinstance(m, torch.nn.Linear):
            m.weight.data = torch.randn(m.weight.shape, generator=g) * (1.0 / m.weight.shape[1]) ** 0.5
            m.bias.data = torch.randn(m.bias.shape, generator=g) * 0.1


def cls_of(name, t):
    return "fc" if name.startswith(("fc.", "classifier.")) else "conv" if t.dim() == 4 else "gamma" if name.endswith("weight") else "beta"


def check_forward(rep, net, running=True):
    """the common checks of a replayed forward: every op teacher-forced, the BatchNorm vectors, the undecided share, the running statistics"""
    bad = {i: v for i, v in rep.fwd.items() if not v[1] <= 1.0}
    assert not bad, "teacher-forced forward: %s" % bad
    badv = {i: v for i, v in rep.vec_ratio.items() if not v <= 1.0}
    assert not badv, "BatchNorm vectors: %s" % badv
    assert rep.undecided_share() <= FR.UNDECIDED_CAP
    if not running:
        return 0.0
    stat = 0.0
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d) and id(m) in rep.stat_tol:
            trm, trv = rep.stat_tol[id(m)]
            stat = max(stat, E.vec_ratio(m.running_mean, rep.running[id(m)][0], trm), E.vec_ratio(m.running_var, rep.running[id(m)][1], trv))
            assert int(m.num_batches_tracked) == rep.running[id(m)][2]
    print("  running statistics max err/tol %.3f" % stat)
    assert stat <= 1.0
    return stat


def run_row(net, x, groups, out_cols, monkeypatch, frozen=(), label="", frozen_buffers=True, recomputed_z=False):
    """-> dict: names (Counter of entry points), log ([(entry point, args)]), rep (the float64 replay), res (id -> (err, bound)), ..."""
    t0 = time.time()
    net.to(DEV)
    net.train()
    if not frozen_buffers:                         # frozen BEFORE the gradient views are attached: their .grad is None, as in a real run
        for m in frozen:
            for p in m.parameters():
                p.requires_grad_(False)
    if getattr(net, "flat_owner", None) is not None:
        net.flat_owner.ensure(torch.device(DEV, torch.cuda.current_device()))
        net.flat_owner.ensure_grads()
    else:                                          # (the policy trunk's flat buffers belong to the joint net around it)
        for p in net.parameters():
            p.grad = torch.zeros_like(p) if p.requires_grad else None
    sentinel = {}
    for m in (frozen if frozen_buffers else ()):
        for p in m.parameters():
            p.grad.fill_(0.25)
            sentinel[id(p)] = p.grad               # the buffer itself: must stay bit for bit what it was
            p.requires_grad_(False)
    net.__dict__.pop("_plist", None)
    named = list(net.named_parameters())
    p64, names = X.leaves(named, torch.float64)
    p32, _ = X.leaves(named, torch.float32)
    run0 = X.running_of(net)
    rec = X.Recorder()
    rec.install(monkeypatch)
    log = []
    real_call = runtime.call
    monkeypatch.setattr(runtime, "call", lambda name, *a: (log.append((name, a)), real_call(name, *a))[1])
    x = x.to(DEV)
    rt = net.rt
    rt.capture = {"aux": {}}
    hip.profiler = hip.LaunchProfiler()
    try:
        out, tape = net._run(x, groups, True)
        assert tuple(out.shape) == tuple(out_cols(x)), (out.shape, out_cols(x))
        g = X.bf(torch.randn(tuple(out.shape), generator=gen(77)))
        run_tape(tape, g.to(DEV), net)
        torch.cuda.synchronize()
        counts = collections.Counter(r[0] for r in hip.profiler.records)
    finally:
        hip.profiler = None
        rt.capture = None
    t1 = time.time()
    got = {id(p): p.grad.detach().cpu().clone() for _, p in named if p.requires_grad}
    rep = X.Replay(rec.calls, groups, p64, run0)
    emu = X.Replay(rec.calls, groups, p32, X.running_of(net), dtype=torch.float32, round_grads=True, recomputed_z=recomputed_z)
    if getattr(net, "out_lazy", None) is not None:      # an op-level graph (tools/executor_ops.py): no head, its output is the Lazy it kept
        rep.output_of(net.out_lazy)
        emu.output_of(net.out_lazy)
    ref = rep.backward(g)
    pert = rep.backward_alg(g)
    bnd = X.bounds(ref, emu.backward(g), X.alg_terms(ref, pert))
    res = X.compare(got, ref, bnd)
    t2 = time.time()
    # ---- report (profiles/executor_rows.md is written from these lines)
    print("\nROW %s: hip %.2f s, replay + emulator %.2f s, %d ops" % (label, t1 - t0, t2 - t1, len(rec.calls)))
    print("  entry points:", {k: v for k, v in sorted(counts.items())})
    fw = collections.defaultdict(float)
    for op, r in rep.fwd.values():
        fw[op] = max(fw[op], r)
    print("  forward max err/tol:", {k: round(v, 3) for k, v in fw.items()}, "vectors %.3f" % max(rep.vec_ratio.values()),
          "undecided share %.5f" % rep.undecided_share())
    cls = collections.defaultdict(lambda: [0.0, 0.0, 1.0])
    for k, (e, b) in res.items():
        n = names[k]
        c = cls_of(n, got[k])
        r = e / b if b > 0 else (0.0 if e == 0 else float("inf"))
        cls[c][0] = max(cls[c][0], r)
        cls[c][1] = max(cls[c][1], bnd[k][0])
        cls[c][2] = min(cls[c][2], bnd[k][0])
    print("  worst err/bound per class (e_emu min..max):", {c: "%.3f (%.2e..%.2e)" % (v[0], v[2], v[1]) for c, v in cls.items()})
    # how much of the bound alg_term supplies
    share = collections.defaultdict(float)
    for k, (e, b) in res.items():
        if b > 0:
            share[cls_of(names[k], got[k])] = max(share[cls_of(names[k], got[k])], (b - X.K * bnd[k][0]) / b)
    print("  largest alg_term / bound per class:", {c: round(v, 3) for c, v in share.items()})
    check_forward(rep, net)
    # ---- gradients
    k, wr = X.worst(res)
    print("  worst gradient err/bound %.3f at %s" % (wr, names[k]))
    over = {names[i]: (e, b) for i, (e, b) in res.items() if not e <= b}
    assert not over, "gradients over the bound (err, bound): %s" % over
    for i, buf in sentinel.items():
        p = [q for _, q in named if id(q) == i][0]
        assert p.grad is buf and bool((buf == 0.25).all()), "a frozen parameter's gradient buffer was touched: " + names[i]
    if not frozen_buffers:                         # no algebraic, dual or weight-gradient path was handed (or made) a buffer for them
        assert all(p.grad is None for m in frozen for p in m.parameters())
    return dict(names=counts, log=log, rep=rep, res=res, pnames=names, net=net, ref=ref, got=got, out=out.detach().cpu().clone())


def resnet(frames, depth=50, **kw):
    from adamml_amd.resnet import ResNet
    torch.manual_seed(0)
    net = ResNet(depth, num_frames=frames, num_classes=11, dropout=0.0, **kw)
    randomize(net, 1)
    return net


def resnet_row(net, hw, clips, groups, monkeypatch, label, prepare=None, frozen=(), rows=None, frozen_buffers=True):
    T = net.orig_num_frames
    if prepare is not None:
        prepare(net)
    x = frames_input(groups * clips * T, hw, 3, net.input_cpad(hw, hw), 5)
    return run_row(net, x, groups, lambda xx: (rows or groups * clips, 11), monkeypatch, frozen=frozen(net) if callable(frozen) else frozen, label=label,
                   frozen_buffers=frozen_buffers)


def residual_bwd_channels(r):
    """channel counts of the adamml_residual_bwd launches (its last three arguments are P, C, G)"""
    return [a[-2] for n, a in r["log"] if n == "adamml_residual_bwd"]


def test_resnet50_streaming_forms(monkeypatch):
    """8 frames of 92 x 92, 8 clips in one group: layer 1 is 23 x 23 (33856 pixels per group), layer 2 12 x 12 with 4 frames (4608)."""
    net = resnet(8)
    r = resnet_row(net, 92, 8, 1, monkeypatch, "resnet50-streaming")
    n = r["names"]
    assert n["adamml_conv_fwd_bn_add_next"] == 2 and net.rt.pre_dropped == 0 and net.rt.pre_pending == 0
    assert n["adamml_conv_fwd_bn_add_tpool"] >= 2
    assert n["adamml_temporal_pool_bwd_code_prod"] == 1
    assert n["adamml_conv_bwd_data_res_prod"] >= 1 and n["adamml_conv_bwd_data_res"] >= 1
    assert n["adamml_alg_sumfix"] >= 1
    assert n["adamml_maxpool2d_bwd_bn_apply"] == 1
    assert n["adamml_temporal_pool_fwd"] == 1 and n["adamml_temporal_pool_bwd_res"] == 1      # layer 3 (2 frames): the unfused pool behind add_act
    assert not [c for c in residual_bwd_channels(r) if c in (256, 512)]          # layers 1 and 2 never take the unfused residual backward


def test_resnet50_tile_and_fallback_forms_grouped(monkeypatch):
    """44 x 44, 2 clips of 4 frames per group, 3 groups: spatial sizes 11, 6, 3, 2 -- odd sizes, partial tiles, per-group statistics."""
    net = resnet(4)
    r = resnet_row(net, 44, 2, 3, monkeypatch, "resnet50-tile-g3")
    n = r["names"]
    assert n["adamml_conv_bwd_data_res_prod"] == 0           # refused by its workgroup term
    assert n["adamml_conv_bwd_data_res"] >= 1 and n["adamml_conv_bwd_weight_grouped"] >= 1
    assert n["adamml_conv_fwd_bn_add_tpool"] == 2 and n["adamml_conv_fwd_bn_add_next"] == 2 and net.rt.pre_dropped == 0


def test_resnet50_without_t_stride(monkeypatch):
    net = resnet(4, without_t_stride=True)
    r = resnet_row(net, 44, 2, 1, monkeypatch, "resnet50-without-t-stride")
    n = r["names"]
    assert n["adamml_temporal_pool_fwd"] == 0 and n["adamml_conv_fwd_bn_add_tpool"] == 0
    assert n["adamml_conv_fwd_bn_add"] + n["adamml_conv_fwd_bn_add_next"] == 7 and n["adamml_residual_bwd"] >= 1


def test_resnet50_avg_pooling(monkeypatch):
    """12 frames (avg pooling needs T >= 3 at every stage, as in the reference: 12, 6, 3), one clip"""
    net = resnet(12, pooling_method="avg")
    r = resnet_row(net, 44, 1, 1, monkeypatch, "resnet50-avg", rows=2)      # (3 frames pool to 2, and the head is told 3 // 2 = 1 per clip)
    n = r["names"]
    assert n["adamml_conv_fwd_bn_add_tpool"] == 0 and n["adamml_temporal_pool_fwd"] == 3
    assert n["adamml_temporal_pool_bwd_res"] == 0 and n["adamml_temporal_pool_bwd"] == 3          # the fused form is refused for avg
    assert n["adamml_residual_bwd"] >= 1


def exact_zeros(r):
    """the reference's exact zeros are exact zeros in the result, element by element (a small non-zero value there would pass a rel-L2
    bound) -> the keys of the tensors that are zero as a whole"""
    nz, whole = 0, []
    for k, v in r["ref"].items():
        z = v == 0
        nz += int(z.sum())
        bad = int((r["got"][k][z] != 0).sum())
        assert bad == 0, "%s: %d elements are exact zeros of the reference but not of the result" % (r["pnames"][k], bad)
        if bool(z.all()):
            whole.append(k)
    print("  exact zeros of the reference: %d elements, %d whole tensors" % (nz, len(whole)))
    assert nz > 0
    return whole


def _zero_bn3(net):
    net.layer1[1].bn3.weight.data.zero_()


def _zero_row(net):
    net.layer1[1].conv3.weight.data[5].zero_()


def _cancelling_row(net):
    """channel 9 of layer1.1.conv3 reads eight inputs that are nearly constant and positive (bn2: gamma 0.02, beta 2) with positive
    weights: |mean| / std of its output is in the hundreds -- sum z^2 = diag(W G W^T) cancels against mean^2"""
    b = net.layer1[1]
    b.bn2.weight.data[:8], b.bn2.bias.data[:8] = 0.02, 2.0
    w = b.conv3.weight.data
    w[9] = 0
    w[9, :8] = w[10, :8].abs() + 0.05


@pytest.mark.parametrize("case", ["bn3-gamma-zero", "conv3-zero-row", "conv3-cancelling-row"])
def test_resnet50_edge_parameters(monkeypatch, case):
    net = resnet(4)
    r = resnet_row(net, 44, 2, 3, monkeypatch, "resnet50-edge-" + case,
                   prepare={"bn3-gamma-zero": _zero_bn3, "conv3-zero-row": _zero_row, "conv3-cancelling-row": _cancelling_row}[case])
    zeros = exact_zeros(r)
    bn3 = net.layer1[1].bn3
    vec = [c for c in r["rep"].calls if c.op == "conv_bn_add" and c.args["bn"] is bn3][0].aux[2].detach().cpu().double()
    if case == "conv3-zero-row":
        # channel 5 of conv3 sees no input: z = 0, variance 0, zhat = 0 -- dgamma[5] is an exact zero, invstd[5] = 1 / sqrt(eps) to the three
        # float32 roundings of (eps, var + eps, rsqrt) and the mean exactly 0
        names = {v: k for k, v in r["pnames"].items()}
        assert float(r["ref"][names["layer1.1.bn3.weight"]][5]) == 0.0 and float(r["got"][names["layer1.1.bn3.weight"]][5]) == 0.0
        assert bool((vec[:, 2, 5] == 0).all())
        assert float((vec[:, 3, 5] - 1e-5 ** -0.5).abs().max()) <= 3 * 2.0 ** -23 * 1e-5 ** -0.5, vec[:, 3, 5]
    if case == "bn3-gamma-zero":
        assert {r["pnames"][k] for k in zeros} >= {"layer1.1.conv1.weight", "layer1.1.conv2.weight", "layer1.1.conv3.weight", "layer1.1.bn1.weight",
                                                    "layer1.1.bn2.bias"}
    if case == "conv3-cancelling-row":
        assert float((vec[:, 2, 9].abs() * vec[:, 3, 9]).min()) > 30.0          # |mean| * invstd


@pytest.mark.parametrize("buffers", ["grad-buffers-kept", "grad-none"])
def test_resnet50_partly_frozen(monkeypatch, buffers):
    """requires_grad = False on the stem and layer 1.  grad-buffers-kept: their gradient buffers stay bit for bit what they were;
    grad-none: they have no buffer at all (frozen before the views are attached) and no path asks for one.  The rest meets the bound."""
    net = resnet(4)
    r = resnet_row(net, 44, 2, 3, monkeypatch, "resnet50-frozen-stem-layer1-" + buffers, frozen=lambda n: [n.conv1, n.bn1, n.layer1],
                   frozen_buffers=buffers == "grad-buffers-kept")
    assert not [k for k in r["res"] if r["pnames"][k].startswith(("conv1.", "bn1.", "layer1."))]
    assert any(r["pnames"][k].startswith("layer2.0.") for k in r["res"])
    n = r["names"]
    assert n["adamml_conv_stem_bwd_weight"] == 0
    # layer 1 cannot take conv_bn_add (its conv3 is frozen): conv_bn + add_act + the unfused temporal pool, whose backward finishes the add
    assert n["adamml_temporal_pool_fwd"] == 2 and n["adamml_temporal_pool_bwd_res"] == 1
    assert n["adamml_conv_bwd_data_alg"] == 4 and n["adamml_conv_bwd_data_dual"] == 4


def _mobilenet_expectations(n):
    assert n["adamml_dwconv_bwd_fused"] == 17                        # once per depthwise conv
    assert n["adamml_dwconv_bwd_weight"] == 0 and n["adamml_dwconv_bwd_data"] == 0 and n["adamml_dwconv_bwd_data_bn"] == 0
    assert n["adamml_conv_bwd_data_dual"] >= 17                      # every projection (and the expansions behind a fused depthwise backward)


def sound_net():
    """-> (net, the fp32 [B, G, H, W] input, G, the shape of the logits)"""
    from adamml_amd.sound_mobilenet_v2 import MobileNetV2
    torch.manual_seed(0)
    net = MobileNetV2(num_classes=11, input_channels=1, dropout=0.0)
    randomize_convs(net, 2)
    randomize(net, 3)
    G, B = 2, 4
    return net, torch.randn(B, G, 64, 64, generator=gen(6)), G, (G * B, 11)


def policy_net():
    """-> (net, 2 x 4 clips of 4 bf16 frames 64 x 64, G, the shape of the features)"""
    from adamml_amd.policy_net import MobileNetV2
    torch.manual_seed(0)
    net = MobileNetV2(num_frames=4, input_channels=3)
    randomize_convs(net, 4)
    randomize(net, 5)
    G, clips = 2, 4
    return net, frames_input(G * clips * 4, 64, 3, 8, 7), G, (G * clips * net.out_frames, 1280)


def test_sound_mobilenet_v2(monkeypatch):
    net, x, G, shape = sound_net()
    r = run_row(net, x, G, lambda xx: shape, monkeypatch, label="sound-mobilenetv2-g2")
    assert r["names"]["adamml_conv_stem1_fwd"] == 1
    _mobilenet_expectations(r["names"])


def test_policy_mobilenet_v2(monkeypatch):
    net, x, G, shape = policy_net()
    r = run_row(net, x, G, lambda xx: shape, monkeypatch, label="policy-mobilenetv2-g2")
    assert r["names"]["adamml_temporal_pool_fwd"] == 2 and r["names"]["adamml_temporal_pool_bwd_res"] == 2
    _mobilenet_expectations(r["names"])


def test_eval_vector_cache_follows_raw_pointer_writes(monkeypatch):
    """The eval-mode BatchNorm affines are cached on the modules, keyed on NetRT.state_gen: after a train step (adamml_bn_finalize rewrites
    the running statistics through raw pointers) and after FlatSGD.step() (gamma / beta rewritten the same way) an eval forward must use
    the NEW values -- its recorded affines and every op of its forward are checked against the float64 eval replay of the current state."""
    from adamml_amd.optim import FlatSGD
    net = resnet(4)
    net.to(DEV)
    net.flat_owner.ensure(torch.device(DEV, torch.cuda.current_device()))
    rec = X.Recorder()
    rec.install(monkeypatch)
    x = frames_input(8, 44, 3, net.input_cpad(44, 44), 5).to(DEV)
    net.rt.capture = {"aux": {}}

    def eval_forward(what):
        net.eval()
        rec.calls = []
        with torch.no_grad():
            out, _ = net._run(x, 1, False)
        torch.cuda.synchronize()
        p64, _ = X.leaves(list(net.named_parameters()), torch.float64)
        rep = X.Replay(rec.calls, 1, p64, X.running_of(net), training=False)
        bad = {i: v for i, v in rep.fwd.items() if not v[1] <= 1.0}
        print("eval %s: %d ops, forward max err/tol %.3f, affines %.3f" % (what, len(rec.calls), max(v[1] for v in rep.fwd.values()),
                                                                            max(rep.vec_ratio.values())))
        assert len(rep.vec_ratio) == 53 and max(rep.vec_ratio.values()) <= 1.0, (what, rep.vec_ratio)
        assert not bad, (what, bad)
        assert bool(torch.isfinite(out).all())
        return out.detach().cpu().clone()

    try:
        a = eval_forward("fresh")
        before = net.bn1.running_mean.detach().cpu().clone()
        net.train()
        net.flat_owner.ensure_grads()
        rec.calls = []
        out, tape = net._run(x, 1, True)
        run_tape(tape, X.bf(torch.randn(2, 11, generator=gen(77))).to(DEV), net)
        torch.cuda.synchronize()
        assert not torch.equal(before, net.bn1.running_mean.detach().cpu())
        b = eval_forward("after a train step")
        assert not torch.equal(a, b)
        FlatSGD(net.flat_owner, lr=1e-3).step()         # (a small step: eval mode does not renormalise, a large one overflows bf16 by layer 3)
        assert all(bool(torch.isfinite(p).all()) for p in net.parameters())
        c = eval_forward("after FlatSGD.step")
        assert not torch.equal(b, c)
    finally:
        net.rt.capture = None


# ------------------------------------------------------------------------------------------------- partial freezes of the other models
class Params:
    """a frozen set given as parameters (run_row freezes `.parameters()` of every entry)"""

    def __init__(self, params):
        self.params = list(params)

    def parameters(self):
        return self.params


def depthwise_weights(net):
    return [m.weight for m in net.modules() if isinstance(m, torch.nn.Conv2d) and m.groups > 1]


def all_but(net, params):
    keep = {id(p) for p in params}
    return [p for p in net.parameters() if id(p) not in keep]


def no_frozen_weight_gradient(r):
    """-> the entry points that compute a weight gradient (the fused depthwise backward among them) and ran, with their counts"""
    n = r["names"]
    return {k: v for k, v in n.items() if ("bwd_weight" in k or k in ("adamml_alg_wgrad_combine", "adamml_dwconv_bwd_fused")) and v}


BUFFERS = ["grad-buffers-kept", "grad-none"]


@pytest.mark.parametrize("buffers", BUFFERS)
def test_policy_mobilenet_v2_frozen_depthwise(monkeypatch, buffers):
    """The 17 depthwise weights frozen: no fused depthwise backward (it would write their gradient); the depthwise data gradient still hands
    the expansion its BatchNorm-backward sums (adamml_dwconv_bwd_data_bn)."""
    net, x, G, shape = policy_net()
    r = run_row(net, x, G, lambda xx: shape, monkeypatch, frozen=[Params(depthwise_weights(net))], label="policy-mobilenetv2-frozen-depthwise-" + buffers,
                frozen_buffers=buffers == BUFFERS[0])
    n = r["names"]
    assert n["adamml_dwconv_bwd_fused"] == 0 and n["adamml_dwconv_bwd_data_bn"] == 17 and n["adamml_dwconv_bwd_weight"] == 0
    assert n["adamml_conv_bwd_weight"] == 35 and n["adamml_conv_bwd_data_dual"] == 17
    assert len(r["res"]) == len(list(net.parameters())) - 17


@pytest.mark.parametrize("buffers", BUFFERS)
def test_policy_mobilenet_v2_depthwise_only(monkeypatch, buffers):
    """Only the depthwise weights train.  The first block's depthwise conv reads the stem's output, below which nothing takes a gradient:
    its backward is the unfused weight gradient alone.  The other 16 take the fused backward (their expansions' inputs lead to trainable
    depthwise weights further down).  No dense conv's weight gradient runs."""
    net, x, G, shape = policy_net()
    dw = depthwise_weights(net)
    r = run_row(net, x, G, lambda xx: shape, monkeypatch, frozen=[Params(all_but(net, dw))], label="policy-mobilenetv2-depthwise-only-" + buffers,
                frozen_buffers=buffers == BUFFERS[0])
    n = r["names"]
    assert n["adamml_dwconv_bwd_weight"] >= 1
    assert n["adamml_dwconv_bwd_weight"] + n["adamml_dwconv_bwd_fused"] == 17
    assert set(no_frozen_weight_gradient(r)) <= {"adamml_dwconv_bwd_weight", "adamml_dwconv_bwd_fused"}, no_frozen_weight_gradient(r)
    assert len(r["res"]) == 17 and {r["got"][k].dim() for k in r["res"]} == {4}


@pytest.mark.parametrize("buffers", BUFFERS)
def test_sound_mobilenet_v2_frozen_batchnorm(monkeypatch, buffers):
    """Every 1-D parameter frozen (gamma, beta, the classifier's bias): the BatchNorms still normalise with batch statistics and still
    update running mean / var / num_batches_tracked (run_row's common checks), their backward still carries the mean and variance terms.
    Entry points, written down: the same backward forms as the all-trainable row (the data gradients do not depend on who trains),
    adamml_bn_bwd_finalize[_affine] with null dgamma / dbeta, and no adamml_colsum_f32 (the classifier's bias gradient)."""
    net, x, G, shape = sound_net()
    r = run_row(net, x, G, lambda xx: shape, monkeypatch, frozen=[Params([p for p in net.parameters() if p.dim() == 1])],
                label="sound-mobilenetv2-frozen-batchnorm-" + buffers, frozen_buffers=buffers == BUFFERS[0])
    n = r["names"]
    assert n["adamml_bn_finalize"] == 52 and n["adamml_conv_stem1_fwd"] == 1 and n["adamml_conv_stem1_bwd_weight"] == 1
    assert n["adamml_dwconv_bwd_fused"] == 17 and n["adamml_conv_bwd_data_dual"] == 17 and n["adamml_conv_bwd_weight"] == 34
    assert n["adamml_bn_bwd_finalize"] + n["adamml_bn_bwd_finalize_affine"] == 52
    assert n["adamml_gemm_f32"] == 1 and n["adamml_colsum_f32"] == 0
    # null dgamma / dbeta in every BatchNorm-backward finalize (arguments 6 and 7)
    fin = [a for name, a in r["log"] if name in ("adamml_bn_bwd_finalize", "adamml_bn_bwd_finalize_affine")]
    assert len(fin) == 52 and all(a[6] is None and a[7] is None for a in fin)
    assert {r["got"][k].dim() for k in r["res"]} == {2, 4}


@pytest.mark.parametrize("buffers", BUFFERS)
def test_resnet50_frozen_conv_weights(monkeypatch, buffers):
    """Every 4-D parameter frozen, the BatchNorms and fc train: no weight gradient, no algebraic backward (it exists to save the pass the
    weight gradient needs) and no conv_bn_add in train mode (its backward is the algebraic one): conv_bn + add_act everywhere."""
    net = resnet(4)
    r = resnet_row(net, 44, 2, 1, monkeypatch, "resnet50-frozen-conv-weights-" + buffers,
                   frozen=lambda n: [Params([p for p in n.parameters() if p.dim() == 4])], frozen_buffers=buffers == BUFFERS[0])
    n = r["names"]
    assert not no_frozen_weight_gradient(r), no_frozen_weight_gradient(r)
    assert not [k for k in n if "_bwd_weight" in k] and n["adamml_alg_wgrad_combine"] == 0
    assert n["adamml_gram_colsum"] == 0 and n["adamml_alg_pack"] == 0 and n["adamml_conv_bwd_data_alg"] == 0
    assert n["adamml_conv_fwd_bn_add"] + n["adamml_conv_fwd_bn_add_next"] + n["adamml_conv_fwd_bn_add_tpool"] == 0
    assert n["adamml_conv_fwd"] == 52 and n["adamml_bn_act_add_mask"] == 16 and n["adamml_conv_bwd_data_dual"] == 8
    assert not [k for k in r["res"] if r["got"][k].dim() == 4] and len(r["res"]) == 2 * 53 + 2


# ------------------------------------------------------------------------------------------------------------------- forward-only rows
def forward_only(net, x, groups, monkeypatch, label, training, nbn):
    """One forward under torch.no_grad() with need_grad = False, replayed (no backward) -> (output, Counter of entry points, replay).
    training: net.train() (batch statistics, running statistics updated) or net.eval() (the affines of the running statistics)."""
    t0 = time.time()
    net.to(DEV)
    if getattr(net, "flat_owner", None) is not None:
        net.flat_owner.ensure(torch.device(DEV, torch.cuda.current_device()))
    net.train(training)
    named = list(net.named_parameters())
    p64, _ = X.leaves(named, torch.float64)
    run0 = X.running_of(net)
    entered = []
    with monkeypatch.context() as mp:
        rec = X.Recorder()
        rec.install(mp)
        enter = runtime._on_wgrad_stream.__enter__
        mp.setattr(runtime._on_wgrad_stream, "__enter__", lambda self: (entered.append(1), enter(self))[1])
        log = []
        real_call = runtime.call
        mp.setattr(runtime, "call", lambda name, *a: (log.append((name, a)), real_call(name, *a))[1])
        rt = net.rt
        rt.capture = {"aux": {}}
        hip.profiler = hip.LaunchProfiler()
        try:
            with torch.no_grad():
                out, tape = net._run(x.to(DEV), groups, False)
            torch.cuda.synchronize()
            counts = collections.Counter(r[0] for r in hip.profiler.records)
        finally:
            hip.profiler = None
            rt.capture = None
    t1 = time.time()
    rep = X.Replay(rec.calls, groups, p64, run0, training=training)
    fw = collections.defaultdict(float)
    for op, r in rep.fwd.values():
        fw[op] = max(fw[op], r)
    print("\nROW %s: hip %.2f s, replay %.2f s, %d ops, %d BatchNorm vectors" % (label, t1 - t0, time.time() - t1, len(rec.calls), len(rep.vec_ratio)))
    print("  entry points:", {k: v for k, v in sorted(counts.items())})
    print("  forward max err/tol:", {k: round(v, 3) for k, v in fw.items()}, "vectors %.3f" % max(rep.vec_ratio.values()),
          "undecided share %.5f" % rep.undecided_share())
    assert len(rep.fwd) == len(rec.calls) and len(rep.vec_ratio) == nbn, (len(rep.fwd), len(rec.calls), len(rep.vec_ratio))
    check_forward(rep, net, running=training)
    if training:
        assert len(rep.stat_tol) == nbn
    else:                     # eval mode leaves the running statistics alone
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                assert torch.equal(m.running_mean.cpu().double(), run0[id(m)][0]) and int(m.num_batches_tracked) == run0[id(m)][2]
    assert not [k for k in counts if "_bwd" in k], counts
    assert not entered and not tape.fns
    # nothing was allocated for a backward: no mask of an add (argument 10 / 12), no pool codes or selected-z tensor (last / argument 7)
    where = {"adamml_bn_act_add_mask": 10, "adamml_conv_fwd_bn_add": 12, "adamml_conv_fwd_bn_add_next": 12, "adamml_conv_fwd_bn_add_tpool": 13,
             "adamml_maxpool2d_fwd": 7}
    assert not [(name, a[where[name]]) for name, a in log if name in where and a[where[name]] is not None]
    assert rt.pre_pending == 0 and rt.pre_dropped == 0
    assert bool(torch.isfinite(out).all())
    return out.detach().cpu().clone(), counts, rep


def test_resnet50_train_nograd(monkeypatch):
    """net.train() under torch.no_grad() (tile-g3 shape): conv_bn_add on `conv_bn_add_supported(..., need_grad=False)`, no masks, no codes,
    running statistics updated.  The grad-mode step straight after meets its bound: nothing of the tape state was left behind."""
    net = resnet(4)
    x = frames_input(3 * 2 * 4, 44, 3, net.input_cpad(44, 44), 5)
    out, n, rep = forward_only(net, x, 3, monkeypatch, "resnet50-train-nograd", True, 53)
    assert n["adamml_bn_finalize"] == 53 and n["adamml_gram_stats"] == 7
    assert n["adamml_conv_fwd_bn_add"] + n["adamml_conv_fwd_bn_add_next"] + n["adamml_conv_fwd_bn_add_tpool"] == 7
    r = resnet_row(net, 44, 2, 3, monkeypatch, "resnet50-grad-step-after-train-nograd")
    assert r["names"]["adamml_conv_fwd_bn_add_tpool"] == 2 and net.rt.pre_pending == 0
    print("  no-grad logits == grad-mode logits bit for bit: %s" % torch.equal(out, r["out"]))


def test_policy_mobilenet_v2_train_nograd(monkeypatch):
    net, x, G, shape = policy_net()
    out, n, rep = forward_only(net, x, G, monkeypatch, "policy-mobilenetv2-train-nograd", True, 52)
    assert tuple(out.shape) == shape
    assert n["adamml_bn_finalize"] == 52 and n["adamml_dwconv_fwd"] == 17 and n["adamml_temporal_pool_fwd"] == 2
    assert n["adamml_conv_fwd_bn_add"] == 0           # train mode: the projections are not expanding convs, no Gram-matrix statistics
    r = run_row(net, x, G, lambda xx: shape, monkeypatch, label="policy-mobilenetv2-grad-step-after-train-nograd")
    _mobilenet_expectations(r["names"])
    print("  no-grad features == grad-mode features bit for bit: %s" % torch.equal(out, r["out"]))


def _mobilenet_eval(net, x, G, shape, monkeypatch, label):
    # non-trivial running statistics first (fresh ones make every eval affine (gamma / sqrt(1 + eps), beta)): one train-mode forward
    net.to(DEV)
    if getattr(net, "flat_owner", None) is not None:
        net.flat_owner.ensure(torch.device(DEV, torch.cuda.current_device()))
    net.train()
    with torch.no_grad():
        net._run(x.to(DEV), G, False)
    torch.cuda.synchronize()
    assert all(float(m.running_mean.abs().max()) > 0 for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d))
    out, n, rep = forward_only(net, x, G, monkeypatch, label, False, 52)
    assert tuple(out.shape) == shape
    assert n["adamml_bn_finalize"] == 0 and n["adamml_bn_eval_affine"] == 52
    assert n["adamml_conv_fwd_bn_add"] == 10          # eval mode: every residual block's projection + BatchNorm + add is one kernel
    return n


def test_sound_mobilenet_v2_eval(monkeypatch):
    """the eval forward AdaMML._forward_skipping runs at inference: the fp32 one-channel [B, G, H, W] stem, 52 eval affines"""
    net, x, G, shape = sound_net()
    n = _mobilenet_eval(net, x, G, shape, monkeypatch, "sound-mobilenetv2-eval")
    assert n["adamml_conv_stem1_fwd"] == 1 and n["adamml_head_fwd"] == 1


def test_policy_mobilenet_v2_eval(monkeypatch):
    """bf16 frames, the two temporal pools, 52 eval affines"""
    net, x, G, shape = policy_net()
    n = _mobilenet_eval(net, x, G, shape, monkeypatch, "policy-mobilenetv2-eval")
    assert n["adamml_temporal_pool_fwd"] == 2 and n["adamml_gap_fwd"] == 1


# ----------------------------------------------------------------------------------------------- op-level rows (tools/executor_ops.py)
def ops_row(label, monkeypatch, **kw):
    O = X.ops_module()
    net = O.make(label)
    randomize_convs(net, 8)
    randomize(net, 9)
    x = net.make_input()
    return run_row(net, x, O.GROUPS, net.out_shape, monkeypatch, label=label, **kw)


def launches(r, name):
    return [a for n, a in r["log"] if n == name]


def test_ops_shared_depthwise_input(monkeypatch):
    r = ops_row("ops-shared-depthwise-input", monkeypatch)
    n = r["names"]
    assert n["adamml_dwconv_bwd_weight"] == 1 and n["adamml_act_bwd_from_output"] == 1 and n["adamml_dwconv_bwd_fused"] == 0
    assert [a[-1] for a in launches(r, "adamml_dwconv_bwd_data")] == [1]            # acc = 1: it adds to the gradient already there


@pytest.mark.parametrize("form", ["conv_bn", "conv_bn_add"])
def test_ops_alg_gemm_arm(monkeypatch, form):
    """256 -> 512: the Cin >= ALG_GEMM_CIN arm of _conv1x1_backward_alg at G = 2 (W^T diag(B_g) W and W G_g through adamml_gemm_f32, read back
    as m_pre / wg_pre).  conv_bn_add: adamml_conv_fwd_bn_add_supported admits the descriptor; G comes from the forward."""
    fused = form == "conv_bn_add"
    # conv_bn_add never stores the raw conv output; here nothing hands its BatchNorm backward partial sums, so adamml_residual_bwd reads it
    # as Lazy.recompute writes it, in bf16: a storage point the emulator is told of (the second adamml_conv_fwd is that recomputation)
    r = ops_row("ops-alg-gemm-arm" + ("-fused" if fused else ""), monkeypatch, recomputed_z=fused)
    n = r["names"]
    assert n["adamml_conv_fwd"] == 2 and n["adamml_residual_bwd"] == (1 if fused else 0)
    assert n["adamml_gemm_f32"] == 2 and n["adamml_alg_pack"] == 1 and n["adamml_alg_wgrad_combine"] == 1 and n["adamml_conv_bwd_data_alg"] == 1
    assert [a[2] is not None for a in launches(r, "adamml_alg_pack")] == [True]                    # m_pre
    assert [a[4] is not None for a in launches(r, "adamml_alg_wgrad_combine")] == [True]           # wg_pre
    assert [(a[-3], a[-2], a[-1]) for a in launches(r, "adamml_alg_pack")] == [(512, 256, 2)]
    assert n["adamml_gram_colsum"] == 1 and n["adamml_conv_fwd_bn_add"] == (1 if form == "conv_bn_add" else 0)
    assert len(r["rep"].alg) == 1


@pytest.mark.parametrize("order,acc", [("pool-first", 1), ("conv-first", 0)])
def test_ops_unfused_maxpool(monkeypatch, order, acc):
    r = ops_row("ops-unfused-maxpool-" + order, monkeypatch)
    n = r["names"]
    assert [a[-1] for a in launches(r, "adamml_maxpool2d_bwd")] == [acc] and n["adamml_maxpool2d_bwd_bn_apply"] == 0
    assert [a[-1] for a in launches(r, "adamml_conv_bwd_data")] == [1 - acc]
    # h's gradient is that of its activated value: its own BatchNorm backward applies the ReLU mask (act = 1) in the reduce and apply passes
    assert [a[3] for a in launches(r, "adamml_bn_bwd_reduce")] == [1] and 1 in [a[3] for a in launches(r, "adamml_bn_bwd_apply")]


def test_ops_accumulating_add(monkeypatch):
    r = ops_row("ops-accumulating-add", monkeypatch)
    accum = [a for a in launches(r, "adamml_bn_act_add") if a[1] is None and a[2] is None and a[5] is not None]
    assert len(accum) >= 1 and all(a[0] == a[9] for a in accum)          # in place: t.grad += g
    assert r["names"]["adamml_residual_bwd"] == 2


# ------------------------------------------------------------------------------------- the BasicBlock arm of ResNet._run (ResNet-18 / -34)
# The host decisions around adamml_conv_bwd_data_res on 3x3 convs: which conv is the last consumer of an add output, when _residual_fusable
# hands the add's backward to conv1's epilogue, how the stride-2 conv1 and the stride-2 1x1 downsample share h.grad, the max-pool output as
# layer1.0's identity operand, the temporal pool finishing the last add of a stage.  Same run_row / forward_only, same K, nothing tuned;
# the weights are randomize(net, 1) on the default initialisation, as for ResNet-50.
ABSENT_BASIC = ("adamml_conv_fwd_bn_add", "adamml_alg_", "adamml_gram_", "adamml_conv_bwd_data_dual", "adamml_conv_bwd_data_res_prod")


def residual_dgrads(r):
    """-> [(Cin, H, what adamml_conv_bwd_data_res_streams answers for the logged descriptor)] of the adamml_conv_bwd_data_res launches,
    in forward order (the tape runs them last layer first)"""
    from ctypes import byref
    out = []
    for a in launches(r, "adamml_conv_bwd_data_res"):
        d = a[0]._obj
        assert (d.KH, d.KW, d.stride, d.pad, d.Cin, d.H) == (3, 3, 1, 1, d.Cout, d.W)
        out.append((d.Cin, d.H, hip.load().adamml_conv_bwd_data_res_streams(byref(d))))
    return out[::-1]


def basic_common(r, convs=19):
    """what every grad-mode BasicBlock row launches: one plain forward conv per conv, no Bottleneck-only form"""
    n = r["names"]
    assert not [k for k in n if k.startswith(ABSENT_BASIC)], sorted(n)
    assert n["adamml_conv_fwd"] == convs and n["adamml_conv_stem_fwd"] == 1 and n["adamml_bn_finalize"] == convs + 1
    assert n["adamml_bn_act_add_mask"] == (convs - 3) // 2 and n["adamml_maxpool2d_fwd"] == 1


def bn_vec(r, bn):
    """the recorded [G, 4, C] vectors (scale, shift, mean, invstd) of the conv_bn call that applied the BatchNorm `bn`"""
    return [c for c in r["rep"].calls if c.op == "conv_bn" and c.args["bn"] is bn][0].snap.vec.detach().cpu().double()


def test_resnet18_c64_g3(monkeypatch):
    """44 x 44, 2 clips of 4 frames per group, 3 groups: spatial sizes 11, 6, 3, 2.  The 64-channel 3x3 residual data gradient (layer1.1.conv1
    finishing layer1.0's add) is the resident-weight kernel of conv3x3_c64.hip; layers 1 and 2 end in a temporal pool that finishes their
    last add, layer 3 is left with one frame (an identity pool) and layer 4 has none: their last adds run adamml_residual_bwd."""
    r = resnet_row(resnet(4, depth=18), 44, 2, 3, monkeypatch, "resnet18-c64-g3")
    n = r["names"]
    basic_common(r)
    assert residual_dgrads(r) == [(64, 11, 2), (128, 6, 0), (256, 3, 0), (512, 2, 0)]
    assert residual_bwd_channels(r) == [512, 256]
    assert n["adamml_temporal_pool_fwd"] == 3 and n["adamml_temporal_pool_bwd_res"] == 2 and n["adamml_temporal_pool_bwd"] == 1
    assert n["adamml_conv_bwd_data"] == 7 and n["adamml_conv_bwd_data_bn"] == 8 and n["adamml_conv_bwd_weight"] == 19
    assert n["adamml_maxpool2d_bwd_bn_apply"] == 1 and n["adamml_conv_stem_bwd_weight"] == 1


def test_resnet18_tile_7x7_without_t_stride(monkeypatch):
    """28 x 28, 2 clips of 4 frames per group, 2 groups, no temporal pool: spatial sizes 7, 4, 2, 1 (8 values per channel and group in layer 4).
    64 channels at W = 7 stay with the tile kernel.  Layer 4's stride-1 3x3 convs see 1 x 1 images: eight of their nine taps only ever
    read padding (layer4.0.conv1, stride 2 on 2 x 2: five of nine), and the weight gradient there is an exact zero."""
    r = resnet_row(resnet(4, depth=18, without_t_stride=True), 28, 2, 2, monkeypatch, "resnet18-tile-7x7-no-t-stride")
    basic_common(r)
    assert residual_dgrads(r) == [(64, 7, 0), (128, 4, 0), (256, 2, 0), (512, 1, 0)]
    assert residual_bwd_channels(r) == [512, 256, 128, 64]
    assert not [k for k in r["names"] if "temporal_pool" in k]
    exact_zeros(r)
    by_name = {v: k for k, v in r["pnames"].items()}
    centre = torch.zeros(3, 3, dtype=torch.bool)
    centre[1, 1] = True
    for name in ("layer4.0.conv2.weight", "layer4.1.conv1.weight", "layer4.1.conv2.weight"):
        ref, got = r["ref"][by_name[name]], r["got"][by_name[name]]
        assert bool((ref[:, :, ~centre] == 0).all()) and bool((got[:, :, ~centre] == 0).all()), name
        assert float(ref[:, :, 1, 1].norm()) > 0 and float(got[:, :, 1, 1].norm()) > 0, name
    ref, got = r["ref"][by_name["layer4.0.conv1.weight"]], r["got"][by_name["layer4.0.conv1.weight"]]
    assert bool((ref[:, :, 0] == 0).all() and (ref[:, :, :, 0] == 0).all() and (got[:, :, 0] == 0).all() and (got[:, :, :, 0] == 0).all())


def test_resnet18_avg_pooling(monkeypatch):
    """12 frames (12, 6, 3), one clip: the average pool refuses the fused backward, every stage's last add runs adamml_residual_bwd"""
    r = resnet_row(resnet(12, depth=18, pooling_method="avg"), 44, 1, 1, monkeypatch, "resnet18-avg", rows=2)
    n = r["names"]
    basic_common(r)
    assert n["adamml_temporal_pool_fwd"] == 3 and n["adamml_temporal_pool_bwd"] == 3 and n["adamml_temporal_pool_bwd_res"] == 0
    assert n["adamml_residual_bwd"] == 4 and n["adamml_conv_bwd_data_res"] == 4
    assert [a[7] for a in launches(r, "adamml_temporal_pool_fwd")] == [12, 6, 3]


def test_resnet18_t8_23x23(monkeypatch):
    """8 frames of 92 x 92, 2 clips: layer 1 is 23 x 23 -- the 64-channel kernel takes a 20-row strip and a ragged 3-row strip per image, at an
    odd width -- and every stage pools (8, 4, 2 frames), so three of the four last adds are finished by the pool's backward."""
    r = resnet_row(resnet(8, depth=18), 92, 2, 1, monkeypatch, "resnet18-t8-23x23")
    n = r["names"]
    basic_common(r)
    assert [a[7] for a in launches(r, "adamml_temporal_pool_fwd")] == [8, 4, 2]
    assert residual_dgrads(r) == [(64, 23, 2), (128, 12, 0), (256, 6, 0), (512, 3, 0)]
    assert n["adamml_temporal_pool_bwd_res"] == 3 and n["adamml_temporal_pool_bwd"] == 0 and residual_bwd_channels(r) == [512]


def test_resnet34_g1(monkeypatch):
    """ResNet-34, 44 x 44, 2 clips of 4 frames.  13 blocks have no downsample branch; layer1.0 is one of them, and its conv1 reads the stem's
    max-pool output, which is no residual add: 12 fused residual data gradients, not 13."""
    net = resnet(4, depth=34)
    r = resnet_row(net, 44, 2, 1, monkeypatch, "resnet34-g1")
    n = r["names"]
    basic_common(r, convs=35)
    assert sum(1 for layer in (net.layer1, net.layer2, net.layer3, net.layer4) for b in layer if b.downsample is None) == 13
    assert [(c, h) for c, h, _ in residual_dgrads(r)] == [(64, 11)] * 2 + [(128, 6)] * 3 + [(256, 3)] * 5 + [(512, 2)] * 2
    assert [s for _, _, s in residual_dgrads(r)] == [2] * 2 + [0] * 10
    assert residual_bwd_channels(r) == [512, 256] and n["adamml_bn_finalize"] == 36 and n["adamml_conv_bwd_weight"] == 35
    assert n["adamml_conv_bwd_data_res"] + n["adamml_temporal_pool_bwd_res"] + n["adamml_residual_bwd"] == 16          # every add finished once


def _zero_bn2(net):
    net.layer1[1].bn2.weight.data.zero_()


def _zero_row_conv2(net):
    net.layer1[1].conv2.weight.data[5].zero_()


@pytest.mark.parametrize("case", ["bn2-gamma-zero", "conv2-zero-row"])
def test_resnet18_edge_parameters(monkeypatch, case):
    """bn2-gamma-zero: the zero_init_residual configuration on layer1.1 -- the BatchNorm'd operand of its add has scale 0, nothing flows into
    its residual branch.  conv2-zero-row: channel 5 of layer1.1.conv2 sees no input (z = 0, variance 0)."""
    net = resnet(4, depth=18)
    r = resnet_row(net, 44, 2, 3, monkeypatch, "resnet18-edge-" + case, prepare={"bn2-gamma-zero": _zero_bn2, "conv2-zero-row": _zero_row_conv2}[case])
    basic_common(r)
    assert residual_dgrads(r) == [(64, 11, 2), (128, 6, 0), (256, 3, 0), (512, 2, 0)]
    zeros = exact_zeros(r)
    by_name = {v: k for k, v in r["pnames"].items()}
    if case == "bn2-gamma-zero":
        assert {r["pnames"][k] for k in zeros} >= {"layer1.1.conv1.weight", "layer1.1.conv2.weight", "layer1.1.bn1.weight", "layer1.1.bn1.bias"}
        assert float(r["ref"][by_name["layer1.1.bn2.weight"]].abs().min()) > 0
    else:
        vec = bn_vec(r, net.layer1[1].bn2)
        k = by_name["layer1.1.bn2.weight"]
        assert float(r["ref"][k][5]) == 0.0 and float(r["got"][k][5]) == 0.0
        assert bool((vec[:, 2, 5] == 0).all())
        assert float((vec[:, 3, 5] - 1e-5 ** -0.5).abs().max()) <= 3 * 2.0 ** -23 * 1e-5 ** -0.5, vec[:, 3, 5]


def batchnorm_params(net):
    return [p for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d) for p in m.parameters()]


@pytest.mark.parametrize("buffers", BUFFERS)
def test_resnet18_partly_frozen(monkeypatch, buffers):
    """requires_grad = False on the stem and layer 1 (3 groups): no gradient for them, no stem or layer-1 weight gradient, no stem BatchNorm
    backward behind the max-pool.  (Layer 1's data gradients and BatchNorm backwards still run -- add_act's output always asks for a
    gradient; that is work nobody reads, not a wrong gradient, and the row does not assert it either way.)"""
    r = resnet_row(resnet(4, depth=18), 44, 2, 3, monkeypatch, "resnet18-frozen-stem-layer1-" + buffers, frozen=lambda n: [n.conv1, n.bn1, n.layer1],
                   frozen_buffers=buffers == BUFFERS[0])
    assert not [k for k in r["res"] if r["pnames"][k].startswith(("conv1.", "bn1.", "layer1."))]
    assert any(r["pnames"][k].startswith("layer2.0.") for k in r["res"]) and len(r["res"]) == 62 - 15
    n = r["names"]
    assert not [k for k in n if k.startswith(ABSENT_BASIC)], sorted(n)
    assert n["adamml_conv_stem_bwd_weight"] == 0 and n["adamml_conv_bwd_weight"] == 15 and n["adamml_maxpool2d_bwd_bn_apply"] == 0


@pytest.mark.parametrize("buffers", BUFFERS)
def test_resnet18_frozen_batchnorm(monkeypatch, buffers):
    """Every gamma / beta frozen: every BatchNorm-backward finalize gets null dgamma / dbeta; the fused 3x3 residual data gradients still run,
    and the sums their epilogue accumulates are still needed for dz (the mean and variance terms of the BatchNorm backward)."""
    r = resnet_row(resnet(4, depth=18), 44, 2, 3, monkeypatch, "resnet18-frozen-batchnorm-" + buffers, frozen=lambda n: [Params(batchnorm_params(n))],
                   frozen_buffers=buffers == BUFFERS[0])
    basic_common(r)
    fin = [a for name, a in r["log"] if name in ("adamml_bn_bwd_finalize", "adamml_bn_bwd_finalize_affine")]
    assert len(fin) == 20 and all(a[6] is None and a[7] is None for a in fin)
    assert residual_dgrads(r) == [(64, 11, 2), (128, 6, 0), (256, 3, 0), (512, 2, 0)] and r["names"]["adamml_conv_bwd_weight"] == 19
    assert {r["got"][k].dim() for k in r["res"]} == {1, 2, 4} and len(r["res"]) == 20 + 2         # the convs, fc.weight and fc.bias


@pytest.mark.parametrize("buffers", BUFFERS)
def test_resnet18_frozen_conv_weights(monkeypatch, buffers):
    """Every 4-D parameter frozen, the BatchNorms and fc train: no weight gradient of any kind, the same data gradients"""
    r = resnet_row(resnet(4, depth=18), 44, 2, 3, monkeypatch, "resnet18-frozen-conv-weights-" + buffers,
                   frozen=lambda n: [Params([p for p in n.parameters() if p.dim() == 4])], frozen_buffers=buffers == BUFFERS[0])
    basic_common(r)
    n = r["names"]
    assert not no_frozen_weight_gradient(r), no_frozen_weight_gradient(r)
    assert not [k for k in n if "_bwd_weight" in k]
    assert residual_dgrads(r) == [(64, 11, 2), (128, 6, 0), (256, 3, 0), (512, 2, 0)]
    assert not [k for k in r["res"] if r["got"][k].dim() == 4] and len(r["res"]) == 2 * 20 + 2


def test_resnet18_train_nograd(monkeypatch):
    """net.train() under torch.no_grad() at the c64-g3 shape: 20 BatchNorms finalized, no mask handed to any add, no backward entry point.
    The grad-mode step straight after meets its bound: nothing of the tape state was left behind."""
    net = resnet(4, depth=18)
    x = frames_input(3 * 2 * 4, 44, 3, net.input_cpad(44, 44), 5)
    out, n, rep = forward_only(net, x, 3, monkeypatch, "resnet18-train-nograd", True, 20)
    assert n["adamml_bn_finalize"] == 20 and n["adamml_conv_fwd"] == 19 and n["adamml_bn_act_add_mask"] == 8 and n["adamml_temporal_pool_fwd"] == 3
    assert not [k for k in n if k.startswith(ABSENT_BASIC)], sorted(n)
    r = resnet_row(net, 44, 2, 3, monkeypatch, "resnet18-grad-step-after-train-nograd")
    basic_common(r)
    assert residual_dgrads(r) == [(64, 11, 2), (128, 6, 0), (256, 3, 0), (512, 2, 0)] and net.rt.pre_pending == 0
    print("  no-grad logits == grad-mode logits bit for bit: %s" % torch.equal(out, r["out"]))


def test_resnet18_eval(monkeypatch):
    """eval mode after one train-mode forward (non-trivial running statistics): 20 eval affines, no finalize, the running statistics and
    num_batches_tracked bit for bit what they were"""
    net = resnet(4, depth=18)
    x = frames_input(3 * 2 * 4, 44, 3, net.input_cpad(44, 44), 5)
    net.to(DEV)
    net.flat_owner.ensure(torch.device(DEV, torch.cuda.current_device()))
    net.train()
    with torch.no_grad():
        net._run(x.to(DEV), 3, False)
    torch.cuda.synchronize()
    bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(bns) == 20 and all(float(m.running_mean.abs().max()) > 0 for m in bns)
    before = [(m.running_mean.detach().cpu().clone(), m.running_var.detach().cpu().clone(), int(m.num_batches_tracked)) for m in bns]
    out, n, rep = forward_only(net, x, 3, monkeypatch, "resnet18-eval", False, 20)
    assert tuple(out.shape) == (6, 11)
    assert n["adamml_bn_eval_affine"] == 20 and n["adamml_bn_finalize"] == 0 and n["adamml_conv_fwd"] == 19
    for m, (rm, rv, nb) in zip(bns, before):
        assert torch.equal(m.running_mean.cpu(), rm) and torch.equal(m.running_var.cpu(), rv) and int(m.num_batches_tracked) == nb == 3
