"""What the host executor (adamml_amd/runtime.py) launches, checked without a GPU: tools/launch_trace.py runs the models' own `_run`
and reverse tape on CPU tensors with every C-ABI launch logged instead of issued (the host logic never reads a tensor value; the
dispatch probes are host functions of the built library).  Two runs give the same trace line for line, and the entry-point expectations
tests/test_executor_gpu.py writes down for its rows hold for the same rows here."""
import importlib.util
import os

import pytest

import __graft_entry__ as ge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    ge.build()
    return ge.LIB


@pytest.fixture(scope="module")
def runs(built):
    spec = importlib.util.spec_from_file_location("launch_trace", os.path.join(ROOT, "tools", "launch_trace.py"))
    lt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lt)
    return lt, lt.trace(), lt.trace()


@pytest.fixture(scope="module")
def rows(runs):
    return {r.label: r for r in runs[1]}


def test_two_runs_give_the_same_trace(runs):
    lt, a, b = runs
    assert [r.label for r in a] == [label for label, _ in lt.ROWS] and len(set(r.label for r in a)) == len(a)
    for ra, rb in zip(a, b):
        assert ra.lines == rb.lines, ra.label
        assert sum(ra.counts.values()) > 0
    assert lt.digest(a) == lt.digest(b)
    # nothing address-like reaches a line: pointers are ordinals, everything else a scalar of the call
    assert not [ln for r in a for ln in r.lines if "data_ptr" in ln or " 0x" in ln]


def test_the_patches_are_undone(runs):
    from adamml_amd import hip, runtime
    assert runtime.call is hip.call and runtime.ptr is hip.ptr and hip.call.__module__ == "adamml_amd.hip"
    assert runtime._on_wgrad_stream.__enter__.__qualname__ == "_on_wgrad_stream.__enter__"


def residual_bwd_channels(r):
    """channel counts of the adamml_residual_bwd launches (its last three arguments are P, C, G)"""
    return [a[-2] for n, a, _ in r.log if n == "adamml_residual_bwd"]


def test_resnet50_streaming_forms(rows):
    r = rows["resnet50-streaming"]
    n = r.counts
    assert n["adamml_conv_fwd_bn_add_next"] == 2 and r.net.rt.pre_dropped == 0 and r.net.rt.pre_pending == 0
    assert n["adamml_conv_fwd_bn_add_tpool"] >= 2
    assert n["adamml_temporal_pool_bwd_code_prod"] == 1
    assert n["adamml_conv_bwd_data_res_prod"] >= 1 and n["adamml_conv_bwd_data_res"] >= 1
    assert n["adamml_alg_sumfix"] >= 1
    assert n["adamml_maxpool2d_bwd_bn_apply"] == 1
    assert n["adamml_temporal_pool_fwd"] == 1 and n["adamml_temporal_pool_bwd_res"] == 1
    assert not [c for c in residual_bwd_channels(r) if c in (256, 512)]


def test_resnet50_tile_and_fallback_forms_grouped(rows):
    r = rows["resnet50-tile-g3"]
    n = r.counts
    assert n["adamml_conv_bwd_data_res_prod"] == 0
    assert n["adamml_conv_bwd_data_res"] >= 1 and n["adamml_conv_bwd_weight_grouped"] >= 1
    assert n["adamml_conv_fwd_bn_add_tpool"] == 2 and n["adamml_conv_fwd_bn_add_next"] == 2 and r.net.rt.pre_dropped == 0


def test_resnet50_without_t_stride(rows):
    n = rows["resnet50-without-t-stride"].counts
    assert n["adamml_temporal_pool_fwd"] == 0 and n["adamml_conv_fwd_bn_add_tpool"] == 0
    assert n["adamml_conv_fwd_bn_add"] + n["adamml_conv_fwd_bn_add_next"] == 7 and n["adamml_residual_bwd"] >= 1


def test_resnet50_avg_pooling(rows):
    n = rows["resnet50-avg"].counts
    assert n["adamml_conv_fwd_bn_add_tpool"] == 0 and n["adamml_temporal_pool_fwd"] == 3
    assert n["adamml_temporal_pool_bwd_res"] == 0 and n["adamml_temporal_pool_bwd"] == 3
    assert n["adamml_residual_bwd"] >= 1


def test_resnet50_partly_frozen(rows):
    n = rows["resnet50-frozen-stem-layer1"].counts
    assert n["adamml_conv_stem_bwd_weight"] == 0
    assert n["adamml_temporal_pool_fwd"] == 2 and n["adamml_temporal_pool_bwd_res"] == 1
    assert n["adamml_conv_bwd_data_alg"] == 4 and n["adamml_conv_bwd_data_dual"] == 4


def _mobilenet_expectations(n):
    assert n["adamml_dwconv_bwd_fused"] == 17
    assert n["adamml_dwconv_bwd_weight"] == 0 and n["adamml_dwconv_bwd_data"] == 0 and n["adamml_dwconv_bwd_data_bn"] == 0
    assert n["adamml_conv_bwd_data_dual"] >= 17


def test_sound_mobilenet_v2(rows):
    n = rows["sound-mobilenetv2-g2"].counts
    assert n["adamml_conv_stem1_fwd"] == 1
    _mobilenet_expectations(n)


def test_policy_mobilenet_v2(rows):
    n = rows["policy-mobilenetv2-g2"].counts
    assert n["adamml_temporal_pool_fwd"] == 2 and n["adamml_temporal_pool_bwd_res"] == 2
    _mobilenet_expectations(n)


def test_forward_only_rows_launch_no_backward(rows):
    for label in ("resnet50-train-nograd", "resnet50-eval", "policy-mobilenetv2-train-nograd", "sound-mobilenetv2-eval", "policy-mobilenetv2-eval"):
        r = rows[label]
        assert not [n for n in r.counts if "_bwd" in n], label
        assert not [e for e in r.log if e[2] is None], label            # no weight-gradient stream marker either
        assert r.net.rt.pre_pending == 0 and r.net.rt.pre_dropped == 0
    assert rows["resnet50-eval"].counts["adamml_bn_finalize"] == 0 and rows["resnet50-train-nograd"].counts["adamml_bn_finalize"] == 53
    n = rows["resnet50-train-nograd"].counts
    assert n["adamml_gram_stats"] == 7 and n["adamml_conv_fwd_bn_add"] + n["adamml_conv_fwd_bn_add_next"] + n["adamml_conv_fwd_bn_add_tpool"] == 7
    n = rows["policy-mobilenetv2-train-nograd"].counts
    assert n["adamml_bn_finalize"] == 52 and n["adamml_dwconv_fwd"] == 17 and n["adamml_temporal_pool_fwd"] == 2 and n["adamml_conv_fwd_bn_add"] == 0
    for label in ("sound-mobilenetv2-eval", "policy-mobilenetv2-eval"):
        n = rows[label].counts
        assert n["adamml_bn_finalize"] == 0 and n["adamml_bn_eval_affine"] == 52 and n["adamml_conv_fwd_bn_add"] == 10, label
    n = rows["sound-mobilenetv2-eval"].counts
    assert n["adamml_conv_stem1_fwd"] == 1 and n["adamml_head_fwd"] == 1
    n = rows["policy-mobilenetv2-eval"].counts
    assert n["adamml_temporal_pool_fwd"] == 2 and n["adamml_gap_fwd"] == 1


def test_unfused_depthwise_forms(rows):
    """frozen depthwise weights: no fused depthwise backward, the data gradient still produces the expansion's sums; a depthwise conv that
    shares its input (no model has one) takes the unfused weight gradient and the accumulating data gradient"""
    n = rows["policy-mobilenetv2-frozen-depthwise"].counts
    assert n["adamml_dwconv_bwd_fused"] == 0 and n["adamml_dwconv_bwd_data_bn"] == 17 and n["adamml_dwconv_bwd_weight"] == 0
    r = rows["ops-shared-depthwise-input"]
    assert r.counts["adamml_dwconv_bwd_weight"] == 1 and r.counts["adamml_act_bwd_from_output"] == 1
    assert [a[-1] for n_, a, _ in r.log if n_ == "adamml_dwconv_bwd_data"] == [1]            # acc = 1: it adds to the gradient already there


def weight_gradient_launches(n):
    return {k: v for k, v in n.items() if ("bwd_weight" in k or k in ("adamml_alg_wgrad_combine", "adamml_dwconv_bwd_fused")) and v}


def launches(r, name):
    return [a for n, a, m in r.log if n == name and m is not None]


def test_policy_mobilenet_v2_frozen_depthwise(rows):
    """frozen depthwise weights: no fused depthwise backward, the data gradient still produces the expansion's sums"""
    n = rows["policy-mobilenetv2-frozen-depthwise"].counts
    assert n["adamml_dwconv_bwd_fused"] == 0 and n["adamml_dwconv_bwd_data_bn"] == 17 and n["adamml_dwconv_bwd_weight"] == 0
    assert n["adamml_conv_bwd_weight"] == 35 and n["adamml_conv_bwd_data_dual"] == 17


def test_policy_mobilenet_v2_depthwise_only(rows):
    n = rows["policy-mobilenetv2-depthwise-only"].counts
    assert n["adamml_dwconv_bwd_weight"] >= 1
    assert n["adamml_dwconv_bwd_weight"] + n["adamml_dwconv_bwd_fused"] == 17
    assert set(weight_gradient_launches(n)) <= {"adamml_dwconv_bwd_weight", "adamml_dwconv_bwd_fused"}


def test_sound_mobilenet_v2_frozen_batchnorm(rows):
    r = rows["sound-mobilenetv2-frozen-batchnorm"]
    n = r.counts
    assert n["adamml_bn_finalize"] == 52 and n["adamml_conv_stem1_fwd"] == 1 and n["adamml_conv_stem1_bwd_weight"] == 1
    assert n["adamml_dwconv_bwd_fused"] == 17 and n["adamml_conv_bwd_data_dual"] == 17 and n["adamml_conv_bwd_weight"] == 34
    assert n["adamml_bn_bwd_finalize"] + n["adamml_bn_bwd_finalize_affine"] == 52
    assert n["adamml_gemm_f32"] == 1 and n["adamml_colsum_f32"] == 0
    fin = launches(r, "adamml_bn_bwd_finalize") + launches(r, "adamml_bn_bwd_finalize_affine")
    assert len(fin) == 52 and all(a[6] is None and a[7] is None for a in fin)


def test_resnet50_frozen_conv_weights(rows):
    n = rows["resnet50-frozen-conv-weights"].counts
    assert not weight_gradient_launches(n)
    assert not [k for k in n if "_bwd_weight" in k] and n["adamml_alg_wgrad_combine"] == 0
    assert n["adamml_gram_colsum"] == 0 and n["adamml_alg_pack"] == 0 and n["adamml_conv_bwd_data_alg"] == 0
    assert n["adamml_conv_fwd_bn_add"] + n["adamml_conv_fwd_bn_add_next"] + n["adamml_conv_fwd_bn_add_tpool"] == 0
    assert n["adamml_conv_fwd"] == 52 and n["adamml_bn_act_add_mask"] == 16 and n["adamml_conv_bwd_data_dual"] == 8


def test_ops_shared_depthwise_input(rows):
    """a depthwise conv that shares its input (no model has one) takes the unfused weight gradient and the accumulating data gradient"""
    r = rows["ops-shared-depthwise-input"]
    n = r.counts
    assert n["adamml_dwconv_bwd_weight"] == 1 and n["adamml_act_bwd_from_output"] == 1 and n["adamml_dwconv_bwd_fused"] == 0
    assert [a[-1] for a in launches(r, "adamml_dwconv_bwd_data")] == [1]            # acc = 1: it adds to the gradient already there


@pytest.mark.parametrize("form", ["conv_bn", "conv_bn_add"])
def test_ops_alg_gemm_arm(rows, form):
    r = rows["ops-alg-gemm-arm" + ("-fused" if form == "conv_bn_add" else "")]
    n = r.counts
    assert n["adamml_gemm_f32"] == 2 and n["adamml_alg_pack"] == 1 and n["adamml_alg_wgrad_combine"] == 1 and n["adamml_conv_bwd_data_alg"] == 1
    assert [a[2] is not None for a in launches(r, "adamml_alg_pack")] == [True]                    # m_pre
    assert [a[4] is not None for a in launches(r, "adamml_alg_wgrad_combine")] == [True]           # wg_pre
    assert [(a[-3], a[-2], a[-1]) for a in launches(r, "adamml_alg_pack")] == [(512, 256, 2)]
    assert n["adamml_gram_colsum"] == 1 and n["adamml_conv_fwd_bn_add"] == (1 if form == "conv_bn_add" else 0)


@pytest.mark.parametrize("order,acc", [("pool-first", 1), ("conv-first", 0)])
def test_ops_unfused_maxpool(rows, order, acc):
    r = rows["ops-unfused-maxpool-" + order]
    assert [a[-1] for a in launches(r, "adamml_maxpool2d_bwd")] == [acc] and r.counts["adamml_maxpool2d_bwd_bn_apply"] == 0
    assert [a[-1] for a in launches(r, "adamml_conv_bwd_data")] == [1 - acc]
    assert [a[3] for a in launches(r, "adamml_bn_bwd_reduce")] == [1] and 1 in [a[3] for a in launches(r, "adamml_bn_bwd_apply")]


def test_ops_accumulating_add(rows):
    r = rows["ops-accumulating-add"]
    accum = [a for a in launches(r, "adamml_bn_act_add") if a[1] is None and a[2] is None and a[5] is not None]
    assert len(accum) >= 1 and all(a[0] == a[9] for a in accum)          # in place: t.grad += g
    assert r.counts["adamml_residual_bwd"] == 2


def test_a_step_leaves_nothing_to_the_cycle_collector(runs):
    """The activations of a step are freed by reference counting when the step ends: a Lazy (or a backward record holding one) that sits in a
    reference cycle keeps gigabytes alive until the cycle collector happens to run, and the next steps run out of memory."""
    import gc
    lt = runs[0]
    gc.collect()
    flags = gc.get_debug()
    gc.set_debug(gc.DEBUG_SAVEALL)
    try:
        r = lt.trace(lt.ROWS[1:2] + lt.ROWS[5:6])            # a ResNet-50 row (conv_bn_add, fused pool) and a MobileNetV2 row
        del r
        gc.collect()
        left = sorted({type(o).__name__ for o in gc.garbage if type(o).__module__ == "adamml_amd.runtime"}
                      - {"NetRT", "Arena", "SyncCtx", "ConvState", "Tape"})       # (a model and what it owns are one cycle, freed with it)
    finally:
        gc.set_debug(flags)
        del gc.garbage[:]
    assert not left, left


# ------------------------------------------------------------------------------------------- the BasicBlock arm (ResNet-18 / -34 rows)
ABSENT_BASIC = ("adamml_conv_fwd_bn_add", "adamml_alg_", "adamml_gram_", "adamml_conv_bwd_data_dual", "adamml_conv_bwd_data_res_prod")


def residual_dgrads(r):
    """-> [(Cin, H, what adamml_conv_bwd_data_res_streams answers for the logged descriptor)] of the adamml_conv_bwd_data_res launches,
    in forward order (the tape runs them last layer first)"""
    from ctypes import byref
    from adamml_amd import hip
    out = []
    for a in launches(r, "adamml_conv_bwd_data_res"):
        d = hip.ConvDesc(*a[0])
        assert (d.KH, d.KW, d.stride, d.pad, d.Cin, d.H) == (3, 3, 1, 1, d.Cout, d.W), a[0]
        out.append((d.Cin, d.H, hip.load().adamml_conv_bwd_data_res_streams(byref(d))))
    return out[::-1]


def basic_common(r, convs=19):
    """what every grad-mode BasicBlock row launches: one plain forward conv and one weight gradient per conv, no Bottleneck-only form"""
    n = r.counts
    assert not [k for k in n if k.startswith(ABSENT_BASIC)], sorted(n)
    assert n["adamml_conv_fwd"] == convs and n["adamml_conv_stem_fwd"] == 1 and n["adamml_bn_finalize"] == convs + 1
    assert n["adamml_bn_act_add_mask"] == (convs - 3) // 2 and n["adamml_maxpool2d_fwd"] == 1


def test_resnet18_c64_g3(rows):
    r = rows["resnet18-c64-g3"]
    n = r.counts
    basic_common(r)
    assert residual_dgrads(r) == [(64, 11, 2), (128, 6, 0), (256, 3, 0), (512, 2, 0)]          # 2: the resident-weight kernel of conv3x3_c64.hip
    assert residual_bwd_channels(r) == [512, 256]
    assert n["adamml_temporal_pool_fwd"] == 3 and n["adamml_temporal_pool_bwd_res"] == 2 and n["adamml_temporal_pool_bwd"] == 1
    assert n["adamml_conv_bwd_data"] == 7 and n["adamml_conv_bwd_data_bn"] == 8 and n["adamml_conv_bwd_weight"] == 19
    assert n["adamml_maxpool2d_bwd_bn_apply"] == 1 and n["adamml_conv_stem_bwd_weight"] == 1


def test_resnet18_tile_7x7_without_t_stride(rows):
    r = rows["resnet18-tile-7x7-no-t-stride"]
    basic_common(r)
    assert residual_dgrads(r) == [(64, 7, 0), (128, 4, 0), (256, 2, 0), (512, 1, 0)]           # W = 7 < 8: the tile kernel
    assert residual_bwd_channels(r) == [512, 256, 128, 64]
    assert not [k for k in r.counts if "temporal_pool" in k]


def test_resnet18_avg_pooling(rows):
    r = rows["resnet18-avg"]
    n = r.counts
    basic_common(r)
    assert n["adamml_temporal_pool_fwd"] == 3 and n["adamml_temporal_pool_bwd"] == 3 and n["adamml_temporal_pool_bwd_res"] == 0
    assert n["adamml_residual_bwd"] == 4 and n["adamml_conv_bwd_data_res"] == 4
    assert [a[7] for a in launches(r, "adamml_temporal_pool_fwd")] == [12, 6, 3]


def test_resnet18_t8_23x23(rows):
    r = rows["resnet18-t8-23x23"]
    n = r.counts
    basic_common(r)
    assert [a[7] for a in launches(r, "adamml_temporal_pool_fwd")] == [8, 4, 2]
    assert residual_dgrads(r) == [(64, 23, 2), (128, 12, 0), (256, 6, 0), (512, 3, 0)]
    assert n["adamml_temporal_pool_bwd_res"] == 3 and n["adamml_temporal_pool_bwd"] == 0 and residual_bwd_channels(r) == [512]


def test_resnet34_g1(rows):
    r = rows["resnet34-g1"]
    n = r.counts
    basic_common(r, convs=35)
    # 13 blocks have no downsample branch; layer1.0 is one of them, and its conv1 reads the max-pool output (no residual add to finish): 12
    assert sum(1 for l in (r.net.layer1, r.net.layer2, r.net.layer3, r.net.layer4) for b in l if b.downsample is None) == 13
    assert [(c, h) for c, h, _ in residual_dgrads(r)] == [(64, 11)] * 2 + [(128, 6)] * 3 + [(256, 3)] * 5 + [(512, 2)] * 2
    assert [s for _, _, s in residual_dgrads(r)] == [2] * 2 + [0] * 10
    assert residual_bwd_channels(r) == [512, 256] and n["adamml_bn_finalize"] == 36 and n["adamml_conv_bwd_weight"] == 35
    assert n["adamml_conv_bwd_data_res"] + n["adamml_temporal_pool_bwd_res"] + n["adamml_residual_bwd"] == 16          # every add finished once


def test_resnet18_partly_frozen(rows):
    n = rows["resnet18-frozen-stem-layer1"].counts
    assert n["adamml_conv_stem_bwd_weight"] == 0 and n["adamml_conv_bwd_weight"] == 15 and n["adamml_maxpool2d_bwd_bn_apply"] == 0
    r = rows["resnet18-frozen-batchnorm"]
    fin = [a for name, a, m in r.log if name.startswith("adamml_bn_bwd_finalize") and m is not None]
    assert len(fin) == 20 and all(a[6] is None and a[7] is None for a in fin)
    assert r.counts["adamml_conv_bwd_data_res"] == 4 and r.counts["adamml_conv_bwd_weight"] == 19
    n = rows["resnet18-frozen-conv-weights"].counts
    assert not weight_gradient_launches(n) and not [k for k in n if "_bwd_weight" in k]
    assert n["adamml_conv_bwd_data_res"] == 4
    for label in ("resnet18-frozen-stem-layer1", "resnet18-frozen-batchnorm", "resnet18-frozen-conv-weights"):
        assert not [k for k in rows[label].counts if k.startswith(ABSENT_BASIC)], label


def test_resnet18_forward_only_rows(rows):
    for label in ("resnet18-train-nograd", "resnet18-eval"):
        r = rows[label]
        assert not [k for k in r.counts if "_bwd" in k], label
        assert not [e for e in r.log if e[2] is None], label
        assert [a[10] for a in launches(r, "adamml_bn_act_add_mask")] == [None] * 8, label          # no mask handed to any add
        assert r.net.rt.pre_pending == 0 and r.net.rt.pre_dropped == 0
    assert rows["resnet18-train-nograd"].counts["adamml_bn_finalize"] == 20 and rows["resnet18-train-nograd"].counts["adamml_bn_eval_affine"] == 0
    assert rows["resnet18-eval"].counts["adamml_bn_finalize"] == 0 and rows["resnet18-eval"].counts["adamml_bn_eval_affine"] == 20
