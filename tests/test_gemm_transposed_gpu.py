"""gemm_f32_tr_kernel (csrc/dwconv_gemm32.hip): adamml_gemm_f32 on operands read down their columns -- the data-gradient (b transposed),
weight-gradient (both) and mixed (a transposed) forms -- against float64 on the same float32 operands, under the bound the K-contiguous
matrix-core kernel owes (tests/abi_ref.py gemm_f32_ref: acc(K) 2^-24 |a| |b|, plus one rounding each for bias and accumulate: the same
fp32 multiply-accumulate, another summation order).  Operands end in NaN slack, the output lies inside guard bands (tests/guarded.py)
with three NaN padding columns, so a ragged-edge load or store outside the tile shows."""
import pytest
import torch

from tests import abi_ref as A

pytestmark = pytest.mark.gpu

from adamml_amd import hip, runtime, synth  # noqa: E402
from adamml_amd.hip import call, ptr  # noqa: E402
from tests.test_conv_conformance_gpu import GB, guard  # noqa: E402,F401  (guard: the autouse check of every row)
from tests.test_abi_conformance_gpu import lay, NAN  # noqa: E402

# one 64 x 64 x 32 tile; one past a tile in every dimension; K below one 32-deep step with ragged M, N; long thin reductions (S B = 360
# rows) with 8 rows / 8 columns; the 2-row weight gradient of a policy FC head, which the dispatch rule keeps on the VALU kernel
SHAPES = [(64, 64, 32, 1), (65, 65, 33, 1), (37, 70, 20, 1), (8, 256, 360, 1), (2048, 8, 360, 1), (2, 256, 360, 0)]
LAYOUTS = {"dx": ("row", "col"), "mixed": ("col", "row"), "dW": ("col", "col")}
# (accumulate, bias, act, output transposed): every value of every option at least once
OPTIONS = [(0, 0, 0, 0), (1, 1, 1, 0), (0, 1, 2, 1), (1, 0, 0, 1)]


@pytest.mark.parametrize("opt", OPTIONS, ids=lambda o: "acc%d-bias%d-act%d-ct%d" % o)
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "M%d-N%d-K%d" % s[:3])
def test_gemm_f32_transposed(shape, layout, opt):
    M, N, K, on = shape
    accumulate, bias, act, c_t = opt
    seed = 7 * M + 3 * N + K + 11 * list(LAYOUTS).index(layout)
    a, b = A.randn32(M, K, seed=seed), A.randn32(N, K, seed=seed + 1)
    bv = A.randn32(N, seed=seed + 2) if bias else None
    c0 = A.randn32(M, N, seed=seed + 3) if accumulate else None
    ref, tol = A.gemm_f32_ref(a, b, bv, act, c0)
    # leading dimensions padded to the next multiple of 4 (the kernel's alignment rule): ragged M, N, K inside aligned rows
    ka, kb = LAYOUTS[layout]
    _, pa, a_sm, a_sk = lay(a, ka, -(M if ka == "col" else K) % 4)
    _, pb, b_sn, b_sk = lay(b, kb, -(N if kb == "col" else K) % 4)
    lib = hip.load()
    assert lib.adamml_gemm_f32_transposed_supported(pa, a_sm, a_sk, pb, b_sn, b_sk, M, N, K) == on
    assert lib.adamml_gemm_f32_uses_mfma(pa, a_sm, a_sk, pb, b_sn, b_sk, K) == 0        # (a k stride != 1: as before)
    ldc = (M if c_t else N) + 3
    cfull = torch.full((N if c_t else M, ldc), NAN, dtype=torch.float32)
    view = cfull[:, :M].t() if c_t else cfull[:, :N]
    if accumulate:
        view.copy_(c0)
    cd = GB.inout(cfull)
    call("adamml_gemm_f32", pa, a_sm, a_sk, pb, b_sn, b_sk, ptr(cd), 1 if c_t else ldc, ldc if c_t else 1, ptr(GB.frozen(bv)), act, accumulate,
         M, N, K)
    GB.check("gemm_f32 transposed")
    out = cd.cpu()
    assert torch.isnan(out[:, -3:]).all(), "wrote outside the strided output"
    r = A.ratio(out[:, :M].t() if c_t else out[:, :N], ref, tol)
    print("  %s %s %s: max err/tol %.4f" % (shape, layout, opt, r))
    assert r <= 1.0, r


def test_policy_stage_backward_matches_the_k_contiguous_kernels():
    """One policy-stage backward (rgb + sound, LSTM head, S = 2, B = 4: S B = 8 rows, the fewest the dispatch rule
    sends to the kernel; 64 px) with the gradient GEMMs on gemm_f32_tr_kernel against the
    same step with runtime.GEMM_TRANSPOSED cleared (K-contiguous copies: gemm_f32_mfma_kernel / the VALU kernel).  Compared: the
    gradients the fp32 GEMMs form (joint FC, LSTM, FC heads; the backbones below round to bf16 and are not this kernel's).  Gate per
    tensor: both kernels owe acc(K) 2^-24 sum|terms| with sum|terms| >= |g|, so the two differ by at most 2 acc(K) 2^-24 max|g| norm-wise
    per GEMM, K = 2560 the longest reduction of the stage (acc = 8 sqrt(K)), times 3 for the GEMMs chained below the joint FC
    (LSTM data gradient -> joint[2] -> joint[0])."""
    from adamml_amd import adamml
    S, B = 2, 4
    # the stage's gradient GEMMs do reach the kernel: dW[4H, F] = d_gates^T feats reduces over the S B rows, dx[S B, F] = d_gates W_ih over 4H
    assert hip.load().adamml_gemm_f32_transposed_supported(0, 1, 1024, 0, 1, 2048, 1024, 2048, S * B) == 1
    assert hip.load().adamml_gemm_f32_transposed_supported(0, 1024, 1, 0, 1, 2048, S * B, 2048, 1024) == 1
    torch.manual_seed(0)
    model = adamml(groups=8, modality=["rgb", "sound"], input_channels=[3, 1], num_segments=S, rng_policy=False, rng_threshold=0.5,
                   causality_modeling="lstm", num_classes=31, depth=50, without_t_stride=False, dropout=0.0, pooling_method="max",
                   fusion_point="logits", unimodality_pretrained=[], learnable_lf_weights=True).to("cuda")
    model.freeze_main_net()
    model.train()
    xs = [t.to("cuda") for t in synth.synth_inputs(["rgb", "sound"], B, S, 8, 64, 64, seed=5)]
    expo = synth.synth_gumbel_exponential(S, 2, B, seed=11).to("cuda")
    target = torch.tensor([3, 17, 0, 30], device="cuda")
    grads = []
    for flag in (True, False):
        runtime.GEMM_TRANSPOSED = flag
        try:
            model.zero_grad()
            logits, sel = model(xs, gumbel_exponential=expo)
            (torch.nn.functional.cross_entropy(logits, target) + sel.mean()).backward()
        finally:
            runtime.GEMM_TRANSPOSED = True
        grads.append({n: p.grad.detach().double().cpu() for n, p in model.policy_net.named_parameters()
                      if p.grad is not None and (".joint." in n or n.startswith(("lstm.", "fcs.")))})
    assert len(grads[0]) >= 10 and grads[0].keys() == grads[1].keys(), sorted(grads[0])
    gate = 3 * 2 * A.acc(2560) * A.U32
    for n, g in grads[0].items():
        d, scale = (g - grads[1][n]).abs().max().item(), grads[1][n].abs().max().item()
        print("  %-28s max|g| %.3e  max diff %.3e  diff / (gate max|g|) %.4f" % (n, scale, d, d / (gate * scale) if scale else 0.0))
        assert scale > 0 and d <= gate * scale, n
