"""The conv checker of tests/conv_ref.py has teeth (CPU only): a correctly rounded float32 emulation of each kernel passes, and
synthetic outputs built from the float64 reference with one planted defect fail by at least twice the tolerance -- or, for the
truncating store that a per-element bound cannot see, by twice the rounding-bias limit.  Shapes are rows of
tests/test_conv_conformance_gpu.py."""
import math

import pytest
import torch

from tests import conv_ref as R


def rand_bf16(*shape, scale=1.0, offset=0.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale + offset).to(torch.bfloat16)


def weights(cout, cin, k, seed=1):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64) * (2.0 / (cin * k * k)) ** 0.5
    return R.bf16(w)


def emulate(fn, *args):
    """the same contraction with float32 operands and accumulation (torch CPU), the result still float64"""
    return fn(*[a.to(torch.float32) if torch.is_tensor(a) else a for a in args]).double()


def fwd32(a, w, s, p):
    return R.to_nhwc(torch.nn.functional.conv2d(R.to_nchw(a)[:, :w.shape[1]], w, stride=s, padding=p))


def truncate_bf16(x):
    """float64 -> float32 -> bf16 by dropping the low 16 bits (round toward zero)"""
    b = x.to(torch.float32).contiguous().view(torch.int32) & ~0xFFFF
    return b.view(torch.float32).double()


def assert_clean(h, ref, ab, n, rho=R.RHO_BF16, extra=None):
    R.check(h, ref, ab, n, rho, extra, what="clean emulation")


def test_accepts_clean_and_rejects_truncating_store():
    # wide row: 1x1 256 -> 640, P = 2049 (conv1x1_wide.hip wide_all_kernel)
    z = rand_bf16(1, 1, 2049, 256, seed=3)
    w = weights(640, 256, 1)
    a = R.lazy_operand(z)
    ref, ab, n = R.conv_fwd_ref(a, w, 1, 0)
    out32 = emulate(fwd32, a, w, 1, 0)
    assert_clean(R.bf16(out32), ref, ab, n)
    b, cnt = R.rounding_bias(truncate_bf16(out32), ref, ab, n)
    assert cnt >= R.BIAS_MIN_ELEMENTS // 10 and b <= -2 * R.BIAS_LIMIT, (b, cnt)
    with pytest.raises(AssertionError):
        R.check(truncate_bf16(out32), ref, ab, n)


def test_rejects_dropped_last_k_slice():
    # generic MODE 0 at K = 2048: 1x1 2048 -> 512, 2 x 7 x 7 pixels (conv_gemm_kernel<64, 0, 3> deep look-ahead with a lazy input)
    z = rand_bf16(2, 7, 7, 2048, seed=4)
    w = weights(512, 2048, 1)
    a = R.lazy_operand(z)
    ref, ab, n = R.conv_fwd_ref(a, w, 1, 0)
    assert_clean(R.bf16(emulate(fwd32, a, w, 1, 0)), ref, ab, n)
    bad = R.bf16(fwd32(a[..., :2016], w[:, :2016], 1, 0))
    assert R.err_ratio(bad, ref, ab, n, R.RHO_BF16) >= 2


def test_rejects_group_one_with_group_zero_vectors():
    # c64 patch kernel, G = 3 per-group vectors: 3x3 64 -> 64 (conv3x3_c64_kernel)
    G, C = 3, 64
    z = rand_bf16(G * 2, 12, 12, C, seed=5)
    g = torch.Generator().manual_seed(6)
    vec = torch.rand(G, 4, C, generator=g) + 0.5
    vec[:, 1] -= 0.8
    w = weights(C, C, 3)
    a = R.lazy_operand(z, vec.view(-1), vec.view(-1)[C:], 1, groups=G, gstride=4 * C)
    ref, ab, n = R.conv_fwd_ref(a, w, 1, 1)
    assert_clean(R.bf16(emulate(fwd32, a, w, 1, 1)), ref, ab, n)
    vbad = vec.clone()
    vbad[1] = vec[0]
    abad = R.lazy_operand(z, vbad.view(-1), vbad.view(-1)[C:], 1, groups=G, gstride=4 * C)
    assert R.err_ratio(R.bf16(fwd32(abad, w, 1, 1)), ref, ab, n, R.RHO_BF16) >= 2


def test_rejects_missing_relu6_upper_clamp():
    # narrow instance (1, 96): 1x1 24 -> 96, lazy ReLU6 over data that crosses 0 and 6 (conv1x1_narrow_fwd_kernel<1, 96>)
    z = rand_bf16(2, 21, 19, 24, scale=3.0, offset=2.0, seed=7)
    g = torch.Generator().manual_seed(8)
    s, t = torch.rand(24, generator=g) + 0.5, torch.randn(24, generator=g)
    w = weights(96, 24, 1)
    a = R.lazy_operand(z, s, t, 2)
    assert (a == 6).any() and (a == 0).any()
    ref, ab, n = R.conv_fwd_ref(a, w, 1, 0)
    assert_clean(R.bf16(emulate(fwd32, a, w, 1, 0)), ref, ab, n)
    abad = R.lazy_operand(z, s, t, 1)
    assert R.err_ratio(R.bf16(fwd32(abad, w, 1, 0)), ref, ab, n, R.RHO_BF16) >= 2


def test_rejects_tail_chunk_reading_the_next_channel_scale():
    # generic MODE 0 with K = 40 (not a multiple of 32): the last 8-channel chunk reads scale[c + 1]
    z = rand_bf16(2, 30, 30, 40, seed=9)
    g = torch.Generator().manual_seed(10)
    s, t = torch.rand(40, generator=g) + 0.5, torch.randn(40, generator=g) * 0.3
    w = weights(200, 40, 1)
    a = R.lazy_operand(z, s, t, 1)
    ref, ab, n = R.conv_fwd_ref(a, w, 1, 0)
    assert_clean(R.bf16(emulate(fwd32, a, w, 1, 0)), ref, ab, n)
    sbad = s.clone()
    sbad[32:39] = s[33:40]
    abad = R.lazy_operand(z, sbad, t, 1)
    assert R.err_ratio(R.bf16(fwd32(abad, w, 1, 0)), ref, ab, n, R.RHO_BF16) >= 2


@pytest.mark.parametrize("P", [2049, 2047])
def test_rejects_unwritten_pixel_tail_tile(P):
    # P mod 128 in {1, 127}: the last partial 128-pixel tile is never stored (the output buffer was zeroed)
    z = rand_bf16(1, 1, P, 64, seed=11)
    w = weights(264, 64, 1)
    a = R.lazy_operand(z)
    ref, ab, n = R.conv_fwd_ref(a, w, 1, 0)
    good = R.bf16(emulate(fwd32, a, w, 1, 0))
    assert_clean(good, ref, ab, n)
    bad = good.clone()
    bad[:, :, P - P % 128:] = 0
    assert R.err_ratio(bad, ref, ab, n, R.RHO_BF16) >= 2


def test_rejects_missing_parity_class_of_stride2_dgrad():
    # stride-2 3x3 pad 1 data gradient by parity class (conv_gemm_kernel MODE 3), odd H and W
    N, H, W, Cin, Cout = 2, 15, 13, 64, 128
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    gz = R.lazy_operand(rand_bf16(N, OH, OW, Cout, seed=12))
    w = weights(Cout, Cin, 3)
    ref, ab, n = R.conv_dgrad_ref(gz, w, (H, W), 2, 1)
    good = R.bf16(emulate(lambda g_, w_: R.to_nhwc(torch.nn.grad.conv2d_input((N, Cin, H, W), w_, R.to_nchw(g_), 2, 1)), gz, w))
    assert_clean(good, ref, ab, n)
    bad = good.clone()
    bad[:, 1::2, 1::2] = 0
    assert R.err_ratio(bad, ref, ab, n, R.RHO_BF16) >= 2


def test_rejects_missing_split_partial_of_wgrad():
    # 1x1 256 -> 512 weight gradient over 2 x 24 x 24 pixels, split into 256-pixel partials (conv_wgrad_glds_kernel<256, 128>)
    N, H, W, Cin, Cout = 2, 24, 24, 256, 512
    a = R.lazy_operand(rand_bf16(N, H, W, Cin, seed=13))
    gz = R.lazy_operand(rand_bf16(N, H, W, Cout, scale=0.25, seed=14))
    ref, ab, n = R.conv_wgrad_ref(a, gz, (Cout, Cin, 1, 1), 1, 0)
    good = emulate(lambda a_, g_: torch.nn.grad.conv2d_weight(R.to_nchw(a_), (Cout, Cin, 1, 1), R.to_nchw(g_)), a, gz)
    assert_clean(good.to(torch.float32).double(), ref, ab, n, rho=R.RHO_F32)
    flat_a, flat_g = a.reshape(-1, Cin), gz.reshape(-1, Cout)
    bad = (flat_g[256:].t() @ flat_a[256:]).view(Cout, Cin, 1, 1)
    assert R.err_ratio(bad, ref, ab, n, R.RHO_F32) >= 2


def test_bn_mask_is_strict_at_the_bounds():
    z = torch.tensor([-2.0, 10.0, 3.0, 12.0, -4.0], dtype=torch.bfloat16).view(1, 1, 5, 1).expand(1, 1, 5, 8).contiguous()
    vec = torch.zeros(4, 8)
    vec[0], vec[1] = 0.5, 1.0                                   # pre-activations 0, 6, 2.5, 7, -1
    assert R.bn_mask(z, vec, 2)[0, 0, :, 0].tolist() == [0, 0, 1, 0, 0]
    assert R.bn_mask(z, vec, 1)[0, 0, :, 0].tolist() == [0, 1, 1, 1, 0]
    assert R.bn_mask(z, vec, 0)[0, 0, :, 0].tolist() == [1, 1, 1, 1, 1]


def test_lazy_operand_propagates_nan_and_zeroes_padding():
    z = torch.ones(1, 1, 2, 8, dtype=torch.bfloat16)
    s, t = torch.ones(8), torch.zeros(8)
    s[1] = math.nan
    a = R.lazy_operand(z, s, t, 1, cin_true=5)
    assert math.isnan(a[0, 0, 0, 1].item()) and a[0, 0, 0, 0].item() == 1.0 and (a[..., 5:] == 0).all()
