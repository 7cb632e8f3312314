"""Refusals and the empty-problem return of the conv_gemm.hip entry points (host only, no GPU): every row returns before any launch --
an argument check, a shape the entry point or conv_plan refuses, or P == 0 -- so the pointers are dummy non-null integers nothing
dereferences.  Return code and the full adamml_last_error_string() text are literals: the order of the checks is part of what is pinned
(`N = 0` with `up = 3` is refused, not empty).  The workspace row holds the launch's own split arithmetic (pf_split) to the answer of
adamml_conv_bwd_data_res_prod_workspace, which the guarded conformance rows size their buffers from."""
import re
from ctypes import byref

import pytest

import __graft_entry__ as ge

OK, EINVAL, EUNSUPPORTED = 0, -1, -2            # csrc/common.h
PTR = 0x1000            # a non-null "pointer"; no row reaches code that reads through it
RELU = 1


def desc(N=8, H=56, cin=64, cout=64, k=1, stride=1, pad=0, up=1):
    from adamml_amd.hip import ConvDesc
    return ConvDesc(N, H, H, cin, H // stride, H // stride, cout, k, k, stride, pad, up, 0, 0, 1, 0)


def fwd(lib, d, x=PTR):
    return lib.adamml_conv_fwd(byref(d), x, PTR, None, None, PTR, PTR, None)


def bn_add(lib, d, bn_vec=PTR):
    return lib.adamml_conv_fwd_bn_add(byref(d), PTR, PTR, None, None, bn_vec, PTR, None, None, 0, RELU, PTR, PTR, None)


def tpool(lib, d, frames, in_scale=None):
    return lib.adamml_conv_fwd_bn_add_tpool(byref(d), PTR, PTR, in_scale, in_scale, PTR, PTR, None, None, 0, RELU, frames, PTR, PTR, None)


def res(lib, d, z_b=None, vec_b=None, sums_b=None):
    return lib.adamml_conv_bwd_data_res(byref(d), PTR, PTR, PTR, 0, PTR, None, RELU, PTR, PTR, PTR, z_b, vec_b, sums_b, None)


def alg(lib, d, accumulate=0, z_in=None, bn_vec=None, sums=None):
    return lib.adamml_conv_bwd_data_alg(byref(d), PTR, PTR, PTR, PTR, PTR, PTR, PTR, accumulate, z_in, bn_vec, RELU, sums, None)


def dual(lib, d):
    return lib.adamml_conv_bwd_data_dual(byref(d), PTR, PTR, PTR, None, PTR, PTR, 0, None, None, 0, None, None)


ROWS = [
    ("fwd_null_x", lambda lib: fwd(lib, desc(), x=None), EINVAL, "conv_fwd: null argument"),
    ("fwd_cin_12", lambda lib: fwd(lib, desc(cin=12)), EINVAL, "conv_fwd: channels must be multiples of 8 (Cin=12 Cout=64)"),
    ("fwd_up_3", lambda lib: fwd(lib, desc(up=3)), EUNSUPPORTED, "conv_fwd: up=3 is not a power of two"),
    ("fwd_3x3_cin_24", lambda lib: fwd(lib, desc(cin=24, k=3, pad=1)), EUNSUPPORTED, "conv_fwd: KxK conv needs power-of-two Cin (got 24)"),
    # 64 x 512 x 512 x 128 = 2^31 input elements
    ("fwd_2_31", lambda lib: fwd(lib, desc(N=64, H=512, cin=128, cout=128)), EUNSUPPORTED, "conv_fwd: input tensor exceeds 2^31 elements"),
    ("fwd_empty", lambda lib: fwd(lib, desc(N=0)), OK, None),
    ("fwd_empty_up_3", lambda lib: fwd(lib, desc(N=0, up=3)), EUNSUPPORTED, "conv_fwd: up=3 is not a power of two"),
    ("bn_add_3x3", lambda lib: bn_add(lib, desc(k=3, pad=1)), EUNSUPPORTED, "conv_fwd_bn_add: 1x1 / stride-1 convs only"),
    ("bn_add_null_vec", lambda lib: bn_add(lib, desc(), bn_vec=None), EINVAL, "conv_fwd_bn_add: null BatchNorm vectors"),
    ("tpool_3_frames", lambda lib: tpool(lib, desc(N=6, cout=128), 3), EUNSUPPORTED,
     "conv_fwd_bn_add_tpool: 1x1 / stride-1 conv, Cout % 128 == 0, ReLU, 2 / 4 / 8 / 16 / 32 frames per clip"),
    ("tpool_lazy_cin_1024", lambda lib: tpool(lib, desc(cin=1024, cout=128), 8, in_scale=PTR), EUNSUPPORTED,
     "conv_fwd_bn_add_tpool: 1x1 / stride-1 conv, Cout % 128 == 0, ReLU, 2 / 4 / 8 / 16 / 32 frames per clip"),
    ("res_stride_2", lambda lib: res(lib, desc(stride=2)), EUNSUPPORTED,
     "conv_bwd_data_res: only 1x1 / stride-1 convs and 3x3 / pad-1 / stride-1 convs with Cin == Cout (a power of two >= 64)"),
    ("res_half_second_bn", lambda lib: res(lib, desc(), z_b=PTR), EINVAL, "conv_bwd_data_res: incomplete second BatchNorm operand"),
    ("alg_z_in_without_vec", lambda lib: alg(lib, desc(cin=128, cout=128), z_in=PTR, sums=PTR), EINVAL,
     "conv_bwd_data_alg: incomplete BatchNorm epilogue operands"),
    ("alg_bn_accumulate", lambda lib: alg(lib, desc(cin=128, cout=128), accumulate=1, z_in=PTR, bn_vec=PTR, sums=PTR), EUNSUPPORTED,
     "conv_bwd_data_alg: the BatchNorm epilogue does not accumulate"),
    # (the K of the data gradient is the forward conv's Cout)
    ("alg_k_40", lambda lib: alg(lib, desc(cin=64, cout=40)), EUNSUPPORTED, "conv_bwd_data_alg: 1x1 / stride-1 convs with Cout % 32 == 0 only"),
    ("dual_cout_1024", lambda lib: dual(lib, desc(cin=64, cout=1024)), EUNSUPPORTED, "conv_bwd_data_dual: only 1x1 / stride-1 convs with Cout <= 512"),
]


@pytest.fixture(scope="module")
def lib():
    ge.build()
    from adamml_amd import hip
    return hip.load()


@pytest.mark.parametrize("name,call,rc,message", ROWS, ids=[r[0] for r in ROWS])
def test_refusal(lib, name, call, rc, message):
    got = call(lib)
    assert got == rc
    if message is not None:
        assert lib.adamml_last_error_string().decode() == message


def test_res_prod_workspace_one_byte_short(lib):
    """A tile-kernel shape of adamml_conv_bwd_data_res_prod (128 * 4096 pixels, 128 gradient channels out: 4096 workgroup tiles) with a
    workspace one byte smaller than the query's answer: the launch refuses, and the byte count it asks for is the query's."""
    d = desc(N=8, H=256, cin=128, cout=64)
    assert lib.adamml_conv_bwd_data_res_prod_supported(byref(d), 64) == 1 and lib.adamml_conv_bwd_data_res_prod_streams(byref(d), 64) == 0
    need = lib.adamml_conv_bwd_data_res_prod_workspace(byref(d))
    assert need == 1366 * 128 * 64 * 4                      # 1536 splits wanted -> 3 pixel tiles per workgroup -> ceil(4096 / 3) = 1366 partials
    rc = lib.adamml_conv_bwd_data_res_prod(byref(d), PTR, PTR, PTR, PTR, RELU, PTR, PTR, None, None, 0, 0, 64, PTR, PTR, need - 1, None)
    message = lib.adamml_last_error_string().decode()
    assert rc == EINVAL and message == "conv_bwd_data_res_prod: workspace too small (need %d bytes)" % need
    assert int(re.search(r"need (\d+) bytes", message).group(1)) == need
