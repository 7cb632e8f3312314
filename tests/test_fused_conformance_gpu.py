"""Conformance of the fused 1x1 kernels of ResNet-50 layers 1 and 2 against float64 references (tests/fused_ref.py).

One row per kernel instance that adamml_conv_fwd_bn_add / _next / _tpool, adamml_conv_bwd_data_res / _res_prod / _dual, adamml_gram_colsum /
adamml_gram_stats, adamml_temporal_pool_bwd_code_prod and the weight packs can select (profiles/fused_conformance_rows.md lists what each
row launched); the row id names the instance in brackets (conv_gemm_kernel rows: cout tile, then FADD / RES / DUAL, EID = identity-side
operands requested at the start of the tile, LZF = fragment-side lazy input, PF = with the product, TPn = pooled over n frames).  Every
row asserts the dispatch probe that selects its kernel, takes every buffer it hands to a kernel from tests/guarded.py (outputs, statistic
accumulators and workspaces inside sentinel bands, asserted untouched; read-only operands compared bit for bit after the launch),
pre-fills the output itself with NaN (an element a kernel never writes fails) and compares per element with the counted error model of
its reference.  The rows that take a workspace run three times: exactly the size the query answers, the same on a workspace that held
other bytes (bit-identical outputs), and one float short (refused, nothing written).

The forward rows (FADD_ROWS, NEXT_ROWS, TPOOL_ROWS) and their operand generators live in tests/fused_ref.py, not here, so that
tests/test_fused_ref_cpu.py can bound their undecided share without a GPU; the backward, Gram and pack rows are defined below."""
import math
import time

import pytest
import torch
from ctypes import byref

from tests import conv_ref as R
from tests import elementwise_ref as E
from tests import fused_ref as F

pytestmark = pytest.mark.gpu

from adamml_amd import hip  # noqa: E402
from adamml_amd.hip import ConvDesc, call, ptr  # noqa: E402
from tests.guarded import workspace_launches  # noqa: E402
from tests.test_conv_conformance_gpu import GB, guard, pack, ssum, zstats, finite_pattern_matches  # noqa: E402,F401  (guard: the autouse check)

WORST = {}            # row id -> max err / tol (printed at the end of the module: pytest -s)
T0 = time.time()
NAN = float("nan")


def record(rid, r):
    WORST[rid] = max(WORST.get(rid, 0.0), r)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    if WORST:
        k = max(WORST, key=WORST.get)
        print("\nfused conformance: C_ACC = %g, largest err/tol %.4f (%s) over %d rows, %.0f s" % (R.C_ACC, WORST[k], k, len(WORST), time.time() - T0))
        for rid in sorted(WORST):
            print("  %-84s %.4f" % (rid, WORST[rid]))


def lib():
    return hip.load()


class Guarded:
    """[rows, c] view of tests/guarded.py: an output (NaN / byte pattern inside its bands), or an in/out buffer initialised from `fill`"""

    def __init__(self, rows, c, dtype, fill=None):
        self.t = GB.inout(fill.reshape(rows, c)) if fill is not None else GB.out((rows, c), dtype)

    def check(self, what, written=True):
        if not written:
            GB.unwritten_ok(self.t)
        GB.check(what)
        return self.t


def untouched(g):
    """the whole allocation is as it was handed out (an unsupported call must not write)"""
    GB.unwritten_ok(g.t)
    return GB.untouched(g.t)


def setenv(monkeypatch, env, *names):
    for n in names:
        monkeypatch.delenv(n, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


def w4(w):
    return w.reshape(w.shape[0], w.shape[1], 1, 1)


def collapse(s, C, G, written=True):
    out = ssum(s)
    if not written:
        GB.unwritten_ok(out)
    return out.cpu()


def stat_acc(G, C):
    return zstats(G, C)


def three(q, outputs, launch, rid):
    """exact / dirty / short launches of a workspace row whose entry point refuses an undersized workspace (tests/guarded.py); outputs()
    -> Guarded objects and accumulators.  The table gets the two extra launches as rows of their own."""
    def raw(o):
        return o.t if isinstance(o, Guarded) else o
    made = []

    def make():
        made.append(outputs())
        return tuple(raw(o) for o in made[-1])

    workspace_launches(GB, q, make, lambda outs, ws, nbytes: launch(made[-1], ws, nbytes), "refuse", rid, sync=torch.cuda.synchronize)
    record(rid + "+dirty", 0.0)
    record(rid + "+short", 0.0)
    return made[0], None


# ------------------------------------------------------------------------------------------------------------------------------ forward
class FwdArgs:
    def __init__(self, row, op, N, H, W):
        Cin, Cout, G = row["Cin"], row["Cout"], row["G"]
        lazy = op["xvec"] is not None
        self.d = ConvDesc(N, H, W, Cin, H, W, Cout, 1, 1, 1, 0, 1, (op["in_act"] or 0) if lazy else 0, 0, G, 4 * Cin if lazy else 0)
        self.x = GB.frozen(op["x"])
        self.xv = GB.frozen(op["xvec"].reshape(-1)) if lazy else None
        self.wp = pack(w4(op["w"]), Cin, 0)
        self.vec = GB.frozen(op["vec"])
        self.idn = GB.frozen(op["idn"])
        self.iv = GB.frozen(op["ivec"].reshape(-1)) if op["ivec"] is not None else None
        self.head = (byref(self.d), ptr(self.x), ptr(self.wp), ptr(self.xv), ptr(self.xv[Cin:]) if lazy else None, ptr(self.vec), ptr(self.idn),
                     ptr(self.iv), ptr(self.iv[Cout:]) if self.iv is not None else None, op["id_gstride"], row["act"])


@pytest.mark.parametrize("row", F.FADD_ROWS, ids=[r["id"] for r in F.FADD_ROWS])
def test_conv_fwd_bn_add(row, monkeypatch):
    setenv(monkeypatch, row.get("env"), "ADAMML_FADD_STREAM")
    G, P, Cout = row["G"], row["P"], row["Cout"]
    op = F.fadd_operands(row)
    r = F.fadd_reference(row, op)
    a = FwdArgs(row, op, 1, P, 1)
    assert lib().adamml_conv_fwd_bn_add_supported(byref(a.d)) == 1
    assert lib().adamml_conv_fwd_bn_add_streams(byref(a.d)) == row["stream"], "dispatch probe"
    # (the probe looks at the shape alone; the streaming kernel also needs an identity: "l2-P4097-relu-noid" answers 1 and runs the tile kernel)
    assert bool(row["stream"] and row["idn"] is not None) == ("fadd_stream_kernel" in row["id"]), "the row id names the other kernel family"
    out = Guarded(G * P, Cout, torch.bfloat16)
    mask = Guarded(G * P, Cout // 8, torch.uint8) if row["mask"] else None
    call("adamml_conv_fwd_bn_add", *a.head, ptr(out.t), ptr(mask.t) if mask else None)
    h = out.check(row["id"]).cpu()
    m = mask.check(row["id"] + " mask").cpu() if mask else None
    q, und = F.fadd_check(h, r, row["act"], m, row["id"])
    assert und <= F.UNDECIDED_CAP
    ex = r["exact"]
    assert ex.any() and torch.equal(h.double().reshape(ex.shape)[ex], r["ref"][ex]), "planted bounds"
    if row["act"]:
        lo, hi = R.ACT_BOUNDS[row["act"]]
        pe = r["pre"][ex]
        assert (pe == lo).any() and (hi == math.inf or (pe == hi).any()), "no pre-activation exactly on a bound"
    record(row["id"], q)


@pytest.mark.parametrize("row", F.NEXT_ROWS, ids=[r["id"] for r in F.NEXT_ROWS])
def test_conv_fwd_bn_add_next(row):
    G, P, Cout, Cn = row["G"], row["P"], row["Cout"], 64
    op = F.fadd_operands(row)
    r = F.fadd_reference(row, op)
    a = FwdArgs(row, op, 1, P, 1)
    assert lib().adamml_conv_fwd_bn_add_next_supported(byref(a.d), Cn) == 1, "dispatch probe"
    wn = F.weight(Cn, Cout, F.seed_of(row["id"]) + 7)
    wnp = pack(w4(wn), Cout, 0)
    out, y = Guarded(G * P, Cout, torch.bfloat16), Guarded(G * P, Cn, torch.bfloat16)
    mask = Guarded(G * P, Cout // 8, torch.uint8) if row["mask"] else None
    st = stat_acc(G, Cn) if row["stats"] else None
    call("adamml_conv_fwd_bn_add_next", *a.head, ptr(out.t), ptr(mask.t) if mask else None, ptr(wnp), ptr(y.t), ptr(st))
    h = out.check(row["id"]).cpu()
    m = mask.check(row["id"] + " mask").cpu() if mask else None
    q, und = F.fadd_check(h, r, row["act"], m, row["id"])
    assert und <= F.UNDECIDED_CAP
    yh = y.check(row["id"] + " y_next").cpu()
    yr, ya, n = F.fwd_bn_add_next_ref(h, wn, G)
    q = max(q, R.check(yh.reshape(yr.shape), yr, ya, n, what=row["id"] + " y_next"))
    if st is not None:
        R.stats_check(ssum(st), yh.reshape(G * P, 1, 1, Cn), what=row["id"] + " stats_next", groups=G)
    record(row["id"], q)


@pytest.mark.parametrize("row", F.TPOOL_ROWS, ids=[r["id"] for r in F.TPOOL_ROWS])
def test_conv_fwd_bn_add_tpool(row, monkeypatch):
    monkeypatch.setenv("ADAMML_FADD_TPOOL_SLICE", row["slice"])
    T, clips, Q, G, Cout = row["T"], row["clips"], row["Q"], row["G"], row["Cout"]
    op = F.tpool_operands(row)
    r, p = F.tpool_reference(row, op)
    a = FwdArgs(dict(row, act=1), op, clips * T, Q, 1)
    assert lib().adamml_conv_fwd_bn_add_tpool_supported(byref(a.d), T, 1, 1 if op["xvec"] is not None else 0) == 1
    assert lib().adamml_conv_fwd_bn_add_tpool_streams(byref(a.d), T) == row["probe"], "dispatch probe"
    rows = G * clips * (T // 2) * Q
    pooled = Guarded(rows, Cout, torch.bfloat16)
    code = Guarded(rows, Cout // 8, torch.int16) if row["code"] else None
    call("adamml_conv_fwd_bn_add_tpool", *a.head, T, ptr(pooled.t), ptr(code.t) if code else None)
    h = pooled.check(row["id"]).cpu()
    c = code.check(row["id"] + " code").cpu() if code else None
    q, und = F.tpool_check(h, c, p, row["id"])
    assert und <= F.UNDECIDED_CAP
    if c is not None:
        cc = F.unpack_codes(c, p["ref"].shape)
        assert (cc[..., Cout - 8:] == 3).all(), "channels whose block output is <= 0 everywhere must carry code 3"
        assert p["must3"].any() and (~p["must3"] & ~p["und3"]).any()
    record(row["id"], q)


# ----------------------------------------------------------------------------------------------------- residual data gradient (+ product)
def _rrow(rid, G, P, C, K, acc, form, res_act, za, zb, stream, env=None):
    return dict(id=rid, G=G, P=P, C=C, K=K, acc=acc, form=form, res_act=res_act, za=za, zb=zb, stream=stream, env=env)


# C = d->Cin (channels of dx), K = d->Cout (channels of dz); form: act' from the stored block output ("out") or the 1-bit mask ("bits");
# stream: what adamml_conv_bwd_data_res_streams must answer.  The probe looks at the shape alone; the launcher adds the argument-level
# condition (accumulate, bits, z_a NULL), which run_res asserts against the kernel family the row id names: "tile-512x128-acc-bits-za-g3-wide"
# has the streaming shape (probe 1) but passes z_a, so the tile kernel serves it (profiles/fused_conformance_rows.md: the trace)
RES_ROWS = [
    _rrow("tile-256x64-acc-out-relu-za-P401[conv_gemm_kernel<64,RES>]", 1, 401, 256, 64, 1, "out", 1, True, False, 0),
    _rrow("tile-24x144-out-none-za-P300[conv_gemm_kernel<64,RES>]", 1, 300, 24, 144, 0, "out", 0, True, False, 0),
    _rrow("tile-256x64-acc-bits-relu6-za-zb-g3[conv_gemm_kernel<64,RES>]", 3, 333, 256, 64, 1, "bits", 2, True, True, 0),
    _rrow("tile-256x64-out-relu-noza-P97[conv_gemm_kernel<64,RES>]", 1, 97, 256, 64, 0, "out", 1, False, False, 0),
    _rrow("tile-512x128-P4095-acc-bits-noza[conv_gemm_kernel<64,RES,EID>]", 1, 4095, 512, 128, 1, "bits", 1, False, False, 0),
    _rrow("tile-512x128-acc-bits-noza-g3-wide-streamoff[conv_gemm_kernel<128,RES,EID>]", 3, 5500, 512, 128, 1, "bits", 1, False, False, 0,
          {"ADAMML_RES_PROD_STREAM": "0"}),
    _rrow("tile-512x128-acc-bits-za-g3-wide[conv_gemm_kernel<128,RES>]", 3, 5500, 512, 128, 1, "bits", 1, True, False, 1),
    _rrow("stream-512x128-P4096-acc-bits-noza[res_prod_stream_kernel<8,128,false,false>]", 1, 4096, 512, 128, 1, "bits", 1, False, False, 1),
    _rrow("stream-512x128-P4121-acc-bits-noza-zb-g3[res_prod_stream_kernel<8,128,false,true>]", 3, 4121, 512, 128, 1, "bits", 1, False, True, 1),
    _rrow("stream-512x128-full-P28224-g2[res_prod_stream_kernel<8,128,false,false>]", 2, 28224, 512, 128, 1, "bits", 1, False, False, 1),
]


def res_operands(row):
    G, P, C, K = row["G"], row["P"], row["C"], row["K"]
    s = F.seed_of(row["id"])
    op = {"dz": E.rand_bf16(G * P, K, scale=0.5, seed=s), "w": F.weight(K, C, s + 1)}
    op["dx_in"] = E.rand_bf16(G * P, C, seed=s + 2) if row["acc"] else None
    ro = E.rand_bf16(G * P, C, scale=3.0, offset=1.0, seed=s + 3).float()
    op["res_out"] = (ro.clamp(0, 6) if row["res_act"] == 2 else ro.clamp_min(0) if row["res_act"] else ro).to(torch.bfloat16)   # exact 0 and 6 occur
    op["m"] = E.act_mask(op["res_out"].double(), row["res_act"]).reshape(G, P, C)
    op["bits"] = F.pack_bits(op["m"].bool())
    op["za"], op["va"] = E.rand_bf16(G * P, C, seed=s + 4), E.bn_vectors(G, C, s + 5)
    op["zb"], op["vb"] = E.rand_bf16(G * P, C, seed=s + 6), E.bn_vectors(G, C, s + 7)
    return op


def run_res(row, op, finite=True):
    """finite=False: the row plants NaN, which the sums then hold as well"""
    G, P, C, K = row["G"], row["P"], row["C"], row["K"]
    d = ConvDesc(1, P, 1, C, P, 1, K, 1, 1, 1, 0, 1, 0, 0, G, 0)
    assert lib().adamml_conv_bwd_data_res_supported(byref(d)) == 1
    assert lib().adamml_conv_bwd_data_res_streams(byref(d)) == row["stream"], "dispatch probe"
    streams = bool(row["stream"] and row["acc"] and row["form"] == "bits" and not row["za"])        # the launcher's own condition
    assert streams == row["id"].startswith("stream-"), "the row id names the other kernel family"
    keep = {k: (GB.frozen(v) if torch.is_tensor(v) and k != "dx_in" else v) for k, v in op.items()}
    wp = pack(w4(op["w"]), C, 1)
    dx = Guarded(G * P, C, torch.bfloat16, fill=op["dx_in"] if row["acc"] else None)
    sa, sb = stat_acc(G, C), stat_acc(G, C)
    bits = row["form"] == "bits"
    res_out = dx.t if (bits and row["acc"]) else keep["res_out"]          # (the mask form never reads res_out: the runtime passes dx)
    call("adamml_conv_bwd_data_res", byref(d), ptr(keep["dz"]), ptr(wp), ptr(dx.t), row["acc"], ptr(res_out), ptr(keep["bits"]) if bits else None,
         row["res_act"], ptr(keep["za"]) if row["za"] else None, ptr(keep["va"]), ptr(sa), ptr(keep["zb"]) if row["zb"] else None,
         ptr(keep["vb"]) if row["zb"] else None, ptr(sb) if row["zb"] else None)
    return dx, collapse(sa, C, G, finite), collapse(sb, C, G, finite)


@pytest.mark.parametrize("row", RES_ROWS, ids=[r["id"] for r in RES_ROWS])
def test_conv_bwd_data_res(row, monkeypatch):
    setenv(monkeypatch, row["env"], "ADAMML_RES_PROD_STREAM")
    G, P, C = row["G"], row["P"], row["C"]
    op = res_operands(row)
    dx, sa, sb = run_res(row, op)
    h = dx.check(row["id"]).cpu()
    ref, ab, n, extra = F.res_ref(F.gview(op["dz"].double(), G), op["w"], op["m"], F.gview(op["dx_in"], G) if row["acc"] else None)
    assert (op["m"] == 1).any() and ((op["m"] == 0).any() or not row["res_act"])         # (no activation: act' is 1 everywhere)
    q = R.check(h.reshape(ref.shape), ref, ab, n, extra=extra, what=row["id"], bias=ref.numel() >= R.BIAS_MIN_ELEMENTS)
    F.res_sums_check(sa, h, op["za"] if row["za"] else None, op["va"], G, row["id"] + " sums_a")
    if row["zb"]:
        F.res_sums_check(sb, h, op["zb"], op["vb"], G, row["id"] + " sums_b")
    else:
        assert (sb == 0).all()
    record(row["id"], q)


def test_conv_bwd_data_res_stream_threshold_is_4096_pixels_per_group():
    """include/adamml_hip.h: both streaming forms of csrc/res_prod_stream.hip (rps_1x1) serve >= 4096 pixels per group"""
    for P, want in ((4095, 0), (4096, 1)):
        for G in (1, 3):
            assert lib().adamml_conv_bwd_data_res_streams(byref(ConvDesc(1, P, 1, 512, P, 1, 128, 1, 1, 1, 0, 1, 0, 0, G, 0))) == want
            assert lib().adamml_conv_bwd_data_res_prod_streams(byref(ConvDesc(1, P, 1, 256, P, 1, 64, 1, 1, 1, 0, 1, 0, 0, G, 0)), 64) == want


# (id, G, P, C, K, lazy a, a_act, streams probe, env)
PROD_ROWS = [
    ("stream-256x64-P4205-lazy-relu-g2[res_prod_stream_kernel<4,64,true,false>]", 2, 4205, 256, 64, True, 1, 1, None),
    ("stream-256x64-P4096-plain-g1[res_prod_stream_kernel<4,64,true,false>]", 1, 4096, 256, 64, False, 0, 1, None),
    ("stream-256x64-full-P70560-lazy-relu6-g2[res_prod_stream_kernel<4,64,true,false>]", 2, 70560, 256, 64, True, 2, 1, None),
    # the tile kernel needs ceil(P / 128) * (C / 128) * groups >= 4096 workgroups: 256 * 2 * 8 exactly, the last pixel tile partial
    ("tile-256x64-P32700-lazy-relu-g8-streamoff[conv_gemm_kernel<128,RES,EID,PF>]", 8, 32700, 256, 64, True, 1, 0, {"ADAMML_RES_PROD_STREAM": "0"}),
    ("tile-512x128-P16300-plain-g8[conv_gemm_kernel<128,RES,EID,PF>]", 8, 16300, 512, 128, False, 0, 0, None),
]


def prod_operands(rid, G, P, C, K, lazy, a_act):
    s = F.seed_of(rid)
    op = {"dz": E.rand_bf16(G * P, K, scale=0.5, seed=s), "w": F.weight(K, C, s + 1), "dx_in": E.rand_bf16(G * P, C, seed=s + 2),
          "bits": torch.randint(0, 256, (G * P * C // 8,), generator=F.gen(s + 3), dtype=torch.int32).to(torch.uint8),
          "a": E.plant_bounds(E.rand_bf16(G * P, 64, scale=3.0 if a_act == 2 else 1.5, offset=1.0 if a_act == 2 else 0.0, seed=s + 4)),
          "av": E.bn_vectors(G, 64, s + 5, a_act) if lazy else None}
    return op


@pytest.mark.parametrize("row", PROD_ROWS, ids=[r[0] for r in PROD_ROWS])
def test_conv_bwd_data_res_prod(row, monkeypatch):
    rid, G, P, C, K, lazy, a_act, streams, env = row
    setenv(monkeypatch, env, "ADAMML_RES_PROD_STREAM")
    d = ConvDesc(1, P, 1, C, P, 1, K, 1, 1, 1, 0, 1, 0, 0, G, 0)
    assert lib().adamml_conv_bwd_data_res_prod_supported(byref(d), 64) == 1
    assert lib().adamml_conv_bwd_data_res_prod_streams(byref(d), 64) == streams, "dispatch probe"
    op = prod_operands(rid, G, P, C, K, lazy, a_act)
    dv = {k: (GB.frozen(v) if torch.is_tensor(v) and k != "dx_in" else v) for k, v in op.items()}
    wp = pack(w4(op["w"]), C, 1)
    avf = dv["av"].reshape(-1) if lazy else None

    def launch(outs, ws, nbytes):
        dx, prod, sa = outs
        call("adamml_conv_bwd_data_res_prod", byref(d), ptr(dv["dz"]), ptr(wp), ptr(dx.t), ptr(dv["bits"]), 1, ptr(sa), ptr(dv["a"]), ptr(avf),
             ptr(avf[64:]) if lazy else None, a_act if lazy else 0, 4 * 64 if lazy else 0, 64, ptr(prod.t), ptr(ws), nbytes)

    def outputs():
        return Guarded(G * P, C, torch.bfloat16, fill=op["dx_in"]), Guarded(G * C, 64, torch.float32), stat_acc(G, C)

    # exact, dirty (the partials are overwritten, never read first), one float short: refused by both launchers before anything runs
    need = lib().adamml_conv_bwd_data_res_prod_workspace(byref(d))
    (dx, prod, sa), _ = three(need, outputs, launch, rid)
    h = dx.check(rid).cpu().reshape(G, P, C)
    ph = prod.check(rid + " prod").cpu().reshape(G, C, 64)
    s = collapse(sa, C, G)
    avc = op["av"].reshape(-1) if lazy else None
    a = F.operand(op["a"], avc, avc[64:] if lazy else None, a_act if lazy else 0, G, 4 * 64 if lazy else 0)
    m = F.unpack_bits(op["bits"], (G, P, C)).double()
    q = 0.0
    for g in range(G):              # per group: the float64 tensors of all eight groups at once are several GB
        sl = slice(g, g + 1)
        ref, ab, n, extra = F.res_ref(F.gview(op["dz"].double(), G)[sl], op["w"], m[sl], F.gview(op["dx_in"], G)[sl])
        q = max(q, R.check(h[sl], ref, ab, n, extra=extra, what="%s group %d" % (rid, g), bias=True))
        pr, pa, pn = F.res_prod_ref(h[sl].double(), a[sl])
        q = max(q, F.prod_check(ph[sl], pr, pa, pn, "%s prod group %d" % (rid, g)))
    F.res_sums_check(s, h, None, None, G, rid + " sums")
    record(rid, q)


def test_conv_bwd_data_res_prod_below_the_workgroup_term_is_refused(monkeypatch):
    """one pixel tile below ceil(P / 128) * (C / 128) * groups >= 4096 (and the streaming kernel off): ADAMML_EUNSUPPORTED, nothing written"""
    monkeypatch.setenv("ADAMML_RES_PROD_STREAM", "0")
    G, C, K = 8, 256, 64
    P = 32700 - 128
    d = ConvDesc(1, P, 1, C, P, 1, K, 1, 1, 1, 0, 1, 0, 0, G, 0)
    assert lib().adamml_conv_bwd_data_res_prod_supported(byref(d), 64) == 0
    assert lib().adamml_conv_bwd_data_res_prod_supported(byref(ConvDesc(1, P + 128, 1, C, P + 128, 1, K, 1, 1, 1, 0, 1, 0, 0, G, 0)), 64) == 1
    dx, prod = Guarded(G * P, C, torch.bfloat16), Guarded(G * C, 64, torch.float32)
    dz = GB.frozen(torch.zeros(G * P, K, dtype=torch.bfloat16))
    wp = GB.frozen(torch.zeros(C, K, dtype=torch.bfloat16))
    bits = GB.frozen(torch.zeros(G * P * C // 8, dtype=torch.uint8))
    a = GB.frozen(torch.zeros(G * P, 64, dtype=torch.bfloat16))
    sa = stat_acc(G, C)
    ws = GB.workspace(4 << 20)
    with pytest.raises(RuntimeError, match=r"\(-2\)"):
        call("adamml_conv_bwd_data_res_prod", byref(d), ptr(dz), ptr(wp), ptr(dx.t), ptr(bits), 1, ptr(sa), ptr(a), None, None, 0, 0, 64, ptr(prod.t),
             ptr(ws), ws.numel())
    torch.cuda.synchronize()
    assert untouched(dx) and untouched(prod) and GB.untouched(sa) and GB.untouched(ws)


# ------------------------------------------------------------------------------------------------------------------------------- dual
# (id, G, P, Cin (channels of dx), Cout (channels of g, z, dz), mode, narrow probe (adamml_conv1x1_narrow_supported(d, 2)))
DUAL_ROWS = [
    ("tile-64x256-plain-P700[conv_gemm_kernel<64,DUAL>]", 1, 700, 64, 256, "plain", 0),
    ("tile-64x256-acc-g3-P333[conv_gemm_kernel<64,DUAL>]", 3, 333, 64, 256, "acc", 0),
    ("tile-128x512-bn-relu-g3-P500[conv_gemm_kernel<64,DUAL>]", 3, 500, 128, 512, "bn1", 0),
    ("tile-256x384-plain-g3-wide[conv_gemm_kernel<128,DUAL>]", 3, 11000, 256, 384, "plain", 0),
    ("tile-256x384-bn-relu6-g3-wide[conv_gemm_kernel<128,DUAL>]", 3, 11000, 256, 384, "bn2", 0),
    ("tile-256x64-acc-g5-wide[conv_gemm_kernel<128,DUAL>]", 5, 6600, 256, 64, "acc", 0),
    ("narrow-96x24-acc-P399[conv1x1_narrow_dgrad_kernel<1,96,DUAL,acc>]", 1, 399, 96, 24, "acc", 1),
    ("narrow-32x16-bn-relu6-g2-P247[conv1x1_narrow_dgrad_kernel<1,32,DUAL,bn>]", 2, 247, 32, 16, "bn2", 1),
    ("narrow-192x32-plain-P209[conv1x1_narrow_dgrad_kernel<1,192,DUAL>]", 1, 209, 192, 32, "plain", 1),
    ("narrow-144x32-bn-relu6-g5-P361[conv1x1_narrow_dgrad_kernel<1,144,DUAL,bn>]", 5, 361, 144, 32, "bn2", 1),
]


@pytest.mark.parametrize("row", DUAL_ROWS, ids=[r[0] for r in DUAL_ROWS])
def test_conv_bwd_data_dual(row):
    rid, G, P, Cin, Cout, mode, narrow = row
    s = F.seed_of(rid)
    d = ConvDesc(1, P, 1, Cin, P, 1, Cout, 1, 1, 1, 0, 1, 0, 0, G, 0)
    assert lib().adamml_conv_bwd_data_dual_supported(byref(d)) == 1
    assert lib().adamml_conv1x1_narrow_supported(byref(d), 2) == narrow, "dispatch probe"
    g, z = E.rand_bf16(G * P, Cout, seed=s), E.rand_bf16(G * P, Cout, scale=2.0, offset=0.5, seed=s + 1)
    aff = torch.randn(G, 3, Cout, generator=F.gen(s + 2)) * torch.tensor([1.0, 0.3, 0.2]).reshape(1, 3, 1)
    w = F.weight(Cout, Cin, s + 3)
    bn = int(mode[2]) if mode.startswith("bn") else None
    zin = E.act_data(G * P, Cin, bn, s + 4) if bn else None
    vin = E.bn_vectors(G, Cin, s + 5, bn) if bn else None
    base = E.rand_bf16(G * P, Cin, seed=s + 6) if mode == "acc" else None
    gd, zd, ad, wp = GB.frozen(g), GB.frozen(z), GB.frozen(aff), pack(w4(w), Cin, 1)
    zind, vind = (GB.frozen(zin), GB.frozen(vin)) if bn else (None, None)
    res = []
    for with_side in (True, False):
        dx = Guarded(G * P, Cin, torch.bfloat16, fill=base)
        side = Guarded(G * P, Cout, torch.bfloat16) if with_side else None
        sums = stat_acc(G, Cin) if bn else None
        call("adamml_conv_bwd_data_dual", byref(d), ptr(gd), ptr(zd), ptr(ad), ptr(side.t) if side else None, ptr(wp), ptr(dx.t),
             1 if mode == "acc" else 0, ptr(zind), ptr(vind), bn or 0, ptr(sums))
        res.append((dx.check(rid).cpu(), side.check(rid + " dz_side").cpu() if side else None, collapse(sums, Cin, G) if bn else None))
    (h, dzh, sm), (h2, _, sm2) = res
    assert torch.equal(h.view(torch.int16), h2.view(torch.int16)), "dx differs without the side output"
    dzr, dza = F.dual_dz_ref(g, z, aff, G)
    q = R.check(dzh.reshape(dzr.shape), dzr, dza, 1, acc=F.DUAL_OPS, what=rid + " dz_side")
    ref, ab, n, extra = F.dual_ref(F.gview(dzh.double(), G), w, base, zin, vin, bn or 0, G)
    q = max(q, R.check(h.reshape(ref.shape), ref, ab, n, extra=extra, what=rid))
    if bn:
        sref, sab = R.bn_dgrad_sums_ref(h.double().reshape(G * P, 1, 1, Cin), zin.reshape(G * P, 1, 1, Cin), vin, G)
        E.sums_check(sm, sref, sab, P, rid + " sums")
        assert torch.equal(sm, sm2)
    record(rid, q)


def test_conv_bwd_data_dual_cout_limit():
    """Cout = 512 is served, Cout = 520 is refused with ADAMML_EUNSUPPORTED and writes nothing"""
    assert lib().adamml_conv_bwd_data_dual_supported(byref(ConvDesc(1, 64, 1, 128, 64, 1, 512, 1, 1, 1, 0, 1, 0, 0, 1, 0))) == 1
    P, Cin, Cout = 64, 128, 520
    d = ConvDesc(1, P, 1, Cin, P, 1, Cout, 1, 1, 1, 0, 1, 0, 0, 1, 0)
    assert lib().adamml_conv_bwd_data_dual_supported(byref(d)) == 0
    g = GB.frozen(torch.zeros(P, Cout, dtype=torch.bfloat16))
    aff = GB.frozen(torch.zeros(3, Cout))
    wp = GB.frozen(torch.zeros(Cin, Cout, dtype=torch.bfloat16))
    dx, side = Guarded(P, Cin, torch.bfloat16), Guarded(P, Cout, torch.bfloat16)
    with pytest.raises(RuntimeError, match=r"\(-2\)"):
        call("adamml_conv_bwd_data_dual", byref(d), ptr(g), ptr(g), ptr(aff), ptr(side.t), ptr(wp), ptr(dx.t), 0, None, None, 0, None)
    torch.cuda.synchronize()
    assert untouched(dx) and untouched(side)


# ------------------------------------------------------------------------------------------------------------------------------- Gram
# (C, P, G, lazy, act): P = 1, 31, either side of the first split boundary of gram_splits (256 pixels per workgroup at least), full size
GRAM_ROWS = [(64, 1, 1, False, 0), (64, 31, 5, True, 2), (64, 256, 1, True, 1), (64, 257, 1, True, 1), (64, 141120, 1, True, 1),
             (128, 1, 5, True, 1), (128, 31, 1, False, 0), (128, 256, 1, True, 0), (128, 257, 5, True, 2), (128, 141120, 1, True, 1),
             (256, 1, 1, True, 2), (256, 31, 5, True, 1), (256, 256, 1, False, 0), (256, 257, 1, True, 0), (256, 141120, 1, True, 1)]


def gram_id(row):
    C, P, G, lazy, act = row
    return "gram-C%d-P%d-g%d-%s-act%d[gram_colsum_kernel<%d,%d>]" % (C, P, G, "lazy" if lazy else "plain", act, C, {64: 8, 128: 4, 256: 2}[C])


def run_gram(x, vec, act, P, C, G, rid):
    xd = GB.frozen(x)
    vd = GB.frozen(vec.reshape(-1)) if vec is not None else None

    def launch(outs, ws, nbytes):
        call("adamml_gram_colsum", ptr(xd), ptr(vd), ptr(vd[C:]) if vd is not None else None, 4 * C, act, ptr(outs[0].t), ptr(outs[1].t), P, C, G,
             ptr(ws), nbytes)

    need = lib().adamml_gram_colsum_workspace(P, C, G)
    (Gm, sv), _ = three(need, lambda: (Guarded(G * C, C, torch.float32), Guarded(G, C, torch.float32)), launch, rid)
    return Gm, sv


@pytest.mark.parametrize("row", GRAM_ROWS, ids=[gram_id(r) for r in GRAM_ROWS])
def test_gram_colsum(row):
    C, P, G, lazy, act = row
    rid = gram_id(row)
    assert lib().adamml_gram_colsum_supported(C) == 1
    s = F.seed_of(rid)
    x = E.plant_bounds(E.rand_bf16(G * P, C, scale=3.0 if act == 2 else 1.5, offset=1.0 if act == 2 else 0.0, seed=s))
    vec = E.bn_vectors(G, C, s + 1, act) if lazy else None
    Gm, sv = run_gram(x, vec, act, P, C, G, rid)
    vf = vec.reshape(-1) if lazy else None
    a = F.operand(x, vf, vf[C:] if lazy else None, act if lazy else 0, G, 4 * C if lazy else 0)
    q = F.gram_check(Gm.check(rid).cpu().reshape(G, C, C), sv.check(rid + " s").cpu(), a, rid)
    record(rid, q)


@pytest.mark.parametrize("Cin,Cout", [(64, 256), (128, 512)])
def test_gram_stats(Cin, Cout):
    """W s and diag(W G W^T) in float64 from a float32 G, s: group 0 has a G whose diagonal dominates by 10^4 (no cancellation: every term
    w_i^2 G_ii is positive), group 1 the rank-one-dominated Gram matrix of all-positive inputs (W G W^T cancels for the rows of W with
    mixed signs; the first 8 rows of W are non-negative: no cancellation there either)"""
    rid = "gram-stats-%dto%d[gram_stats_kernel]" % (Cin, Cout)
    s = F.seed_of(rid)
    w = F.weight(Cout, Cin, s)
    w[:8] = w[:8].abs()
    g = F.gen(s + 1)
    off = torch.randn(Cin, Cin, generator=g)
    G0 = (off + off.t()) * 0.5 + torch.diag(1e4 * (torch.rand(Cin, generator=g) + 1.0))
    a = (torch.randn(4000, Cin, generator=g) * 0.3 + 2.0).clamp_min(0)
    G1 = a.double().t() @ a.double()
    Gm = torch.stack([G0, ((G1 + G1.t()) * 0.5).float()]).float()          # (exactly symmetric: the kernel reads G by columns)
    sv = torch.stack([torch.randn(Cin, generator=g) * 50, a.sum(0)]).float()
    out = GB.out((4 * Cout,), torch.float64)
    wp, Gd, sd = pack(w4(w), Cin, 0), GB.frozen(Gm), GB.frozen(sv)
    call("adamml_gram_stats", ptr(wp), ptr(Gd), ptr(sd), ptr(out), Cout, Cin, 2)
    GB.check(rid)
    ref, tol = F.gram_stats_ref(w, Gm, sv)
    q = F.ratio(out.cpu().reshape(2, 2 * Cout), ref, tol)
    assert q <= 1.0, "%s: max err/tol %.3g" % (rid, q)
    cancel = ref[1, Cout:].abs() / (tol[1, Cout:] / ((Cin + F.GRAM_STATS_OPS) * E.U64))
    assert cancel[8:].min() < 0.2 and cancel[:8].min() > 0.999 and (ref[0, Cout:].abs() / (tol[0, Cout:] / ((Cin + F.GRAM_STATS_OPS) * E.U64))).min() > 0.99
    record(rid, q)


# -------------------------------------------------------------------------------------------------- temporal pool backward + product
TPB_ROWS = [(1, 49, 5, True), (2, 169, 3, False), (3, 784, 1, True), (1, 16, 1, False)]      # (clips, Q, G, lazy a): T = 8, C = 256, Cin = 64


def tpb_id(r):
    """<T, Cin, waves, ALLFULL>: the launcher picks ALLFULL when Q % 16 == 0 (no partial 16-pixel block)"""
    return "tpb-clips%d-Q%d-g%d-%s[tpool_bwd_prod_kernel<8,64,4,%s>]" % (r[0], r[1], r[2], "lazy" if r[3] else "plain", "true" if r[1] % 16 == 0 else "false")


@pytest.mark.parametrize("row", TPB_ROWS, ids=[tpb_id(r) for r in TPB_ROWS])
def test_temporal_pool_bwd_code_prod(row):
    clips, Q, G, lazy = row
    rid = tpb_id(row)
    T, C, Cin, To = 8, 256, 64, 4
    assert lib().adamml_temporal_pool_bwd_code_prod_supported(T, C, Cin) == 1, "dispatch probe"
    s = F.seed_of(rid)
    rows, P = G * clips * To * Q, clips * T * Q
    gy = E.rand_bf16(rows, C, seed=s)
    code = torch.randint(0, 4, (rows, C), generator=F.gen(s + 1))
    assert all((code == k).any() for k in range(4))
    a = E.plant_bounds(E.rand_bf16(G * P, Cin, scale=1.5, seed=s + 2))
    av = E.bn_vectors(G, Cin, s + 3) if lazy else None
    avd = GB.frozen(av.reshape(-1)) if lazy else None
    gyd, cd, ad = GB.frozen(gy), GB.frozen(E.pack_codes(code)), GB.frozen(a)

    def launch(outs, ws, nbytes):
        call("adamml_temporal_pool_bwd_code_prod", ptr(gyd), ptr(cd), ptr(outs[0].t), ptr(outs[2]), ptr(ad), ptr(avd),
             ptr(avd[Cin:]) if lazy else None, 4 * Cin if lazy else 0, 1 if lazy else 0, ptr(outs[1].t), ptr(ws), nbytes, clips, T, Q, C, Cin, G)

    need = lib().adamml_temporal_pool_bwd_code_prod_workspace(clips, T, Q, C, Cin, G)
    (g2, prod, sa), _ = three(need, lambda: (Guarded(G * P, C, torch.bfloat16), Guarded(G * C, Cin, torch.float32), stat_acc(G, C)), launch, rid)
    avf = av.reshape(-1) if lazy else None
    ao = F.operand(a, avf, avf[Cin:] if lazy else None, 1 if lazy else 0, G, 4 * Cin if lazy else 0)
    g2r, pr, pa, n = F.tpool_bwd_code_prod_ref(gy.reshape(G * clips * To, Q, C), code.reshape(G * clips * To, Q, C), ao, T, G)
    h = g2.check(rid).cpu()
    assert torch.equal(h.double().reshape(g2r.shape), g2r), rid + ": g2 is not the routed gradient rounded once"
    q = F.prod_check(prod.check(rid + " prod").cpu().reshape(G, C, Cin), pr, pa, n, rid + " prod")
    F.res_sums_check(collapse(sa, C, G), h, None, None, G, rid + " sums")
    record(rid, q)


# ------------------------------------------------------------------------------------------------------------------------------- packs
PACK_SPECS = [(64, 3, 7, 7, 0), (24, 144, 1, 1, 0), (24, 144, 1, 1, 1), (200, 10, 3, 3, 0), (200, 10, 3, 3, 1), (96, 1, 3, 3, 2),
              (2048, 512, 1, 1, 0), (2048, 512, 1, 1, 1), (8, 20, 1, 1, 1), (130, 36, 1, 1, 0)]


def test_weight_packs_follow_the_index_map():
    """adamml_pack_conv_weight and adamml_pack_conv_weights_batched (blocks of adamml_pack_block_elems elements) against the numpy index
    map, bit for bit; Cin not a multiple of 8 (padded channels zero), Cout and element counts not multiples of the block"""
    from adamml_amd.runtime import pad8
    epb = lib().adamml_pack_block_elems()
    assert epb > 0
    ws, singles, batched, refs, specs = [], [], [], [], []
    for i, (cout, cin, kh, kw, mode) in enumerate(PACK_SPECS):
        w = torch.randn(cout, cin, kh, kw, generator=F.gen(100 + i))
        cp = pad8(cin)
        ref = F.pack_ref(w, cp, mode)
        n = ref.numel()
        s = Guarded(n, 1, ref.dtype)
        b = Guarded(n, 1, ref.dtype)
        wd = GB.frozen(w)
        call("adamml_pack_conv_weight", ptr(wd), ptr(s.t), cout, 1 if mode == 2 else cin, 1 if mode == 2 else cp, kh, kw, mode)
        ws.append(wd); singles.append(s); batched.append(b); refs.append(ref); specs.append((cout, cin, kh, kw, mode, cp))
    assert any(r.numel() % epb for r in refs)
    rows, blk = F.pack_table(specs, [(w.data_ptr(), b.t.data_ptr()) for w, b in zip(ws, batched)], epb)
    table = GB.frozen(torch.tensor(rows, dtype=torch.int64))
    call("adamml_pack_conv_weights_batched", ptr(table), len(rows), blk)
    for spec, s, b, ref in zip(PACK_SPECS, singles, batched, refs):
        hs, hb = s.check("pack %s" % (spec,)).cpu().reshape(ref.shape), b.check("batched pack %s" % (spec,)).cpu().reshape(ref.shape)
        assert torch.equal(hs, ref), "pack %s" % (spec,)
        assert torch.equal(hb, ref), "batched pack %s" % (spec,)


# ----------------------------------------------------------------------------------------------------------- non-finite operands
NAN_FWD = [r for r in F.FADD_ROWS if r["id"].startswith(("tile-64to256-relu-lazyg-g3[", "l2-P4097-relu6-lazy0-g3["))]


def poison(row, op):
    """a NaN in x (one pixel, one channel), in idn (one element) and in the shift of one BatchNorm channel of group 0"""
    P = row["P"]
    op["x"][P // 2, 5] = NAN
    op["idn"][P // 3, 40] = NAN
    op["vec"][0, 1, 9] = NAN
    return op


@pytest.mark.parametrize("row", NAN_FWD, ids=[r["id"] for r in NAN_FWD])
def test_conv_fwd_bn_add_propagates_nan(row):
    G, P, Cout = row["G"], row["P"], row["Cout"]
    op = poison(row, F.fadd_operands(row))
    r = F.fadd_reference(row, op)
    a = FwdArgs(row, op, 1, P, 1)
    assert lib().adamml_conv_fwd_bn_add_streams(byref(a.d)) == row["stream"]
    out = Guarded(G * P, Cout, torch.bfloat16)
    call("adamml_conv_fwd_bn_add", *a.head, ptr(out.t), None)
    finite_pattern_matches(out.check(row["id"], written=False).cpu().reshape(r["ref"].shape), r["ref"], row["id"] + " NaN")


def test_conv_fwd_bn_add_next_propagates_nan():
    row = F.NEXT_ROWS[1]
    G, P, Cout, Cn = row["G"], row["P"], row["Cout"], 64
    op = poison(row, F.fadd_operands(row))
    r = F.fadd_reference(row, op)
    a = FwdArgs(row, op, 1, P, 1)
    wn = F.weight(Cn, Cout, 5)
    out, y = Guarded(G * P, Cout, torch.bfloat16), Guarded(G * P, Cn, torch.bfloat16)
    wnp = pack(w4(wn), Cout, 0)
    call("adamml_conv_fwd_bn_add_next", *a.head, ptr(out.t), None, ptr(wnp), ptr(y.t), None)
    GB.unwritten_ok(y.t)                                                 # (NaN is what the row expects, in y_next too)
    finite_pattern_matches(out.check(row["id"], written=False).cpu().reshape(r["ref"].shape), r["ref"], row["id"] + " NaN")
    yr = r["ref"] @ wn.double().t()                      # (a NaN of the block output reaches every next-conv channel of its pixel)
    finite_pattern_matches(y.check(row["id"], written=False).cpu().reshape(yr.shape), yr, row["id"] + " NaN y_next")


@pytest.mark.parametrize("row", [RES_ROWS[0], RES_ROWS[2], RES_ROWS[8]], ids=[RES_ROWS[i]["id"] for i in (0, 2, 8)])
def test_conv_bwd_data_res_propagates_nan(row, monkeypatch):
    """a NaN in dz (a whole pixel of the gradient) and in the identity-path gradient (one element): non-finite exactly where the mask
    passes the gradient -- act' selects, as torch's threshold backward does: a masked element is 0, not NaN * 0"""
    setenv(monkeypatch, row["env"], "ADAMML_RES_PROD_STREAM")
    G, P, C = row["G"], row["P"], row["C"]
    op = res_operands(row)
    op["dz"][P // 2, 3] = NAN
    op["dx_in"][P // 3, 17] = NAN
    op["m"][0, P // 3, 17] = 1.0
    op["res_out"][P // 3, 17] = 1.0
    op["bits"] = F.pack_bits(op["m"].bool())
    dx, _, _ = run_res(row, op, finite=False)
    ref = F.res_ref(F.gview(op["dz"].double(), G), op["w"], torch.ones_like(op["m"]), F.gview(op["dx_in"], G))[0]
    ref = torch.where(op["m"] > 0, ref, torch.zeros_like(ref))
    finite_pattern_matches(dx.check(row["id"], written=False).cpu().reshape(ref.shape), ref, row["id"] + " NaN")


# ------------------------------------------------------------------------------------------------------------------------------- chain
def test_bottleneck_tail_chain_gram_stats_finalize_fused_conv():
    """gram_colsum -> gram_stats -> bn_finalize -> conv_fwd_bn_add, as adamml_amd/runtime.py runs a bottleneck tail in training, against
    the float64 train-mode relu(BN(W a) + idn) of the same bf16 operands.  Bound: the model of the last kernel at the true BatchNorm
    vectors + the first-order propagation of the statistics' error into scale and shift (F.chain_reference), |z| e_scale + e_shift,
    as `extra`; the vectors themselves are held to that propagated bound."""
    rid = "chain-64to256-g3[gram_colsum+gram_stats+bn_finalize+conv_gemm_kernel<64,FADD,EID,LZF>]"
    G, P, Cin, Cout, eps = 3, 2000, 64, 256, 1e-5
    row = dict(id=rid, G=G, P=P, Cin=Cin, Cout=Cout, in_act=1, act=1, idn="plain")
    op = F.fadd_operands(row)
    s = F.seed_of(rid)
    op["w"] = F.weight(Cout, Cin, s + 2)                       # (no planted channels: a zero row has zero variance)
    gamma = (torch.rand(Cout, generator=F.gen(s + 8)) + 0.5).float()
    beta = (torch.randn(Cout, generator=F.gen(s + 9)) * 0.3).float()
    a = FwdArgs(row, op, 1, P, 1)
    need = lib().adamml_gram_colsum_workspace(P, Cin, G)
    assert need > 0
    ws = GB.workspace(need)
    Gm, sv = GB.out((G, Cin, Cin), torch.float32), GB.out((G, Cin), torch.float32)
    call("adamml_gram_colsum", ptr(a.x), ptr(a.xv), ptr(a.xv[Cin:]), 4 * Cin, 1, ptr(Gm), ptr(sv), P, Cin, G, ptr(ws), need)
    GB.check(rid + " gram_colsum")
    Gm, sv = GB.frozen(Gm), GB.frozen(sv)                                # (each kernel's output is the next one's read-only operand)
    sums = GB.out((G, 2 * Cout), torch.float64)
    call("adamml_gram_stats", ptr(a.wp), ptr(Gm), ptr(sv), ptr(sums), Cout, Cin, G)
    GB.check(rid + " gram_stats")
    sums = GB.frozen(sums)
    vec = GB.out((G, 4, Cout), torch.float32)
    gd, bd = GB.frozen(gamma), GB.frozen(beta)
    call("adamml_bn_finalize", ptr(sums), 1, G, float(P), ptr(gd), ptr(bd), None, None, 0.1, eps, ptr(vec), Cout)
    GB.check(rid + " bn_finalize")
    vec = GB.frozen(vec)
    out = Guarded(G * P, Cout, torch.bfloat16)
    head = list(a.head)
    head[5] = ptr(vec)
    call("adamml_conv_fwd_bn_add", *head, ptr(out.t), None)
    ch = F.chain_reference(row, op, gamma, beta, eps)
    qv = F.ratio(vec.cpu(), ch["vec"], ch["vec_tol"])
    assert qv <= 1.0, "%s: BatchNorm vectors max err/tol %.3g" % (rid, qv)
    q = F.ratio(out.check(rid).cpu().reshape(ch["ref"].shape), ch["ref"], ch["tol"])
    assert q <= 1.0, "%s: max err/tol %.3g" % (rid, q)
    record(rid, max(q, qv))
