"""CPU-only checks (no GPU, no reference): the C-ABI library loads and exports every declared symbol, the model
registry reproduces the reference state_dict contract, the MAC counts of the stage plan match the constants in the
reference (utils/utils.py:512-523), and the product path refuses to run without a GPU."""
import ctypes
import gzip
import json
import os
import re

import pytest
import torch

import __graft_entry__ as ge
from adamml_amd import abi
from tests.golden_cases import CASES, CH
from tests.oracle_harness import manifest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    ge.build()
    return ge.LIB


def test_library_exports_every_declared_symbol(built):
    declared = set(abi.FUNCTIONS)
    assert len(declared) >= 28
    lib = ctypes.CDLL(built)
    for sym in sorted(declared):
        assert hasattr(lib, sym), "missing export " + sym
    from adamml_amd import hip
    hip.load()
    assert set(hip.SIGNATURES) <= declared
    assert lib.adamml_version() >= 100
    # ... and nothing else: the dynamic symbol table IS the C ABI (-fvisibility=hidden + csrc/exports.map; round 4 also exported 40
    # kernel handles and device stubs)
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", built], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert exported == declared, sorted(exported ^ declared)
    # the switch of earlier versions is accepted both ways and changes nothing (round-4 advisor finding)
    assert lib.adamml_set_deterministic(1) == 0 and lib.adamml_set_deterministic(0) == 0 and lib.adamml_get_deterministic() == 1


# entry points no test module has to name, with the reason (everything else declared in the header must appear in a tests/test_*.py)
ABI_TEST_EXEMPT = {
    "adamml_last_error_string": "query: hip.call reads it on every failing launch",
    "adamml_plan_run": "plan plumbing: every model row replayed through adamml_amd/plan.py, bit for bit against eager (tests/test_launch_plan_rows_gpu.py, "
                       "tests/test_launch_plan_gpu.py); its records decoded against the eager launch list (tests/test_launch_plan_cpu.py)",
    "adamml_plan_events_create": "plan plumbing: the weight-gradient stream rows of tests/test_launch_plan_rows_gpu.py replay through its events",
    "adamml_plan_events_destroy": "plan plumbing: runs when a plan of tests/test_launch_plan_rows_gpu.py is dropped (the eviction scenario)",
}


def test_every_declared_entry_point_is_named_by_a_test_module():
    """A kernel entry point the suite never calls by name is a gap: every function of include/adamml_hip.h is called in some tests/test_*.py,
    or is in ABI_TEST_EXEMPT with its reason (the error string, plan plumbing); the exemption list holds nothing stale.
    Dispatch probes are not exempt: a row asserts them (test_dispatch_probes_answer_as_documented for those no GPU row reads)."""
    import glob
    declared = set(abi.FUNCTIONS)
    text = "".join(open(f).read() for f in glob.glob(os.path.join(ROOT, "tests", "test_*.py")))
    text = re.sub(r"ABI_TEST_EXEMPT = \{.*?\n\}\n", "", text, flags=re.S)         # (the exemption list itself names nothing)
    # named = called: the name as a string literal (hip.call("name", ..)) or as an attribute of the loaded library (lib.name(..)); a mention
    # in a comment or a docstring does not count
    named = {s for s in declared if re.search(r"[\"']%s[\"']|\.%s\b" % (s, s), text)}
    assert set(ABI_TEST_EXEMPT) <= declared, sorted(set(ABI_TEST_EXEMPT) - declared)
    assert not (set(ABI_TEST_EXEMPT) & named), "exempt although a test names it: %s" % sorted(set(ABI_TEST_EXEMPT) & named)
    missing = declared - named - set(ABI_TEST_EXEMPT)
    assert not missing, "entry points no test module names: %s" % sorted(missing)
    assert all(len(r) > 10 for r in ABI_TEST_EXEMPT.values())


# the modules that compare kernels with a float64 (or byte-exact integer) reference under a counted error model
CONFORMANCE_MODULES = ("test_conv_conformance_gpu.py", "test_elementwise_conformance_gpu.py", "test_abi_conformance_gpu.py",
                       "test_fused_conformance_gpu.py", "test_spectrogram_gpu.py", "test_jpeg_gpu.py", "test_video_gpu.py")
# size queries and dispatch probes compute nothing a float64 reference could check
CONFORMANCE_QUERY_SUFFIXES = ("_workspace", "_supported", "_streams")
# entry points that launch no kernel of their own, with the reason no conformance row names them (keys without the adamml_ prefix: the full
# name as a string literal would count as a call in test_every_declared_entry_point_is_named_by_a_test_module)
CONFORMANCE_EXEMPT = {
    "version": "plumbing: a constant (test_library_exports_every_declared_symbol reads it)",
    "last_error_string": "plumbing: hip.call reads it on every failing launch",
    "set_deterministic": "plumbing: accepted and ignored, there is one reduction mode (test_library_exports_every_declared_symbol)",
    "get_deterministic": "plumbing: always 1 (test_library_exports_every_declared_symbol)",
    "plan_run": "plan plumbing: replays recorded launches of entry points that have their own rows; the replay itself is compared with eager "
                "per model row (tests/test_launch_plan_rows_gpu.py, tests/test_launch_plan_gpu.py) and decoded on the host (tests/test_launch_plan_cpu.py)",
    "plan_events_create": "plan plumbing: the weight-gradient stream rows of tests/test_launch_plan_rows_gpu.py",
    "plan_events_destroy": "plan plumbing: the eviction scenario of tests/test_launch_plan_rows_gpu.py",
    "plan_num_entry_points": "plan plumbing: the length of the thunk table (test_launch_plan_thunks_are_in_sync_with_the_c_abi)",
}


# the conformance modules whose rows take every device buffer from tests/guarded.py
GUARDED_MODULES = CONFORMANCE_MODULES[:4]
# (module, line) -> why this line may create a device tensor outside tests/guarded.py
DEVICE_ALLOC_EXEMPT = {
    ("test_conv_conformance_gpu.py", "model.to(DEV).train()"): "the whole-network NaN row: the model owns its parameters, no buffer is handed to a kernel by the row",
    ("test_conv_conformance_gpu.py", "y = model(x.to(DEV))"): "the whole-network NaN row: the network input, consumed by the executor",
    ("test_elementwise_conformance_gpu.py", "g = torch.Generator(device=DEV).manual_seed(seed)"): "large rows: the generator of operands made on the device (0.3 - 0.6 GB)",
    ("test_elementwise_conformance_gpu.py", "t = (torch.randn(rows, C, generator=g, device=DEV) * scale + offset).to(torch.bfloat16)"):
        "large rows: the operand is made on the device and handed to guarded.frozen on the next line",
    ("test_elementwise_conformance_gpu.py",
     "out, ab = torch.zeros(G, 2 * C, dtype=torch.float64, device=DEV), torch.zeros(G, 2 * C, dtype=torch.float64, device=DEV)"):
        "large rows: accumulators of the float64 reference computed by torch on the device, no kernel of the library sees them",
}
DEVICE_ALLOC = re.compile(r"device\s*=\s*DEV|\.to\(DEV\)|\.cuda\(\)")


def test_guarded_modules_create_no_device_tensor_of_their_own():
    """In the four float64 conformance modules every buffer a kernel sees comes from tests/guarded.py (guard bands, frozen operands): no
    `device=DEV`, `.to(DEV)` or `.cuda()` in the module text but the lines of DEVICE_ALLOC_EXEMPT, which holds nothing stale"""
    assert len(GUARDED_MODULES) == 4 and all(m.endswith("_conformance_gpu.py") for m in GUARDED_MODULES)
    seen = set()
    for m in GUARDED_MODULES:
        text = open(os.path.join(ROOT, "tests", m)).read()
        assert re.search(r"^from tests\.guarded import |^from tests\.test_conv_conformance_gpu import .*\bGB\b", text, re.M), m + ": does not use tests/guarded.py"
        for no, line in enumerate(text.splitlines(), 1):
            if DEVICE_ALLOC.search(line):
                key = (m, line.strip())
                assert key in DEVICE_ALLOC_EXEMPT, "%s:%d creates a device tensor outside tests/guarded.py: %s" % (m, no, line.strip())
                seen.add(key)
    assert seen == set(DEVICE_ALLOC_EXEMPT), "stale exemptions: %s" % sorted(set(DEVICE_ALLOC_EXEMPT) - seen)
    assert all(len(r) > 10 for r in DEVICE_ALLOC_EXEMPT.values())


# workspace queries no guarded conformance module has to call, with the reason (keys without the adamml_ prefix, as CONFORMANCE_EXEMPT)
WORKSPACE_QUERY_EXEMPT = {
    "jpeg_decode_workspace": "the decoder clamps every workspace address by construction and tests/test_jpeg_gpu.py is byte-exact",
}


def test_every_workspace_query_is_called_by_a_guarded_conformance_module():
    """A workspace-size query nobody checks against what the kernel touches is a gap: every adamml_*_workspace of the header is called by
    name in one of the GUARDED_MODULES (whose rows allocate exactly the answer inside guard bands), or is in WORKSPACE_QUERY_EXEMPT"""
    queries = {n for n in abi.FUNCTIONS if n.endswith("_workspace")}
    assert len(queries) >= 9
    text = "".join(open(os.path.join(ROOT, "tests", m)).read() for m in GUARDED_MODULES)
    called = {q for q in queries if re.search(r"\.%s\(" % q, text)}
    exempt = {"adamml_" + k for k in WORKSPACE_QUERY_EXEMPT}
    assert exempt <= queries and not (exempt & called), sorted(exempt)
    assert not (queries - called - exempt), "workspace queries no guarded conformance module calls: %s" % sorted(queries - called - exempt)
    # and every call passes its answer on: no module sizes a workspace through the grow-only scratch of adamml_amd/hip.py
    assert not re.search(r"hip\.(wgrad_workspace|scratch)\(", text)
    assert all(len(r) > 10 for r in WORKSPACE_QUERY_EXEMPT.values())


def test_every_computing_entry_point_is_named_by_a_float64_conformance_module():
    """Being called by some test is not being checked: every function of include/adamml_hip.h that computes something -- everything but
    the size queries and dispatch probes (CONFORMANCE_QUERY_SUFFIXES) -- is called in one of the CONFORMANCE_MODULES, or is in
    CONFORMANCE_EXEMPT with its reason; the exemption list holds nothing stale (undeclared, a query, or named by a conformance module)."""
    declared = set(abi.FUNCTIONS)
    text = ""
    for m in CONFORMANCE_MODULES:
        path = os.path.join(ROOT, "tests", m)
        assert os.path.exists(path), "conformance module missing: " + m
        text += open(path).read()
    named = {s for s in declared if re.search(r"[\"']%s[\"']|\.%s\b" % (s, s), text)}
    queries = {s for s in declared if s.endswith(CONFORMANCE_QUERY_SUFFIXES)}
    exempt = {"adamml_" + k for k in CONFORMANCE_EXEMPT}
    assert exempt <= declared - queries, sorted(exempt - (declared - queries))
    assert not (exempt & named), "exempt although a conformance module names it: %s" % sorted(exempt & named)
    missing = declared - queries - named - exempt
    assert not missing, "entry points no float64 conformance module names: %s" % sorted(missing)
    assert all(len(r) > 10 for r in CONFORMANCE_EXEMPT.values())


def test_dispatch_probes_answer_as_documented(built):
    """The probes the runtime reads to label launches, on the shapes include/adamml_hip.h documents for them (host functions: no GPU)."""
    from ctypes import byref
    from adamml_amd import hip
    from adamml_amd.hip import ConvDesc
    lib = hip.load()

    def desc(H, cin, cout, k=1, stride=1, pad=0):
        return ConvDesc(8, H, H, cin, H // stride, H // stride, cout, k, k, stride, pad, 1, 1, 0, 1, 0)
    assert [lib.adamml_gram_colsum_supported(c) for c in (64, 128, 256, 96, 8, 512)] == [1, 1, 1, 0, 0, 0]
    l1, l2, l3 = desc(56, 64, 256), desc(28, 128, 512), desc(14, 256, 1024)
    assert lib.adamml_conv_fwd_bn_add_supported(byref(l1)) == 1 and lib.adamml_conv_fwd_bn_add_supported(byref(l2)) == 1
    assert lib.adamml_conv_fwd_bn_add_supported(byref(desc(56, 64, 64, 3, 1, 1))) == 0           # not 1x1
    assert lib.adamml_conv_fwd_bn_add_supported(byref(desc(56, 64, 256, 1, 2, 0))) == 0          # not stride 1
    for frames in (2, 4, 8):            # 0 = tile kernel, 1 = the 64 -> 256 streaming kernel, 2 = the 128 -> 512 wave-slice kernel
        assert [lib.adamml_conv_fwd_bn_add_tpool_streams(byref(d), frames) for d in (l1, l2, l3)] == [1, 2, 0]
    # the layer-1 shape of the product-fused residual data gradient: d->Cin == 256, d->Cout == 64, a_channels == 64
    assert lib.adamml_conv_bwd_data_res_prod_streams(byref(desc(56, 256, 64)), 64) == 1
    assert lib.adamml_conv_bwd_data_res_prod_streams(byref(desc(28, 512, 128)), 64) == 0
    assert lib.adamml_conv_bwd_data_res_prod_streams(byref(desc(56, 256, 64)), 32) == 0
    # ... from 4096 pixels per group on (8 x 22 x 22 = 3872, 8 x 23 x 23 = 4232), as adamml_conv_bwd_data_res_streams at the layer-2 shape
    assert [lib.adamml_conv_bwd_data_res_prod_streams(byref(desc(h, 256, 64)), 64) for h in (22, 23)] == [0, 1]
    assert [lib.adamml_conv_bwd_data_res_streams(byref(desc(h, 512, 128))) for h in (22, 23)] == [0, 1]
    # the two probes the conformance rows assert on their operands, on the host side of their predicates
    assert lib.adamml_gemm_f32_uses_mfma(4096, 64, 1, 8192, 64, 1, 64) == 1 and lib.adamml_gemm_f32_uses_mfma(4096, 64, 1, 8192, 64, 1, 62) == 0
    assert lib.adamml_gemm_f32_uses_mfma(4100, 64, 1, 8192, 64, 1, 64) == 0 and lib.adamml_gemm_f32_uses_mfma(4096, 1, 64, 8192, 64, 1, 64) == 0
    assert lib.adamml_clip_to_nhwc_four_pixel(4096, 8192, 6, 8, 6, 8, 4) == 1 and lib.adamml_clip_to_nhwc_four_pixel(4096, 8192, 6, 10, 6, 10, 4) == 0
    assert lib.adamml_clip_to_nhwc_four_pixel(4096, 8192, 6, 8, 6, 8, 8) == 0 and lib.adamml_clip_to_nhwc_four_pixel(4096, 8192, 6, 8, 3, 4, 4) == 0


def _namespace_scope_prototypes(src):
    """Names of the adamml_* functions DECLARED without a body at namespace scope of a C++ source (multi-line prototypes included):
    statements that end in `;` outside every brace other than those of a namespace or a linkage specification."""
    src = re.sub(r"//[^\n]*|/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r'"(?:\\.|[^"\\\n])*"', '""', src)
    src = re.sub(r"^[ \t]*#[^\n]*", "", src, flags=re.M)
    found, stmt, opened = [], "", []            # opened: per open brace, whether it is transparent (namespace / extern "C")
    for ch in src:
        if ch == "{":
            opened.append(all(opened) and re.search(r'(\bnamespace\b[\w\s:]*|\bextern\s*"")\s*$', stmt) is not None)
            stmt = ""
        elif ch == "}":
            opened.pop()
            stmt = ""
        elif ch == ";":
            m = re.match(r'\s*(?:extern\s*""\s*)?[\w\s\*&:<>]*?\b(adamml_\w+)\s*\(.*\)\s*$', stmt, flags=re.S)
            if all(opened) and m:
                found.append(m.group(1))
            stmt = ""
        else:
            stmt += ch
    assert not opened
    return found


def test_internal_launchers_are_declared_once_in_the_internal_header():
    """A launcher that one csrc/*.hip file defines and another calls is declared in csrc/conv_internal.h and nowhere else: no .hip file holds
    a bodiless declaration of an adamml_* function (a prototype of its own drifts from the definition unnoticed: with C++ linkage the
    mismatch compiles, links and fails when the library is loaded), and every .hip file that defines or calls a declared function includes
    the header."""
    import glob
    csrc = os.path.join(ROOT, "adamml_amd", "csrc")
    assert _namespace_scope_prototypes('namespace {\nint adamml_a(int x,\n  int y = 1);\n}\nextern "C" { int adamml_b(); }\n'
                                       'int adamml_c(int v) { return adamml_a(v); }\n// int adamml_d();\n') == ["adamml_a", "adamml_b"]
    declared = set(_namespace_scope_prototypes(open(os.path.join(csrc, "conv_internal.h")).read()))
    assert len(declared) >= 30, sorted(declared)
    sources = sorted(glob.glob(os.path.join(csrc, "*.hip")))
    assert len(sources) >= 20
    stray, missing, used = {}, [], set()
    for path in sources:
        src = open(path).read()
        name = os.path.basename(path)
        protos = _namespace_scope_prototypes(src)
        if protos:
            stray[name] = protos
        code = re.sub(r"//[^\n]*|/\*.*?\*/", " ", src, flags=re.S)
        names = set(re.findall(r"\b(adamml_\w+)\s*\(", code)) & declared
        used |= names
        if names and not re.search(r'^#include "conv_internal\.h"', src, flags=re.M):
            missing.append(name)
    assert not stray, "prototypes outside csrc/conv_internal.h: %s" % stray
    assert not missing, "files that define or call a function of csrc/conv_internal.h without including it: %s" % missing
    assert used == declared, "declared but neither defined nor called: %s" % sorted(declared - used)


def test_row_walk_helpers_live_in_one_header():
    """The thread map of the row-walking kernels (struct ChanMap), the channel bound MAXC and block_channel_publish are defined in
    csrc/rowwalk.h and in no csrc/*.hip (two copies of the thread map diverge unnoticed: each file compiles against its own), and every
    .hip file that uses one of them includes the header."""
    import glob
    csrc = os.path.join(ROOT, "adamml_amd", "csrc")
    strip = lambda src: re.sub(r"//[^\n]*|/\*.*?\*/", " ", src, flags=re.S)
    define = r"\bstruct\s+ChanMap\b\s*\{|\bconstexpr\s+int\s+MAXC\b|\bvoid\s+block_channel_publish\s*\("
    header = strip(open(os.path.join(csrc, "rowwalk.h")).read())
    assert len(re.findall(define, header)) == 3
    copies, missing, users = {}, [], 0
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip"))):
        src = open(path).read()
        code, name = strip(src), os.path.basename(path)
        found = re.findall(define, code)
        if found:
            copies[name] = found
        if re.search(r"\b(ChanMap|MAXC|block_channel_publish)\b", code):
            users += 1
            if not re.search(r'^#include "rowwalk\.h"', src, flags=re.M):
                missing.append(name)
    assert not copies, "row-walk helpers defined outside csrc/rowwalk.h: %s" % copies
    assert not missing, "files that use a row-walk helper without including csrc/rowwalk.h: %s" % missing
    assert users >= 3


WAVE_SLICE_HELPERS = ("wave_uniform", "lazy_lo", "lazy_hi", "fill_lazy_vec", "lazy8", "stage8", "unstage8", "tr_frag", "staged_outer_product",
                      "chunk_lane_fold", "persistent_blocks")


def wave_slice_hits(csrc):
    """What test_wave_slice_helpers_live_in_one_header counts in a csrc directory: (copies, missing includes, files that use a helper)"""
    import glob
    strip = lambda src: re.sub(r"//[^\n]*|/\*.*?\*/", " ", src, flags=re.S)
    define = r"\b(?:float|void|bf16x8|int)\s+(%s)\s*\(" % "|".join(WAVE_SLICE_HELPERS)
    # the idioms the helpers replace, under the names their copies had: the readfirstlane lambda, the private short-vector typedef, the
    # transpose-read lambda frag(base, row_bytes, blk), the private static_for, the per-file grid helpers
    idiom = (r"\bauto\s+uniform\s*=\s*\[|\btypedef\b[^;]*\bs16x4_\s*;|\bauto\s+frag\s*=\s*\[[^\]]*\]\s*\(\s*const\s+char\s*\*\s*base\b|"
             r"\bvoid\s+static_for_k\s*\(|\bint\s+(?:rps|fs)_blocks\s*\(")
    copies, missing, users = [], [], 0
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h"))):
        src = open(path).read()
        code, name = strip(src), os.path.basename(path)
        # (the one place the attribute may be named: adamml_raise_lds_limit in common.h)
        attr = len(re.findall(r"\bhipFuncAttributeMaxDynamicSharedMemorySize\b", code))
        if name == "common.h":
            body = re.search(r"\bint\s+adamml_raise_lds_limit\s*\([^)]*\)\s*\{(.*?)\n\}", code, flags=re.S)
            attr -= len(re.findall(r"\bhipFuncAttributeMaxDynamicSharedMemorySize\b", body.group(1))) if body else 0
        copies += [(name, "hipFuncAttributeMaxDynamicSharedMemorySize")] * attr
        if name == "waveslice.h" or not name.endswith(".hip"):
            continue
        copies += [(name, m.group(0).split("(")[0].strip()) for m in re.finditer(define, code)]
        copies += [(name, " ".join(m.group(0).split())[:40]) for m in re.finditer(idiom, code, flags=re.S)]
        if re.search(r"\b(%s)\s*[<(]" % "|".join(WAVE_SLICE_HELPERS), code):
            users += 1
            if not re.search(r'^#include "waveslice\.h"', src, flags=re.M):
                missing.append(name)
    return copies, missing, users


def test_wave_slice_helpers_live_in_one_header():
    """The idioms of the barrier-free wave-slice streaming kernels -- wave-uniform clamp bounds, the lazy-operand fill and transform, the
    8-byte staging accesses, the transpose-read fragment and the outer product over two staged tiles, the chunk-lane fold, the persistent
    grid -- are defined in csrc/waveslice.h and in no csrc/*.hip (these kernels promise the tile kernels' bits through "same rounding
    points, same epilogue expression": a copy that drifts breaks that unnoticed); no .hip keeps one of the old copies (a `uniform`
    readfirstlane lambda, an s16x4_ typedef, a `frag` transpose-read lambda, static_for_k, rps_blocks / fs_blocks);
    hipFuncAttributeMaxDynamicSharedMemorySize is named in csrc only inside common.h's adamml_raise_lds_limit; every .hip that uses a helper
    includes the header.  (On the csrc of the commit before the header this finds 33 hits: profiles/r11_bench_parent_vs_waveslice.txt.)"""
    csrc = os.path.join(ROOT, "adamml_amd", "csrc")
    strip = lambda src: re.sub(r"//[^\n]*|/\*.*?\*/", " ", src, flags=re.S)
    header = strip(open(os.path.join(csrc, "waveslice.h")).read())
    for name in WAVE_SLICE_HELPERS:
        assert len(re.findall(r"\b(?:float|void|bf16x8|int)\s+%s\s*\(" % name, header)) == 1, name
    common = strip(open(os.path.join(csrc, "common.h")).read())
    assert len(re.findall(r"\bint\s+adamml_raise_lds_limit\s*\(", common)) == 1
    assert len(re.findall(r"\bvoid\s+static_for\s*\(", common)) == 1
    copies, missing, users = wave_slice_hits(csrc)
    assert not copies, "wave-slice idioms outside csrc/waveslice.h (or the LDS attribute outside adamml_raise_lds_limit): %s" % copies
    assert not missing, "files that use a wave-slice helper without including csrc/waveslice.h: %s" % missing
    assert users >= 7


def test_environment_switch_registry_matches_the_code():
    """DESIGN.md appendix B is the complete registry of the ADAMML_* variables the product reads: the names adamml_amd/**/*.py takes from
    os.environ plus the names adamml_amd/csrc/* passes to getenv are exactly its operational and test-hook groups (the infrastructure
    group holds what only bench.py, the tests and tools/ read)."""
    import glob
    pkg = os.path.join(ROOT, "adamml_amd")
    read = set()
    for f in glob.glob(os.path.join(pkg, "**", "*.py"), recursive=True):
        for line in open(f):
            if "os.environ" in line:
                read |= set(re.findall(r"[\"'](ADAMML_[A-Z0-9_]+)[\"']", line))
    for f in glob.glob(os.path.join(pkg, "csrc", "*")):
        read |= set(re.findall(r"getenv\(\s*\"(ADAMML_[A-Z0-9_]+)\"", open(f).read()))
    doc = open(os.path.join(ROOT, "DESIGN.md")).read()
    groups = {}
    for part in doc[doc.index("## Appendix B"):].split("\n### ")[1:]:
        title, _, body = part.partition("\n")
        rows = [ln.split("|")[1] for ln in body.splitlines() if ln.startswith("| `ADAMML_")]
        groups[title.strip()] = {n for cell in rows for n in re.findall(r"`(ADAMML_[A-Z0-9_]+)`", cell)}
    assert set(groups) == {"Operational", "Test hooks", "Infrastructure"}, sorted(groups)
    assert all(groups.values())
    assert not (groups["Operational"] & groups["Test hooks"]) and not ((groups["Operational"] | groups["Test hooks"]) & groups["Infrastructure"])
    listed = groups["Operational"] | groups["Test hooks"]
    assert read == listed, "read but not listed: %s; listed but not read: %s" % (sorted(read - listed), sorted(listed - read))


def _build(c):
    from adamml_amd import adamml
    mod = c["modality"]
    return adamml(groups=c["groups"], modality=mod, input_channels=[CH[m] for m in mod], num_segments=c["S"], rng_policy=False,
                  rng_threshold=0.5, causality_modeling=c.get("causality", "lstm"), num_classes=31, depth=50,
                  without_t_stride=False, dropout=0.5, pooling_method="max", fusion_point="logits", unimodality_pretrained=[],
                  learnable_lf_weights=True)


@pytest.mark.parametrize("name", ["adamml_rgb_sound", "adamml_rgb_sound_nolstm", "adamml_rgb_flow_rgbdiff", "adamml_4mod"])
def test_state_dict_contract_matches_reference(name):
    c = CASES[name]
    sd = _build(c).state_dict()
    man = manifest(c)
    assert list(sd.keys()) == list(man.keys())
    for k in man:
        assert tuple(sd[k].shape) == tuple(man[k].shape) and sd[k].dtype == man[k].dtype, k
    if name == "adamml_rgb_sound":
        assert len(sd) == 1271            # 644 params + 627 buffers


def test_unimodal_registry_and_surface():
    import argparse
    from adamml_amd import build_model, MODEL_TABLE
    assert set(MODEL_TABLE) == {"adamml", "resnet", "sound_mobilenet_v2"}
    ns = argparse.Namespace(backbone_net="adamml", groups=8, modality=["rgb", "sound"], input_channels=[3, 1], num_segments=5,
                            rng_policy=False, rng_threshold=0.5, causality_modeling="lstm", num_classes=31, depth=50,
                            without_t_stride=False, dropout=0.5, pooling_method="max", fusion_point="logits",
                            unimodality_pretrained=[], learnable_lf_weights=True, dataset="kinetics-sounds", dense_sampling=False,
                            frames_per_group=1, lr_scheduler="multisteps", sync_bn=True, batch_size=72, prefix="", epochs=20,
                            extra_flag_ignored=123)
    model, arch = build_model(ns)
    assert arch == ("kinetics-sounds-rgb-sound-adamml-j_mobilenet_v2-lstm-joint_resnet-50_mobilenet_v2-logits-llf-ts-max-f8"
                    "-multisteps-syncbn-bs72-e20")
    assert model.mean("rgb") == [0.485, 0.456, 0.406] and model.mean("sound") == [0.5]
    assert model.policy_net.temperature == 5.0
    model.decay_temperature()
    assert abs(model.policy_net.temperature - 5.0 * 0.965) < 1e-9
    model.freeze_policy_net()
    assert not model.update_policy_net and not any(p.requires_grad for p in model.policy_net.parameters())
    model.unfreeze_policy_net()
    model.freeze_main_net()
    assert not model.update_main_net and all(p.requires_grad for p in model.policy_net.parameters())
    n_pol = sum(p.numel() for p in model.policy_net.parameters())
    n_main = sum(p.numel() for p in model.main_net.parameters())
    assert round((n_pol + n_main) / 1e6, 2) == 42.09       # 42.09 M parameters


def test_mac_counts_match_reference_constants():
    """utils/utils.py:512-523 hard-codes per-segment MAC counts; the conv/linear layers of our containers reproduce them."""
    from adamml_amd.resnet import ResNet
    from adamml_amd.sound_mobilenet_v2 import MobileNetV2 as SoundNet
    from adamml_amd.policy_net import MobileNetV2 as PolicyNet

    def macs_resnet(cin):
        net = ResNet(50, 8, 31, input_channels=cin)
        t, h = 8, 224
        total = 8 * (112 * 112) * 64 * 49 * cin
        h = 56
        inpl = 64
        for li, (planes, layer) in enumerate(zip((64, 128, 256, 512), (net.layer1, net.layer2, net.layer3, net.layer4))):
            for b in layer:
                s = b.stride
                total += t * h * h * inpl * planes
                ho = h // s
                total += t * ho * ho * planes * planes * 9
                total += t * ho * ho * planes * planes * 4
                if b.downsample is not None:
                    total += t * ho * ho * inpl * planes * 4
                h = ho
                inpl = planes * 4
            if li < 3:
                t = max(1, t // 2)
        return total                      # the reference constants count convolutions only (no FC)

    assert macs_resnet(3) == 14135984128
    assert macs_resnet(10) == 16338911232

    def macs_mbv2(net, h, t, cin, plans, last_c, policy):
        total = t * (h // 2) ** 2 * 32 * 9 * cin
        h //= 2
        for bp in plans:
            if bp.tpool:
                t = t // 2
            if bp.pw is not None:
                total += t * h * h * bp.pw[0].cin_true * bp.pw[0].cout
            s = bp.dw[0].stride
            h = (h + 2 - 3) // s + 1
            total += t * h * h * bp.dw[0].cout * 9
            total += t * h * h * bp.pwl[0].cin_true * bp.pwl[0].cout
        total += t * h * h * last_c[0] * last_c[1]
        return total

    snd = SoundNet(num_classes=31, input_channels=1)
    assert macs_mbv2(snd, 256, 1, 1, snd._plans, (320, 1280), False) == 381739008
    pol = PolicyNet(num_frames=4, input_channels=3)
    assert macs_mbv2(pol, 160, 4, 3, pol._plans, (320, 1280), True) == 375446400
    # (the reference's rgbdiff constant 909 283 200 is not reproduced by its own 4-frame x 15-channel policy net --
    #  that architecture gives 463 920 000 -- so it is not asserted)


def test_product_path_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from adamml_amd.resnet import resnet
    m = resnet(depth=50, num_classes=31, without_t_stride=False, groups=8, dropout=0.5, pooling_method="max", input_channels=3,
               imagenet_pretrained=False)
    with pytest.raises(RuntimeError, match="no CPU"):
        m(torch.zeros(1, 24, 64, 64))


def test_unsupported_options_raise_like_the_reference():
    from adamml_amd.joint_resnet_mobilenetv2 import JointResNetMobileNetV2
    with pytest.raises(ValueError, match="only support logits mode"):
        JointResNetMobileNetV2(50, 8, ["rgb"], 31, input_channels=[3], fusion_point="fc2")
    from adamml_amd.runtime import temporal_pool, NetRT, Lazy
    with pytest.raises(ValueError, match="only support avg or max"):
        temporal_pool(NetRT(), Lazy(torch.zeros(8, 1, 1, 8, dtype=torch.bfloat16)), 8, "median")


def test_interleaver_is_deterministic_round_robin_and_propagates_errors():
    """adamml_amd.interleave: jobs advance one yield point per turn in fixed order (the property that keeps the collective
    sequence identical on every rank), results come back in job order, grad mode is inherited, exceptions are re-raised."""
    import torch
    from adamml_amd import interleave
    log = []

    def job(name, n):
        def f():
            for i in range(n):
                log.append((name, i, torch.is_grad_enabled()))
                interleave.yield_point()
            return name * 2
        return f

    with torch.no_grad():
        res = interleave.run_interleaved([(job("a", 3), None), (job("b", 1), None), (job("c", 2), None)], None)
    assert res == ["aa", "bb", "cc"]
    assert [(n, i) for n, i, _ in log] == [("a", 0), ("b", 0), ("c", 0), ("a", 1), ("c", 1), ("a", 2)]
    assert not any(g for _, _, g in log)
    interleave.yield_point()                     # a no-op outside a job

    def boom():
        interleave.yield_point()
        raise ValueError("boom")
    with pytest.raises(ValueError):
        interleave.run_interleaved([(job("x", 2), None), (boom, None)], None)


def test_optimizer_state_interchanges_with_torch_optim():
    """Checkpoint interchange (train_adamml.py:296-301, 373-383): the flat optimizers save torch.optim's per-parameter
    layout and load it back, so `optimizer.load_state_dict(checkpoint['optimizer'])` works in both directions."""
    import torch.nn as nn
    from adamml_amd.backbone import FlatBuffers
    from adamml_amd.optim import FlatSGD, FlatAdam
    torch.manual_seed(0)
    net = nn.Sequential(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4), nn.Linear(4, 2))
    fb = FlatBuffers(net)
    fb.ensure(torch.device("cpu"))
    # ours -> torch
    sgd = FlatSGD(fb, lr=0.05, momentum=0.9, weight_decay=1e-4)
    sgd.mom, sgd.steps = torch.randn_like(fb.flat), 3
    ref = torch.optim.SGD(net.parameters(), lr=0.01, momentum=0.9)
    ref.load_state_dict(sgd.state_dict())
    assert ref.param_groups[0]["lr"] == 0.05 and ref.param_groups[0]["weight_decay"] == 1e-4
    off = 0
    for p in net.parameters():
        assert torch.equal(ref.state[p]["momentum_buffer"].reshape(-1), sgd.mom[off:off + p.numel()])
        off += p.numel()
    # torch -> ours (a real torch step creates the state)
    for p in net.parameters():
        p.grad = torch.randn_like(p)
    ref.step()
    sgd2 = FlatSGD(fb, lr=0.01)
    sgd2.load_state_dict(ref.state_dict())
    assert sgd2.lr == 0.05 and sgd2.steps == 1
    assert torch.equal(sgd2.mom, torch.cat([ref.state[p]["momentum_buffer"].reshape(-1) for p in net.parameters()]))
    adam = torch.optim.Adam(net.parameters(), lr=1e-3, weight_decay=5e-4)
    adam.step()
    adam.step()
    fa = FlatAdam(fb, lr=1.0)
    fa.load_state_dict(adam.state_dict())
    assert fa.steps == 2 and fa.lr == 1e-3 and fa.weight_decay == 5e-4
    assert torch.equal(fa.v, torch.cat([adam.state[p]["exp_avg_sq"].reshape(-1) for p in net.parameters()]))
    adam2 = torch.optim.Adam(net.parameters(), lr=1.0)
    adam2.load_state_dict(fa.state_dict())
    for p in net.parameters():
        assert torch.equal(adam2.state[p]["exp_avg"], adam.state[p]["exp_avg"]) and float(adam2.state[p]["step"]) == 2.0
    # a checkpoint without optimizer state (or with another parameter list) leaves the state empty instead of mis-assigning it
    fa.load_state_dict({"param_groups": adam.state_dict()["param_groups"], "state": {}})
    assert fa.m is None and fa.steps == 0


def test_torch_library_ops_are_registered_with_fake_implementations():
    """SURVEY.md section 8b "who calls it": the backbone call and the leaf operators are torch.library custom ops (namespace
    `adamml`) with register_fake -- shapes / dtypes propagate under FakeTensorMode without a GPU and without the library."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    import adamml_amd.ops  # noqa: F401
    c = CASES["adamml_rgb_sound"]
    m = _build(c)
    for name in ("backbone_call", "clip_to_nhwc", "gemm_f32", "conv_fwd", "temporal_pool"):
        assert hasattr(torch.ops.adamml, name), name
    with FakeTensorMode():
        S, B = 3, 2
        y = torch.ops.adamml.backbone_call(torch.zeros(1), torch.empty(S * B * 8, 96, 96, 8, dtype=torch.bfloat16), [],
                                           m.main_net.nets[0]._handle, S, False)
        assert tuple(y.shape) == (S * B, 31) and y.dtype == torch.float32
        y = torch.ops.adamml.backbone_call(torch.zeros(1), torch.empty(S * B, 96, 96, 8, dtype=torch.bfloat16), [],
                                           m.main_net.nets[1]._handle, S, False)
        assert tuple(y.shape) == (S * B, 31)
        f = torch.ops.adamml.backbone_call(torch.zeros(1), torch.empty(S * B * 4, 160, 160, 8, dtype=torch.bfloat16), [],
                                           m.policy_net.joint_net.nets[0]._handle, S, False)
        assert tuple(f.shape) == (S * B, 1280)                       # 4 frames -> 2 -> 1 through the two temporal max-pools
        t = torch.ops.adamml.clip_to_nhwc(torch.empty(B, S * 8 * 3, 224, 224), S, 8, 3, 160, 160, 2)
        assert tuple(t.shape) == (S, B * 4, 160, 160, 8) and t.dtype == torch.bfloat16
        g = torch.ops.adamml.gemm_f32(torch.empty(5, 7), torch.empty(9, 7), torch.empty(9), 1, False, True)
        assert tuple(g.shape) == (5, 9)
        y = torch.ops.adamml.conv_fwd(torch.empty(4, 56, 56, 64, dtype=torch.bfloat16), torch.empty(128, 9 * 64, dtype=torch.bfloat16),
                                      None, None, None, 3, 3, 2, 1, 0, 1)
        assert tuple(y.shape) == (4, 28, 28, 128) and y.dtype == torch.bfloat16
        p = torch.ops.adamml.temporal_pool(torch.empty(2 * 8, 7, 7, 256, dtype=torch.bfloat16), 8, 0, 1)
        assert tuple(p.shape) == (2 * 4, 7, 7, 256)
    # the real implementations refuse CPU tensors (no fallback)
    with pytest.raises(RuntimeError):
        torch.ops.adamml.gemm_f32(torch.zeros(2, 2), torch.zeros(2, 2), None, 0, False, True)


def test_stock_ddp_wrap_switches_to_autograd_delivered_gradients():
    """The first forward that arrives THROUGH torch's DistributedDataParallel switches the backbones to delivering parameter
    gradients through autograd (so DDP's AccumulateGrad hooks fire) and detaches the flat .grad views; attribute probes
    (hasattr / dir / inspect.getmembers -- loggers, tracing tools) have no such side effect, a direct forward neither, and the
    flat optimizers refuse to step on a detached sub-network instead of silently leaving the weights untouched."""
    import inspect
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel
    from adamml_amd.optim import FlatSGD, FlatAdam
    m = _build(CASES["adamml_rgb_sound"])
    assert not hasattr(m, "_ddp_params_and_buffers_to_ignore")
    dir(m)
    inspect.getmembers(m)
    assert not any(n.expose_param_grads for n in m.backbones()) and not m._flat_main.detached
    x = [torch.zeros(1, 2 * 8 * 3, 64, 64), torch.zeros(1, 2, 64, 64)]
    with pytest.raises(RuntimeError):
        m(x)                                             # direct call: CPU tensors are refused, nothing switched
    assert not any(n.expose_param_grads for n in m.backbones()) and not m._flat_main.detached
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        ddp = DistributedDataParallel(m, find_unused_parameters=True)       # train_adamml.py:129
        assert not any(n.expose_param_grads for n in m.backbones())      # construction alone does not switch either
        with pytest.raises(RuntimeError):
            ddp(x)                                       # the forward reaches the module (and is refused: CPU tensors) ...
        assert all(n.expose_param_grads for n in m.backbones())          # ... through DDP: switched
        assert m._flat_main.detached and m._flat_policy.detached
        with pytest.raises(RuntimeError, match="delivered through autograd"):
            FlatSGD(m._flat_main, lr=0.1).step()
        with pytest.raises(RuntimeError, match="delivered through autograd"):
            FlatAdam(m._flat_policy, lr=0.1).step()
    finally:
        dist.destroy_process_group()


def test_lr_schedules_match_torch_schedulers():
    """train.LRSchedule (closed form, stepped with the epoch like train_adamml.py:499-500 `scheduler.step(epoch + 1)`... the
    reference builds StepLR / MultiStepLR / CosineAnnealingLR at train_adamml.py:259-270) gives torch's learning rates."""
    import warnings
    from adamml_amd.train import LRSchedule

    class Opt:
        lr = 0.0
    base, epochs, steps = 0.01, 20, [6, 12, 17]
    for kind in ("step", "multisteps", "cosine"):
        p = torch.nn.Parameter(torch.zeros(1))
        ref_opt = torch.optim.SGD([p], lr=base)
        ref = {"step": lambda: torch.optim.lr_scheduler.StepLR(ref_opt, steps[0]),
               "multisteps": lambda: torch.optim.lr_scheduler.MultiStepLR(ref_opt, steps),
               "cosine": lambda: torch.optim.lr_scheduler.CosineAnnealingLR(ref_opt, epochs, eta_min=0)}[kind]()
        o = Opt()
        mine = LRSchedule(o, kind, base, epochs, steps)
        for epoch in range(1, epochs + 1):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                ref_opt.step()
                ref.step()
            mine.step(epoch)
            assert abs(o.lr - ref_opt.param_groups[0]["lr"]) <= 1e-12 + 1e-9 * base, (kind, epoch, o.lr, ref_opt.param_groups[0]["lr"])
        # checkpointed state restores the same point (train_adamml.py:300-301)
        o2 = Opt()
        m2 = LRSchedule(o2, kind, base, epochs, steps)
        m2.load_state_dict(mine.state_dict())
        assert o2.lr == o.lr


def test_readme_commands_parse():
    """The five `python3 train_adamml.py ...` command lines of the reference's README (README.md:68,89,100,111,161; fixture
    tests/golden/readme_train_adamml_commands.txt) parse VERBATIM with the restated launcher's parser, every flag of opts.py:5-149
    exists with the reference's destination name, and the three concrete recipes resolve to the model configuration the reference
    derives from them (train_adamml.py:70-95)."""
    import shlex
    from adamml_amd import train
    lines = [l for l in open(os.path.join(ROOT, "tests", "golden", "readme_train_adamml_commands.txt")).read().splitlines()
             if l and not l.startswith("#")]
    assert len(lines) == 5
    parsed = []
    for l in lines:
        argv = shlex.split(l)
        assert argv[:2] == ["python3", "train_adamml.py"]
        parsed.append(train.arg_parser().parse_args(argv[2:]))
    tmpl, rgb_audio, rgb_flow, four, evaluate = parsed
    assert tmpl.multiprocessing_distributed and tmpl.workers == 96 and tmpl.datadir == ["/PATH/TO/MODALITY1", "/PATH/TO/MODALITY2"]
    assert rgb_audio.modality == ["rgb", "sound"] and rgb_audio.cost_weights == [1.0, 0.05] and rgb_audio.sync_bn
    assert rgb_audio.lr == 0.001 and rgb_audio.p_lr == 0.01 and rgb_audio.lr_scheduler == "multisteps" and rgb_audio.lr_steps == [10, 15]
    assert rgb_flow.modality == ["rgb", "flow", "rgbdiff"] and len(rgb_flow.datadir) == 3 and len(rgb_flow.unimodality_pretrained) == 2
    assert four.modality == ["rgb", "sound", "flow", "rgbdiff"] and four.cost_weights == [0.5, 0.05, 0.8]
    assert evaluate.evaluate and evaluate.pretrained == "/PATH/TO/ADAMML_MODEL" and not evaluate.multiprocessing_distributed
    # the placeholders of the template lines are rejected where the reference's argparse `choices` would reject them
    with pytest.raises(SystemExit):
        train.resolve_args(tmpl, log=lambda *_: None)
    notes = []
    for a, chans in ((rgb_audio, [3, 1]), (rgb_flow, [3, 10, 15]), (four, [3, 1, 10, 15])):
        a.dataset = "kinetics-sounds"                        # (README placeholder DATASET)
        train.resolve_args(a, log=notes.append)
        assert a.num_classes == 31 and a.input_channels == chans and a.groups == 8 and a.num_segments == 5 and a.depth == 50
    assert notes and "--workers" in notes[0] and "--dense_sampling" in notes[0]     # inert flags are reported, not rejected
    # every destination of the reference's parser exists here (names read off opts.py:5-149)
    dests = ("backbone_net depth dropout groups num_segments frames_per_group without_t_stride pooling_method fusion_point prefix "
             "learnable_lf_weights causality_modeling cost_weights rng_policy rng_threshold gammas penalty_type gpu gpu_id cudnn_benchmark "
             "batch_size lr p_lr lr_scheduler lr_steps momentum nesterov weight_decay epochs warmup_epochs finetune_epochs resume auto_resume "
             "pretrained unimodality_pretrained start_epoch clip_gradient curr_stage workers datadir dataset threed_data input_size "
             "disable_scaleup random_sampling dense_sampling augmentor_ver scale_range modality mean std skip_normalization fps audio_length "
             "resampling_rate logdir print_freq show_model evaluate num_crops num_clips val_num_clips pred_files pred_weights after_softmax "
             "lazy_eval sync_bn world_size rank dist_url hostfile dist_backend multiprocessing_distributed").split()
    ns = vars(train.arg_parser().parse_args([]))
    assert [d for d in dests if d not in ns] == []


def test_plateau_schedule_follows_torch():
    """train.LRSchedule('plateau') stepped with validation losses == torch.optim.lr_scheduler.ReduceLROnPlateau('min') defaults
    (train_adamml.py:268-269,460-462)."""
    from adamml_amd import train

    class _Opt:
        lr = 0.1
    o = _Opt()
    s = train.LRSchedule(o, "plateau", 0.1, 50, [15])
    p = torch.nn.Parameter(torch.zeros(1))
    topt = torch.optim.SGD([p], lr=0.1)
    ts = torch.optim.lr_scheduler.ReduceLROnPlateau(topt, "min")
    losses = [1.0, 0.9, 0.8] + [0.8] * 12 + [0.7] + [0.75] * 13
    for e, v in enumerate(losses):
        s.step(e + 1, v)
        ts.step(v)
        assert abs(o.lr - topt.param_groups[0]["lr"]) < 1e-12, (e, o.lr, topt.param_groups[0]["lr"])
    assert o.lr < 0.0011


def test_launch_plan_thunks_are_in_sync_with_the_c_abi(built):
    """csrc/plan_thunks.inc (generated by tools/gen_plan_thunks.py) has one case per stream-taking entry point of include/adamml_hip.h,
    numbered by its position in sorted(hip.SIGNATURES) -- the numbering adamml_amd/plan.py records with -- and the library agrees on the
    count; the record structure has the size the header declares."""
    import subprocess
    import sys
    from adamml_amd import hip, plan
    path = os.path.join(ROOT, "adamml_amd", "csrc", "plan_thunks.inc")
    before = open(path).read()
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_plan_thunks.py")], stdout=subprocess.DEVNULL)
    assert open(path).read() == before, "plan_thunks.inc is stale: run tools/gen_plan_thunks.py and rebuild"
    names = sorted(hip.SIGNATURES)
    for i, n in enumerate(names):
        assert ("case %d: return %s(" % (i, n)) in before
        assert plan.fn_id(n) == i
    lib = ctypes.CDLL(built)
    assert lib.adamml_plan_num_entry_points() == len(names)
    assert ctypes.sizeof(plan.PlanOp) == 4 * 4 + 2 * 4 + 8 * plan.MAX_ARGS
    assert abi.DEFINES["ADAMML_PLAN_MAX_ARGS"] == plan.MAX_ARGS


def test_launch_plan_recorder_encodes_calls_slots_waits_and_segments():
    """adamml_amd/plan.py Recorder (no GPU needed: it only looks at addresses): a recorded call becomes one adamml_plan_op_t with the
    entry point's index, the stream's slot, descriptor COPIES, pointer values, doubles as bit patterns, and slot references for the
    call's input (slot 0) and the incoming gradient (slot 1); waits number their events; boundaries split segments per phase."""
    import struct
    from adamml_amd import hip, plan
    x = torch.zeros(8)
    rec = plan.Recorder(x)
    d = hip.ConvDesc(2, 8, 8, 16, 8, 8, 32, 1, 1, 1, 0, 1, 0, 0, 1, 0)
    rec.call("adamml_conv_bwd_data", (ctypes.byref(d), x.data_ptr(), 0x1000, None, 1), 0xAAA0)
    op = rec.cur[-1]
    assert (op.kind, op.fn, op.nargs, op.stream) == (plan.KIND_CALL, plan.fn_id("adamml_conv_bwd_data"), 5, 0)
    assert op.slot_mask == 0b00010 and op.a[1] == 0                     # argument 1 = the call's input: slot 0, not its address
    assert op.a[2] == 0x1000 and op.a[3] == 0 and op.a[4] == 1
    copy = ctypes.cast(op.a[0], ctypes.POINTER(hip.ConvDesc)).contents   # a private copy of the descriptor, alive as long as the recorder
    d.Cout = 7
    assert copy.Cout == 32 and copy.N == 2
    rec.call("adamml_bn_finalize", (0x2000, 32, 5, 123.5, 0x10, 0x20, None, None, 0.1, 1e-5, 0x30, 64), 0xBBB0)
    op = rec.cur[-1]
    assert op.stream == 1 and rec.streams == [0xAAA0, 0xBBB0]           # second stream handle -> slot 1
    assert struct.unpack("<d", struct.pack("<Q", op.a[3]))[0] == 123.5 and abs(struct.unpack("<d", struct.pack("<Q", op.a[8]))[0] - 0.1) < 1e-7
    rec.wait(0xBBB0, 0xAAA0)
    rec.wait(0xAAA0, 0xBBB0)
    w0, w1 = rec.cur[-2], rec.cur[-1]
    assert (w0.kind, w0.stream, w0.a[0], w0.a[1]) == (plan.KIND_WAIT, 1, 0, 0) and (w1.stream, w1.a[0], w1.a[1]) == (0, 1, 1) and rec.n_events == 2
    z = torch.zeros(6, dtype=torch.float64)
    rec.zero(z, 0xAAA0)
    assert (rec.cur[-1].kind, rec.cur[-1].a[0], rec.cur[-1].a[1]) == (plan.KIND_ZERO, z.data_ptr(), 48)
    hit = []
    rec.boundary(lambda: hit.append(1))
    rec.call("adamml_conv_bwd_data", (ctypes.byref(d), 0x1, 0x2, 0x3, 0), 0xAAA0)
    rec.end_forward()
    assert [s.n for s in rec.fwd] == [5, 1] and rec.fwd[0].boundary is not None and rec.fwd[1].boundary is None
    g = torch.zeros(4)
    rec.begin_backward(g)
    rec.call("adamml_conv_bwd_data", (ctypes.byref(d), g.data_ptr(), x.data_ptr(), 0x3, 0), 0xAAA0)
    rec.end_backward()
    op = rec.bwd[0].ops[0]
    assert op.slot_mask == 0b00110 and (op.a[1], op.a[2]) == (1, 0)      # gradient = slot 1, input = slot 0
    rec.call("adamml_conv_bwd_data", (ctypes.byref(d), 1, 2), 0xAAA0)    # wrong argument count: the recording is marked failed, not wrong
    assert rec.failed is not None


def test_imagenet_initialisation_from_local_files_matches_the_reference(tmp_path):
    """models/resnet.py:19-33,251-257, models/sound_mobilenet_v2.py:186-196, models/policy_net.py:193-203,221: the reference starts from
    downloaded ImageNet weights, converting a non-RGB stem to the mean over RGB expanded to the input channels and dropping the
    classifier.  adamml_amd.imagenet_init does the same from LOCAL files.  Golden = the reference's own functions run on synthetic files
    with the published names and shapes (tools/gen_imagenet_init_golden.py -> tests/golden/imagenet_init.npz); the test writes the
    identical files (name-keyed generator) and compares every state_dict entry of the initialised models."""
    import warnings
    import numpy as np
    from adamml_amd import imagenet_init, policy_net
    from adamml_amd.resnet import resnet
    from adamml_amd.sound_mobilenet_v2 import sound_mobilenet_v2
    from tests.imagenet_init_cases import CASES as ICASES, torchvision_like, digest
    gold = np.load(os.path.join(ge.ROOT, "tests", "golden", "imagenet_init.npz"))
    dli = policy_net.MobileNetV2(1000, num_frames=1, input_channels=3).state_dict()       # (the d-li14 file is named like the policy net itself)
    files = {"resnet50": torchvision_like("resnet50"), "mobilenet_v2": torchvision_like("mobilenet_v2"),
             "mobilenetv2_160x160": torchvision_like("mobilenetv2_160x160", like=dli)}
    for arch, sd in files.items():
        torch.save(sd, str(tmp_path / (arch + "-0000.pth")))
    # three ways to name the files: configure(), $ADAMML_IMAGENET_DIR, the launcher's --imagenet_weights
    imagenet_init.configure(resnet50=str(tmp_path / "resnet50-0000.pth"))
    os.environ["ADAMML_IMAGENET_DIR"] = str(tmp_path)
    try:
        assert imagenet_init.path_for("mobilenet_v2").endswith("mobilenet_v2-0000.pth")
        assert imagenet_init.path_for("mobilenetv2_160x160").endswith("mobilenetv2_160x160-0000.pth")
        with warnings.catch_warnings():
            warnings.simplefilter("error")                       # everything is configured: no "keeps its random initialisation" warning
            for name, c in ICASES.items():
                if c["kind"] == "resnet":
                    m = resnet(50, 31, False, 8, 0.5, "max", c["ch"], imagenet_pretrained=True)
                elif c["kind"] == "sound":
                    m = sound_mobilenet_v2(31, c["ch"], 0.5, imagenet_pretrained=True)
                else:
                    m = policy_net.JointMobileNetV2(8, ["x"], input_channels=[c["ch"]]).nets[0]      # models/policy_net.py:215-222
                got = digest(m.state_dict(), c["stem"])
                keys = [k[len(name) + 1:] for k in gold.files if k.startswith(name + "/")]
                assert sorted(keys) == sorted(got), (name, set(keys) ^ set(got))
                for k in keys:
                    g = gold[name + "/" + k]
                    if k.endswith("num_batches_tracked") or not (k.startswith("fc.") or k.startswith("classifier")):
                        assert np.allclose(got[k], g, rtol=1e-6, atol=1e-7), (name, k)
                    # (fc / classifier are NOT loaded: both sides keep their own random initialisation there -- only the size is compared)
                    assert got[k].shape == g.shape and (k == c["stem"] or got[k][-1] == g[-1]), (name, k)
                stem = m.state_dict()[c["stem"]]
                assert stem.shape[1] == c["ch"]
                if c["ch"] != 3:                                 # mean over RGB, repeated: all input channels equal
                    assert torch.equal(stem, stem[:, :1].expand_as(stem))
    finally:
        del os.environ["ADAMML_IMAGENET_DIR"]
        imagenet_init.configure(resnet50=None)
    # the launcher flag (opts.py has no equivalent: the reference downloads) and the quiet default
    from adamml_amd import train
    a = train.arg_parser().parse_args(["--backbone_net", "adamml", "--modality", "rgb", "sound", "--dataset", "kinetics-sounds",
                                       "--imagenet_weights", "resnet50=" + str(tmp_path / "resnet50-0000.pth")])
    try:
        a = train.resolve_args(a, log=lambda *x: None)
        assert a.imagenet_pretrained is True and imagenet_init.path_for("resnet50").endswith("resnet50-0000.pth")
    finally:
        imagenet_init.configure(resnet50=None)
    with pytest.warns(UserWarning, match="no local file"):
        imagenet_init._WARNED.clear()
        resnet(50, 31, False, 8, 0.5, "max", 3, imagenet_pretrained=True)


def test_autograd_end_of_backward_callback():
    """backbone.queue_end_of_backward wraps the one semi-private torch hook the package uses (the engine's queue_callback, as torch's
    own DistributedDataParallel / FSDP do): a callback queued from inside a backward node runs exactly once, after EVERY node of that
    backward pass has run, and a later backward pass does not run it again."""
    from adamml_amd.backbone import queue_end_of_backward
    log = []

    class Node(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, tag):
            ctx.tag = tag
            return x * 2

        @staticmethod
        def backward(ctx, g):
            log.append("node" + ctx.tag)
            if ctx.tag == "B":                       # the LAST node of the forward is the first to run in backward
                queue_end_of_backward(lambda: log.append("end"))
            return g * 2, None
    x = torch.ones(3, requires_grad=True)
    Node.apply(Node.apply(x, "A"), "B").sum().backward()
    assert log == ["nodeB", "nodeA", "end"], log
    Node.apply(x, "A").sum().backward()
    assert log == ["nodeB", "nodeA", "end", "nodeA"], log


def test_swapped_parameter_object_is_rehomed_by_the_next_call():
    """Round-4 advisor finding: a parameter OBJECT replaced in the middle of the list (a new `fc` for another class count, the usual
    fine-tuning edit) must be picked up by the very next ensure() -- not by the every-32nd-call walk, during which the old object would
    be updated by the fused optimizer and the new one silently ignored.  HipBackbone reports the assignment to every FlatBuffers that
    manages it (its own and the enclosing sub-network's)."""
    import torch.nn as nn
    from adamml_amd import adamml
    m = adamml(groups=8, modality=["rgb", "sound"], input_channels=[3, 1], num_segments=2, rng_policy=False, rng_threshold=0.5,
               causality_modeling="lstm", num_classes=31, depth=50, without_t_stride=False, dropout=0.5, pooling_method="max",
               fusion_point="logits", unimodality_pretrained=[], learnable_lf_weights=True)
    cpu = torch.device("cpu")
    fb = m._flat_main
    fb.ensure(cpu)
    fb.ensure(cpu)                                   # (fast path from now on)
    res = m.main_net.nets[0]
    assert len(res._params()) == len(list(res.parameters()))
    lo, hi = fb.flat.data_ptr(), fb.flat.data_ptr() + fb.flat.numel() * 4
    old_fc = res.fc
    res.fc = nn.Linear(2048, 7)                      # swapped after "step 1"
    assert "_plist" not in res.__dict__              # the backbone's cached list is dropped at once
    fb.ensure(cpu)                                   # the next call (not the 32nd) re-homes
    assert any(p is res.fc.weight for p in fb.params) and not any(p is old_fc.weight for p in fb.params)
    assert lo != fb.flat.data_ptr() or fb.flat.numel() != (hi - lo) // 4          # rebuilt: the parameter count changed
    lo, hi = fb.flat.data_ptr(), fb.flat.data_ptr() + fb.flat.numel() * 4
    assert lo <= res.fc.weight.data_ptr() < hi and lo <= res.fc.bias.data_ptr() < hi
    assert any(p is res.fc.weight for p in res._params())
    # same shape swap (data_ptr probes of the first / last parameter cannot see it)
    res.layer1[0].bn1.weight = nn.Parameter(torch.full((64,), 3.0))
    res.__setattr__("_touch", nn.Identity())         # (a deeper edit is reported by an explicit assignment on the backbone -- or by invalidate())
    fb.ensure(cpu)
    assert lo <= res.layer1[0].bn1.weight.data_ptr() < hi or fb.flat.data_ptr() != lo
    assert float(res.layer1[0].bn1.weight.data[0]) == 3.0
    # the Sound-MobileNetV2 head is an item of a Sequential: `net.classifier[1] = nn.Linear(...)` goes through Sequential.__setitem__, not
    # through the backbone's __setattr__ (round-5 advisor finding) -- backbone.NotifyingSequential reports it the same way
    snd = m.main_net.nets[1]
    fb.ensure(cpu)
    fb.ensure(cpu)
    old_head = snd.classifier[1]
    snd.classifier[1] = nn.Linear(old_head.in_features, 5)
    assert "_plist" not in snd.__dict__
    fb.ensure(cpu)                                   # the next call re-homes the new head
    assert any(p is snd.classifier[1].weight for p in fb.params) and not any(p is old_head.weight for p in fb.params)
    lo, hi = fb.flat.data_ptr(), fb.flat.data_ptr() + fb.flat.numel() * 4
    assert lo <= snd.classifier[1].weight.data_ptr() < hi
    assert list(snd.state_dict().keys())[-2:] == ["classifier.1.weight", "classifier.1.bias"]       # (state_dict names of a plain Sequential)


def test_parity_bounds_table_respects_the_stated_tolerances():
    """tests/parity_bounds.json is re-based by tools/rebase_bounds.py from one GPU run; whatever a re-base does, no bound may drift
    past the stated tolerance of its category (logits <= 4e-2, policy logits <= 8e-2, running statistics <= 3e-2, replay gradients
    p90 <= 0.13, ...) and every bound is min(1.3 x measured, ceiling)."""
    from tests import parity_bounds as pb
    t = pb.table()
    assert len(t) >= 40
    assert pb.CEILINGS["logits"] <= 4e-2 and pb.CEILINGS["plog"] <= 8e-2 and pb.CEILINGS["stats"] <= 3e-2 and pb.CEILINGS["replay_p90"] <= 0.13
    for k, e in t.items():
        # every entry has its OWN ceiling <= the category's (round-5 advisor finding: a category-wide ceiling let a tight entry drift)
        ceil = e["ceil"]
        assert ceil <= pb.CEILINGS[e["cat"]] * (1 + 1e-9), (k, e)
        if pb.is_soft(e["cat"]):
            # printed regression figures of the emulation-gated forward quantities (tests/parity_bounds.emu_gate is their hard gate):
            # 1.3 x the last measurement, the category's STATED tolerance kept beside it for the record
            assert e.get("soft") and abs(e["bound"] - pb.FACTOR * e["measured"]) <= 2e-3 * e["bound"], (k, e)
            continue
        assert 0 < e["measured"] <= ceil, (k, e)
        assert e["bound"] <= ceil * (1 + 1e-9), (k, e)
        assert abs(e["bound"] - min(pb.FACTOR * e["measured"], ceil)) <= 2e-3 * e["bound"], (k, e)
    # the re-base refuses a figure above an entry's ceiling and, without --allow-growth, one that grew by more than 10 %
    old = t["c4.eval.logits"]
    with pytest.raises(SystemExit):
        pb.rebased_entry("eval_logits", 1.2 * old["measured"], old, False, "c4.eval.logits")
    assert pb.rebased_entry("eval_logits", 1.2 * old["measured"], old, True, "x")["ceil"] == old["ceil"]
    with pytest.raises(SystemExit):
        pb.rebased_entry("eval_logits", 2.5 * old["measured"], old, True, "c4.eval.logits")        # (above its own ceiling although below the category's 6e-2)
    # the emulation fixtures of the full-size cases exist and the emulation-relative gate has its constants
    for name in ("resnet50_c1", "adamml_c2", "adamml_c4", "adamml_c5"):
        assert os.path.exists(os.path.join(ROOT, "tests", "golden", name + "_bf16emu.npz")), name
    assert pb.EMU_K <= 2.0 and pb.EMU_K_HE <= 1.0 and all(pb.EMU_FLOOR[c] <= 0.25 * pb.CEILINGS[c] * (1 + 1e-9) for c in pb.EMU_FLOOR)
    for case in ("c1.train", "c2.train_main", "c2.train_policy", "c4.train_main", "c5.train_main", "c5.train_policy"):
        assert case + ".logits" in t and case + ".stats" in t and case + ".head" in t
    src = open(os.path.join(ROOT, "tests", "test_parity_fullsize_gpu.py")).read()
    assert "_tol=" not in src and "max_tol" not in src          # no scattered literals left in the full-size file
    # the 20-step trajectory reads the table too (round 5: its literals vetoed a data-gradient kernel that rounds dz in its loader)
    assert pb.CEILINGS["traj_emu"] <= 5e-2 and pb.CEILINGS["traj_ref_mean"] <= 0.10
    assert all(k in t for k in ("traj_c2.loss_vs_emu_max", "traj_c2.loss_vs_ref_max", "traj_c2.loss_vs_ref_mean", "traj_c2.final_logits", "traj_c2.fc_update"))
    assert "<= 0.0" not in open(os.path.join(ROOT, "tests", "test_train_trajectory_gpu.py")).read()
