"""adamml_amd/abi.py, the one reader of include/adamml_hip.h, without a GPU: the parser on hand-made snippets, and what Python restates of
the header by hand against it, kind for kind: the ctypes declarations of the loaded library (hip.load), the launch table (hip.SIGNATURES,
plan.fn_id) and the constants that copy a #define."""
import ctypes

import pytest

import __graft_entry__ as ge
from adamml_amd import abi

SNIPPET = """
/* a block comment that holds a prototype: int adamml_fake(int x); and a call adamml_other(1) */
#define ADAMML_API __attribute__((visibility("default")))
#define ADAMML_SNIPPET_SLOTS 32
#define ADAMML_SNIPPET_HEX 0x10
typedef struct { int32_t a, b; } adamml_snippet_t;
// int adamml_fake(int x);
ADAMML_API int adamml_spread(const adamml_conv_desc_t* d, const void* x,
                             double* stats /* [slots][2C] */,
                             size_t n, int64_t m, float f, double g,
                             hipStream_t stream);
ADAMML_API int adamml_pointers(const float* const* p, int n);
ADAMML_API size_t adamml_bytes(int n);
ADAMML_API const char* adamml_text(void);
int adamml_bare(void);
"""


def test_parser_reads_prototypes_and_defines_and_skips_comments():
    by, defs = abi.parse(SNIPPET)
    assert list(by) == ["adamml_spread", "adamml_pointers", "adamml_bytes", "adamml_text", "adamml_bare"]      # header order, no adamml_fake
    spread = by["adamml_spread"]                                                  # a prototype over four lines, a comment inside it
    assert spread.ret == "int" and spread.params == [("const adamml_conv_desc_t*", "d"), ("const void*", "x"), ("double*", "stats"), ("size_t", "n"),
                                                     ("int64_t", "m"), ("float", "f"), ("double", "g"), ("hipStream_t", "stream")]
    desc = ctypes.POINTER(ctypes.c_int32)
    assert spread.argtypes(desc) == [desc, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int64, ctypes.c_float, ctypes.c_double,
                                     ctypes.c_void_p]
    assert spread.launches and spread.restype is ctypes.c_int
    assert by["adamml_pointers"].params == [("const float* const*", "p"), ("int", "n")]
    assert by["adamml_pointers"].argtypes(desc) == [ctypes.c_void_p, ctypes.c_int] and not by["adamml_pointers"].launches
    assert by["adamml_bytes"].ret == "size_t" and by["adamml_bytes"].restype is ctypes.c_size_t
    assert by["adamml_text"].ret == "const char*" and by["adamml_text"].restype is ctypes.c_char_p
    assert by["adamml_text"].params == [] and by["adamml_bare"].params == [] and by["adamml_text"].argtypes(desc) == []      # (void)
    assert str(by["adamml_text"]) == "const char* adamml_text(void)" and str(by["adamml_bytes"]) == "size_t adamml_bytes(int n)"
    assert defs == {"ADAMML_SNIPPET_SLOTS": 32, "ADAMML_SNIPPET_HEX": 16}         # integer defines only: not ADAMML_API


@pytest.mark.parametrize("proto, named", [
    ("int adamml_odd(int n, unsigned short x);", ["adamml_odd", "unsigned short"]),             # a parameter type outside the vocabulary
    ("int adamml_odd(int n, float* const x);", ["adamml_odd", "float* const"]),
    ("int adamml_odd(int);", ["adamml_odd"]),                                                   # no parameter name
    ("unsigned int adamml_odd(int n);", ["adamml_odd", "unsigned int"]),                        # a return type outside it
    ("void adamml_odd(int n);", ["adamml_odd", "void"]),
    ("int adamml_odd(int n, void (*cb)(int));", ["adamml_odd"]),                                # a declaration the reader cannot take apart
])
def test_parser_refuses_what_it_does_not_know(proto, named):
    with pytest.raises(ValueError) as e:
        abi.parse("int adamml_fine(int n);\n" + proto)
    assert all(n in str(e.value) for n in named), str(e.value)


def same(row, want):
    """two lists of ctypes kinds hold the same objects (plan.Recorder tells the kinds apart with `is`)"""
    return len(row) == len(want) and all(a is b for a, b in zip(row, want))


def test_library_is_declared_as_the_header_says():
    """After hip.load() every function of the header is an attribute of the library whose argtypes are, kind for kind, what the header's
    parameter types map to, with restype c_size_t exactly for the size_t returns, c_char_p exactly for the error string, c_int otherwise."""
    from adamml_amd import hip
    ge.build()
    lib = hip.load()
    fns = abi.FUNCTIONS
    assert len(fns) >= 114
    restypes = {}
    for name, f in fns.items():
        fn = getattr(lib, name)
        assert same(list(fn.argtypes or []), f.argtypes(hip._DESC)), (name, fn.argtypes, str(f))
        assert fn.restype is f.restype, (name, fn.restype, f.ret)
        restypes.setdefault(fn.restype, set()).add(name)
    sized = {n for n, f in fns.items() if f.ret == "size_t"}
    assert len(sized) >= 9 and all(n.endswith("_workspace") for n in sized)
    assert restypes == {ctypes.c_size_t: sized, ctypes.c_char_p: {"adamml_" + "last_error_string"},
                        ctypes.c_int: set(fns) - sized - {"adamml_" + "last_error_string"}}


def test_launch_set_is_the_headers_stream_taking_functions():
    """hip.SIGNATURES holds exactly the functions whose last parameter is hipStream_t, every row kind for kind what the header's parameter
    types map to (a c_int where the header says size_t, a c_float where it says double, would load, pass every count check and truncate
    the value or replay the wrong bits from a launch plan), and plan.fn_id numbers them in sorted order: the numbering
    csrc/plan_thunks.inc was generated with."""
    from adamml_amd import hip, plan
    fns = abi.FUNCTIONS
    streamed = sorted(n for n, f in fns.items() if f.params and f.params[-1][0] == "hipStream_t")
    assert sorted(hip.SIGNATURES) == streamed == sorted(n for n, f in fns.items() if f.launches) and len(streamed) >= 72
    assert [plan.fn_id(n) for n in streamed] == list(range(len(streamed)))
    assert abi.SCALARS == {"int": hip._I, "float": hip._F, "double": hip._D, "size_t": hip._Z, "int64_t": hip._L, "hipStream_t": hip._P}
    for n in streamed:
        assert same(hip.SIGNATURES[n], fns[n].argtypes(hip._DESC)), (n, hip.SIGNATURES[n], str(fns[n]))


def test_python_constants_equal_the_headers_defines():
    from adamml_amd import hip, jpeg, plan
    d = abi.DEFINES
    assert d == {"ADAMML_STAT_SLOTS": hip.STAT_SLOTS, "ADAMML_ACT_NONE": hip.ACT_NONE, "ADAMML_ACT_RELU": hip.ACT_RELU, "ADAMML_ACT_RELU6": hip.ACT_RELU6,
                 "ADAMML_JPEG_SUBSEQ_BYTES": jpeg.SUBSEQ_BYTES, "ADAMML_PLAN_MAX_ARGS": plan.MAX_ARGS, "ADAMML_PLAN_CALL": plan.KIND_CALL,
                 "ADAMML_PLAN_WAIT": plan.KIND_WAIT, "ADAMML_PLAN_ZERO": plan.KIND_ZERO}
