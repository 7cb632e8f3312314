"""The one reader of include/adamml_hip.h: every function the header declares (name, return type, parameters, and the ctypes kinds they
map to) and its integer #defines.  tools/gen_plan_thunks.py generates the replay thunks from it; the tests take the declared names from
it and check the tables adamml_amd/hip.py states by hand against it (tests/test_abi_cpu.py).  Standard library only."""
import collections
import os
import re
from ctypes import c_void_p, c_int, c_int64, c_float, c_double, c_size_t, c_char_p

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "adamml_hip.h")

# the whole vocabulary of the header; a type outside it is an error, never a guessed c_void_p
SCALARS = {"int": c_int, "float": c_float, "double": c_double, "size_t": c_size_t, "int64_t": c_int64, "hipStream_t": c_void_p}
RETURNS = {"int": c_int, "size_t": c_size_t, "const char*": c_char_p}
DESC = "const adamml_conv_desc_t*"


class Function(collections.namedtuple("Function", "name ret params")):
    """ret: the C return type; params: [(C type, parameter name)], both as the header spells them with single spaces"""
    __slots__ = ()

    def __str__(self):
        return "%s %s(%s)" % (self.ret, self.name, ", ".join("%s %s" % p for p in self.params) or "void")

    @property
    def launches(self):
        """an entry point that enqueues work (a key of hip.SIGNATURES): hip.call appends the stream, a launch plan can replay it"""
        return self.ret == "int" and bool(self.params) and self.params[-1][0] == "hipStream_t"

    @property
    def restype(self):
        return RETURNS[self.ret]

    def argtypes(self, desc):
        """desc: the ctypes type of `const adamml_conv_desc_t*` (the structure is declared by the caller, hip.ConvDesc)"""
        return [desc if t == DESC else c_void_p if t.endswith("*") else SCALARS[t] for t, _ in self.params]


def parse(text):
    """-> ({name: Function} in header order, {name: value} of the integer #defines)"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = {m.group(1): int(m.group(2), 0)
               for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(-?(?:0[xX][0-9a-fA-F]+|[1-9]\d*|0))[ \t]*$", text, flags=re.M)}
    text = ";" + re.sub(r"^[ \t]*#[^\n]*", "", text, flags=re.M)
    functions = {}
    # a statement `[ADAMML_API] <return type> adamml_name(<parameters>);` -- whatever stands in front of the name is the return type
    for m in re.finditer(r"(?<=[;{}])\s*(?:ADAMML_API\s+)?([^;{}()]*?)\s*\b(adamml_\w+)\s*\(([^;{}()]*)\)\s*;", text):
        ret, name, params = " ".join(m.group(1).split()), m.group(2), " ".join(m.group(3).split())
        if ret not in RETURNS:
            raise ValueError("%s: return type %r is not one of %s" % (name, ret, sorted(RETURNS)))
        plist = []
        for p in ([] if params == "void" else params.split(",")):
            pm = re.fullmatch(r"\s*(.*?)\s*\b(\w+)\s*", p)
            ctype = pm.group(1) if pm else ""
            if not (ctype.endswith("*") or ctype in SCALARS):
                raise ValueError("%s: parameter %r has type %r, which is neither a pointer nor one of %s" % (name, p.strip(), ctype, sorted(SCALARS)))
            plist.append((ctype, pm.group(2)))
        functions[name] = Function(name, ret, plist)
    unread = set(re.findall(r"\b(adamml_\w+)\s*\(", text)) - set(functions)
    if unread:
        raise ValueError("declarations this reader cannot parse: %s" % sorted(unread))
    return functions, defines


with open(HEADER) as _f:
    FUNCTIONS, DEFINES = parse(_f.read())
