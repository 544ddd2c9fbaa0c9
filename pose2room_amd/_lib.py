"""ctypes loader for libp2r_hip.so (C ABI declared in include/p2r_hip.h) and for the extension libraries next to it.

The libraries are built in-tree by `pose2room_amd/csrc/Makefile`
(`__graft_entry__.build()`).  Loading fails loudly: there is no Python or CPU
fallback for any entry point.

A header is the one declaration of its library's ABI, and a `Library` binds the two: `prototypes()` parses the header
into the `argtypes` / `restype` of every entry point, `struct()` into the `ctypes.Structure` of every `typedef struct`,
and `launch` / `launch_on` check a call against its prototype before anything is enqueued.  `main` is libp2r_hip.so;
the module-level `lib`, `marshal`, `launch_on` and `launch` are its methods.

The parser is no C parser.  It reads the subset the headers use -- `/* */` comments, preprocessor lines,
`typedef struct { ... } name;` blocks of pointer / int / long long / double fields, and prototypes
`type p2r_name(type name, ...);` over int, float, double, long long, unsigned long long and pointers -- and raises
P2RLibraryError, naming the header and the declaration, on anything else.
"""
import collections
import ctypes
import keyword
import numbers
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# P2R_LIB_PATH: another build of the SAME library (A/B timing of kernel variants on one box, tools/ab_bench.sh); the
# loader's checks (ABI version, every declared symbol) apply to it unchanged
LIB_PATH = os.environ.get("P2R_LIB_PATH") or os.path.join(_HERE, "libp2r_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "p2r_hip.h")

ABI_VERSION = 3     # p2r_abi_version() of the library this loader was written against (include/p2r_hip.h)


class P2RLibraryError(RuntimeError):
    pass


# ---- the header ---------------------------------------------------------------------------------------------------------
_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double,
            "long long": ctypes.c_longlong, "unsigned long long": ctypes.c_ulonglong}
_KINDS = {ctypes.c_int: "i", ctypes.c_longlong: "i", ctypes.c_ulonglong: "i", ctypes.c_float: "f",
          ctypes.c_double: "f", ctypes.c_void_p: "p"}
_STRUCT_RE = re.compile(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;")
_PROTO_RE = re.compile(r"([A-Za-z_][\w\s]*?[\s\*]+)(p2r_[a-z0-9_]+)\s*\(([^()]*)\)\s*;")

# one entry point: kinds = 'i' (integer) / 'f' (floating) / 'p' (pointer) per parameter in front of the stream; pointer =
# the same as one flag per parameter, scalars = the positions of the others (what `marshal` walks)
Prototype = collections.namedtuple("Prototype", "name text restype argtypes kinds has_stream pointer scalars")


def _code(header_path):
    """the header without comments and preprocessor lines"""
    with open(header_path) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return re.sub(r"^\s*#.*$", "", text, flags=re.M)


def declared_symbols(header_path=HEADER_PATH):
    """Names of every function the C header declares (used by the export test)."""
    return sorted(set(re.findall(r"\b(p2r_[a-z0-9_]+)\s*\(", _code(header_path))))


def _ctype(decl, what):
    """`decl` = a parameter or field declaration without its name: anything with a `*` is a pointer"""
    if "*" in decl:
        return ctypes.c_void_p
    base = " ".join(t for t in decl.split() if t != "const")
    if base not in _SCALARS:
        raise P2RLibraryError(f"type '{base}' in `{what}` is outside the subset the binding maps "
                              f"({', '.join(_SCALARS)}, pointers)")
    return _SCALARS[base]


def _parse_prototype(ret, name, params):
    text = " ".join(f"{ret.strip()} {name}({params});".split())
    ret = " ".join(ret.split())
    if ret == "const char *":
        restype = ctypes.c_char_p
    elif "*" in ret:
        raise P2RLibraryError(f"return type '{ret}' of `{text}` is outside the subset the binding maps")
    else:
        restype = _ctype(ret, text)
    argtypes, names = [], []
    if params.strip() != "void":
        for p in params.split(","):
            m = re.fullmatch(r"\s*(.*?[\s\*])(\w+)\s*", p, flags=re.S)
            if m is None:
                raise P2RLibraryError(f"cannot read parameter '{p.strip()}' of `{text}`")
            argtypes.append(_ctype(m.group(1), text))
            names.append(m.group(2))
    has_stream = bool(names) and names[-1] in ("stream", "stream_h") and argtypes[-1] is ctypes.c_void_p
    kinds = "".join(_KINDS[t] for t in (argtypes[:-1] if has_stream else argtypes))
    return Prototype(name, text, restype, tuple(argtypes), kinds, has_stream, tuple(k == "p" for k in kinds),
                     tuple(i for i, k in enumerate(kinds) if k != "p"))


def _parse_struct(body, name):
    fields = []
    for decl in body.split(";"):
        if not decl.strip():
            continue
        first, *more = decl.split(",")
        m = re.fullmatch(r"\s*(.*?[\s\*])(\w+)\s*", first, flags=re.S)
        if m is None:
            raise P2RLibraryError(f"cannot read field '{decl.strip()}' of struct {name}")
        base = m.group(1).replace("*", " ")
        pieces = [(m.group(1), m.group(2))]
        for d in more:       # further declarators of the line share the base type: `const float *x, *x2;`
            m = re.fullmatch(r"\s*(\**)\s*(\w+)\s*", d)
            if m is None:
                raise P2RLibraryError(f"cannot read field '{decl.strip()}' of struct {name}")
            pieces.append((base + m.group(1), m.group(2)))
        for typ, field in pieces:
            fields.append((field + "_" if keyword.iskeyword(field) else field, _ctype(typ, f"struct {name}: {decl.strip()}")))
    return type(name, (ctypes.Structure,), {"_fields_": fields})


def _parse(header_path):
    """-> ({name: Prototype}, {name: ctypes.Structure}) of the header; an error names the header it was reading"""
    code = _code(header_path)
    try:
        structs = {m.group(2): _parse_struct(m.group(1), m.group(2)) for m in _STRUCT_RE.finditer(code)}
        protos = {m.group(2): _parse_prototype(*m.groups()) for m in _PROTO_RE.finditer(_STRUCT_RE.sub("", code))}
        unread = sorted(set(declared_symbols(header_path)) - set(protos))
        if unread:
            raise P2RLibraryError(f"the declarations of {unread} are outside the subset the binding reads")
    except P2RLibraryError as e:
        raise P2RLibraryError(f"{os.path.basename(header_path)}: {e}") from None
    return protos, structs


def check(status, what):
    if status != 0:
        raise RuntimeError(f"libp2r_hip: {what} failed with status {status}")


def ptr(t):
    """Device pointer of a torch tensor (or NULL for None)."""
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def current_stream(device):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


# ---- launches -------------------------------------------------------------------------------------------------------------
# what a pointer parameter takes besides a tensor and None: an address, a host array (job lists, counts), byref(struct)
_HOST_POINTERS = (int, ctypes.c_void_p, ctypes.Array, type(ctypes.byref(ctypes.c_int())))


def _address(proto, i, a):
    if hasattr(a, "data_ptr"):
        return a.data_ptr()
    if not isinstance(a, _HOST_POINTERS):
        raise TypeError(f"{proto.name}: argument {i} = {a!r} where a pointer is declared: {proto.text}")
    return a


def _scalar(proto, i, a):
    if proto.kinds[i] == "i":
        if not isinstance(a, numbers.Integral):
            raise TypeError(f"{proto.name}: argument {i} = {a!r} where an integer is declared: {proto.text}")
        return int(a)
    if not isinstance(a, numbers.Real):
        raise TypeError(f"{proto.name}: argument {i} = {a!r} where a float or double is declared: {proto.text}")
    return float(a)


class Library(object):
    """One shared library bound from its header: libp2r_hip.so (`main` below) and every extension library next to it
    (csrc/Makefile: EXTS) is one of these.  The header is read once per object, at the first use; the library is loaded
    by the first `lib()`.  abi_version: what the library's p2r_abi_version() must return, where it has one."""

    def __init__(self, header_path, lib_path, abi_version=None):
        self.header_path, self.lib_path, self.abi_version = header_path, lib_path, abi_version
        self._protos = self._structs = self._handle = None

    def prototypes(self):
        """name -> Prototype of every entry point the header declares."""
        if self._protos is None:
            self._protos, self._structs = _parse(self.header_path)
        return self._protos

    def struct(self, name):
        """The ctypes.Structure of the header's `typedef struct { ... } name;` (a field named like a Python keyword gets
        a trailing underscore: p2r_pw_rjob.in is `in_`)."""
        self.prototypes()
        return self._structs[name]

    def lib(self):
        """The ctypes.CDLL with the header's restype / argtypes on every entry point.  A missing library is an error."""
        if self._handle is None:
            if not os.path.exists(self.lib_path):
                raise P2RLibraryError(
                    f"{self.lib_path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                    "(or `make -C pose2room_amd/csrc`). pose2room_amd has no CPU fallback.")
            try:
                l = ctypes.CDLL(self.lib_path)
            except OSError as e:  # pragma: no cover
                raise P2RLibraryError(f"cannot load {self.lib_path}: {e}") from e
            if self.abi_version is not None:
                l.p2r_abi_version.restype = ctypes.c_int
                if l.p2r_abi_version() != self.abi_version:
                    raise P2RLibraryError(f"{os.path.basename(self.lib_path)} ABI version {l.p2r_abi_version()} != "
                                          f"{self.abi_version}: stale library, rebuild it (make -C pose2room_amd/csrc)")
            for name, proto in self.prototypes().items():
                fn = getattr(l, name)
                fn.restype, fn.argtypes = proto.restype, proto.argtypes
            self._handle = l
        return self._handle

    # The three below run thousands of times per train step: `self._protos or ...` and `self._handle or ...` are the
    # loaded state read without a call.
    def marshal(self, name, args):
        """`args` = the parameters of entry point `name` in header order, without the trailing stream -> the list that
        goes to the library: tensors as their address, None as NULL, integers as Python ints.  Raises TypeError unless
        the count is exact (ctypes accepts surplus arguments) and every argument is of its parameter's kind.  Needs no
        GPU."""
        proto = (self._protos or self.prototypes()).get(name)
        if proto is None:
            raise P2RLibraryError(f"{name} is not declared in {os.path.basename(self.header_path)}")
        if len(args) != len(proto.pointer):
            raise TypeError(f"{name}: {len(args)} arguments for {len(proto.pointer)} parameters"
                            f"{' in front of the stream' if proto.has_stream else ''}: {proto.text}")
        try:        # the common case in one pass: every pointer a tensor or None
            out = [a.data_ptr() if p and a is not None else a for a, p in zip(args, proto.pointer)]
        except AttributeError:      # host arrays (job lists, counts), byref(struct), plain addresses
            out = [_address(proto, i, a) if p and a is not None else a
                   for i, (a, p) in enumerate(zip(args, proto.pointer))]
        for i in proto.scalars:
            if type(out[i]) is not int:
                out[i] = _scalar(proto, i, out[i])
        return out

    def launch_on(self, name, stream, *args):
        """Entry point `name` on `stream` (what `current_stream` returns), for a block of launches under one device
        guard and one stream lookup, both the caller's.  The entry point is looked up at every call: bench.py and the
        tests replace attributes of the library object to time or trap launches."""
        if not (self._protos or self.prototypes())[name].has_stream:
            raise TypeError(f"{name} takes no stream: call lib().{name} directly")
        check(getattr(self._handle or self.lib(), name)(*self.marshal(name, args), stream), name)

    def launch(self, name, device, *args):
        """One launch of entry point `name` on the current stream of `device`, made current for the call; `args` as
        for `marshal`.  Raises when the library returns a non-zero status."""
        import torch
        if device.index is None or device.index == torch.cuda.current_device():
            self.launch_on(name, current_stream(device), *args)     # `device` is current: a guard would change nothing
        else:
            with torch.cuda.device(device):
                self.launch_on(name, current_stream(device), *args)


def extension(name):
    """The Library of extension `name`: libp2r_<name>.so next to libp2r_hip.so, bound from include/p2r_<name>.h."""
    return Library(os.path.join(os.path.dirname(HEADER_PATH), f"p2r_{name}.h"), os.path.join(_HERE, f"libp2r_{name}.so"))


# libp2r_hip.so itself, and its methods under the names the ops, bench.py, the tests and tools/ call
main = Library(HEADER_PATH, LIB_PATH, ABI_VERSION)
lib, marshal, launch_on, launch = main.lib, main.marshal, main.launch_on, main.launch


def prototypes(header_path=None):
    """name -> Prototype of every entry point of p2r_hip.h; with header_path, of that header, read at every call."""
    return main.prototypes() if header_path is None else _parse(header_path)[0]


def struct(name, header_path=None):
    """`Library.struct` of p2r_hip.h; with header_path, of that header, read at every call."""
    return main.struct(name) if header_path is None else _parse(header_path)[1][name]


def sum_leading(part, tr64=False):
    """part [P, ...] f32 (kernel partials, one row per workgroup) -> part.sum(0), optionally with every trailing
    64 x 64 block transposed; one streaming launch (csrc/bn_act.hip: p2r_sum_leading)."""
    import torch
    P = part.shape[0]
    M = part.numel() // P
    if not (part.is_cuda and part.dtype == torch.float32 and part.is_contiguous() and M % 4 == 0
            and part.data_ptr() % 16 == 0):
        out = part.sum(0)
        return out.transpose(-1, -2).contiguous() if tr64 else out
    out = torch.empty(part.shape[1:], dtype=torch.float32, device=part.device)
    launch("p2r_sum_leading", part.device, P, M, part, out, int(bool(tr64)))
    return out
