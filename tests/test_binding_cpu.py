"""The Python binding of the C ABI is generated from include/p2r_hip.h (pose2room_amd/_lib.py): argtypes and restype of
every entry point, the ctypes mirror of every struct, and the launch helper's checks -- all without a GPU (the library
itself is needed, as in test_abi.py)."""
import ctypes
import keyword
import os
import re
import shutil
import subprocess

import pytest
import torch

from pose2room_amd import _lib

STRUCTS = ('p2r_pw_job', 'p2r_pw_wjob', 'p2r_pw_bnjob', 'p2r_pw_bnbjob', 'p2r_pw_rjob', 'p2r_mix_head',
           'p2r_mdn_sample_head', 'p2r_mdn_sample_head_ex', 'p2r_sample_store', 'p2r_batch_out')
EINVAL = -22


def _position(name, param):
    """index of parameter `param` in the header's prototype of `name`"""
    params = re.search(r"\((.*)\)", _lib.prototypes()[name].text).group(1).split(",")
    return [re.search(r"(\w+)\s*$", p).group(1) for p in params].index(param)


# ---- 1. argtypes from the header ---------------------------------------------------------------------------------------
def test_every_entry_point_has_the_headers_argtypes():
    l = _lib.lib()
    protos = _lib.prototypes()
    assert sorted(protos) == _lib.declared_symbols() and len(protos) == 75
    for name, proto in protos.items():
        fn = getattr(l, name)
        params = re.search(r"\((.*)\)", proto.text).group(1)
        count = 0 if params.strip() == "void" else params.count(",") + 1
        assert fn.argtypes is not None and len(fn.argtypes) == count, proto.text
        assert fn.restype in (ctypes.c_int, ctypes.c_ulonglong, ctypes.c_char_p), proto.text
        assert len(proto.kinds) == count - proto.has_stream
    assert sum(p.argtypes.count(ctypes.c_void_p) for p in protos.values()) == 477


def test_argtypes_spot_checks():
    l = _lib.lib()
    assert _position('p2r_ball_query', 'radius') == 3
    assert l.p2r_ball_query.argtypes[3] is ctypes.c_float
    assert l.p2r_nms3d.argtypes[_position('p2r_nms3d', 'overlap_threshold')] is ctypes.c_double
    assert l.p2r_sum_leading.argtypes[_position('p2r_sum_leading', 'M')] is ctypes.c_longlong
    assert l.p2r_mdn_sample.argtypes[_position('p2r_mdn_sample', 'seed')] is ctypes.c_ulonglong      # the Philox key
    assert l.p2r_rowsum_short.argtypes[0] is ctypes.c_longlong
    assert l.p2r_bn_finalize.argtypes[_position('p2r_bn_finalize', 'eps')] is ctypes.c_double
    assert l.p2r_build_arch.restype is ctypes.c_char_p and l.p2r_abi_version.restype is ctypes.c_int
    for name in ('p2r_stgcn_gcn3_signature', 'p2r_stgcn_gcn3h_signature', 'p2r_stgcn_gcn3h_weight_grad_signature'):
        assert getattr(l, name).restype is ctypes.c_ulonglong
    # every pointer, whatever it points to, and the stream
    assert set(l.p2r_gather_points.argtypes[4:]) == {ctypes.c_void_p}
    assert l.p2r_stgcn_gcn2_forward.argtypes[-1] is ctypes.c_void_p and _lib.prototypes()['p2r_stgcn_gcn2_forward'].has_stream
    assert not _lib.prototypes()['p2r_stgcn_gcn3h_pairs'].has_stream


@pytest.mark.parametrize("decl,named", [
    ("int p2r_widget(int n, size_t bytes, void *stream);", "p2r_widget"),
    ("short p2r_widget(int n, void *stream);", "p2r_widget"),
    ("float *p2r_widget(int n);", "p2r_widget"),
    ("int p2r_widget(int n, int (*callback)(int), void *stream);", "p2r_widget"),
    ("typedef struct p2r_thing { const float *x; short k; } p2r_thing;", "p2r_thing"),
])
def test_unmapped_type_fails_to_bind_and_names_the_declaration(tmp_path, decl, named):
    header = tmp_path / "p2r_hip.h"
    header.write_text("/* a header */\n#define P2R_OK 0\nint p2r_abi_version(void);\n" + decl + "\n")
    with pytest.raises(_lib.P2RLibraryError) as e:
        _lib.prototypes(header_path=str(header))
    assert named in str(e.value)
    header.write_text("int p2r_abi_version(void);\nint p2r_widget(int n, double x, const long long *p, void *stream);\n")
    protos = _lib.prototypes(header_path=str(header))
    assert protos['p2r_widget'].argtypes == (ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p)
    assert protos['p2r_widget'].kinds == 'ifp'


# ---- 2. struct layout against the compiler ---------------------------------------------------------------------------
def _c_compiler():
    for cc in ('cc', 'gcc', 'clang'):
        if shutil.which(cc):
            return shutil.which(cc)
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    for cc in (os.path.join(rocm, 'llvm', 'bin', 'clang'), os.path.join(rocm, 'lib', 'llvm', 'bin', 'clang')):
        if os.path.exists(cc):
            return cc
    pytest.fail("no C compiler found (cc, gcc, clang, the ROCm clang): the struct layout cannot be checked")


def test_struct_layouts_match_the_compiler(tmp_path):
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    assert sorted(re.findall(r"\}\s*(\w+)\s*;", text)) == sorted(STRUCTS)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "p2r_hip.h"', 'int main(void) {']
    for s in STRUCTS:
        lines.append(f'  printf("{s} sizeof %zu\\n", sizeof({s}));')
        for field, _ in _lib.struct(s)._fields_:
            c_name = field[:-1] if field.endswith('_') and keyword.iskeyword(field[:-1]) else field
            lines.append(f'  printf("{s} {field} %zu\\n", offsetof({s}, {c_name}));')
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([_c_compiler(), "-std=c99", "-I", os.path.dirname(_lib.HEADER_PATH), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {tuple(ln.split()[:2]): int(ln.split()[2]) for ln in out.splitlines()}
    want = {}
    for s in STRUCTS:
        cls = _lib.struct(s)
        assert issubclass(cls, ctypes.Structure)
        want[s, 'sizeof'] = ctypes.sizeof(cls)
        for field, _ in cls._fields_:
            want[s, field] = getattr(cls, field).offset
    assert got == want
    assert 'in_' in dict(_lib.struct('p2r_pw_rjob')._fields_)        # `in` is a Python keyword


def test_op_modules_use_the_generated_structs():
    from pose2room_amd.p2rnet import device_loader, mdn_sample_op, pw_op
    assert pw_op._Job is _lib.struct('p2r_pw_job') and pw_op._WJob is _lib.struct('p2r_pw_wjob')
    assert pw_op._BnJob is _lib.struct('p2r_pw_bnjob') and pw_op._BnbJob is _lib.struct('p2r_pw_bnbjob')
    assert pw_op._RJob is _lib.struct('p2r_pw_rjob') and pw_op._MixHead is _lib.struct('p2r_mix_head')
    assert mdn_sample_op._SampleHead is _lib.struct('p2r_mdn_sample_head')
    assert mdn_sample_op._SampleHeadEx is _lib.struct('p2r_mdn_sample_head_ex')
    assert device_loader._Store is _lib.struct('p2r_sample_store') and device_loader._Out is _lib.struct('p2r_batch_out')
    # built by keyword from ptr() values, addresses and None, as the tests and the ops do
    t = torch.zeros(4)
    j = pw_op._RJob(in_=_lib.ptr(t), out=t.data_ptr(), P=3, M=8)
    assert j.in_ == t.data_ptr() == j.out and (j.P, j.M) == (3, 8)
    b = pw_op._BnJob(part=None, eps=1e-5, momentum=-1.0, C=64)
    assert b.part is None and b.eps == 1e-5 and b.momentum == -1.0 and b.C == 64


# ---- 3. / 4. the launch helper -----------------------------------------------------------------------------------------
class _Recorder(object):
    """replaces an entry point on the library object the way bench.py's LaunchTimer does"""

    def __init__(self, name):
        self.name, self.lib, self.calls = name, _lib.lib(), []
        self.orig = getattr(self.lib, name)

    def __enter__(self):
        def wrapper(*args, **kwargs):
            self.calls.append((args, kwargs))
            return self.orig(*args)
        setattr(self.lib, self.name, wrapper)
        return self

    def __exit__(self, *exc):
        setattr(self.lib, self.name, self.orig)


_NAME = 'p2r_stgcn_tconv_weight_grad'
_GOOD = (2, 16, 65, 3, None, None, None, None, 256, None, None)           # V = 65: P2R_EINVAL before the device is touched


@pytest.mark.parametrize("args", [
    _GOOD + (None,),                                      # one too many (ctypes would pass it on)
    _GOOD[:-1],                                           # one too few
    (2.0,) + _GOOD[1:],                                   # a float where the header says int
    _GOOD[:4] + ("x",) + _GOOD[5:],                       # a string where the header says pointer
    _GOOD[:4] + (1.5,) + _GOOD[5:],                       # a float where the header says pointer
], ids=["surplus", "missing", "float-for-int", "str-for-pointer", "float-for-pointer"])
def test_helper_refuses_before_it_calls(args):
    stream = ctypes.c_void_p(0)
    with _Recorder(_NAME) as rec:
        with pytest.raises(TypeError) as e:
            _lib.launch_on(_NAME, stream, *args)
        assert rec.calls == []
    assert _NAME in str(e.value)
    with pytest.raises(TypeError):
        _lib.marshal(_NAME, args)


def test_helper_refuses_scalar_kinds():
    m = _lib.marshal
    with pytest.raises(TypeError):
        m('p2r_sum_leading', (3, 8.0, None, None, 0))                        # long long M
    with pytest.raises(TypeError):
        m('p2r_ball_query', (1, 8, 2, "0.3", 4, None, None, None))          # float radius
    with pytest.raises(TypeError):
        m('p2r_ball_query', (1, 8, 2, torch.tensor(0.3), 4, None, None, None))
    with pytest.raises(_lib.P2RLibraryError):
        m('p2r_no_such_entry', ())
    with pytest.raises(TypeError):                                           # no stream parameter: not a launch
        _lib.launch_on('p2r_stgcn_gcn3_signature', ctypes.c_void_p(0), 0)
    # what does pass: ints (also > 2^31 for long long / unsigned long long), an int for a double, host arrays, byref
    big = 3 * 2 ** 31
    assert m('p2r_sum_leading', (3, big, None, None, 0))[1] == big
    assert m('p2r_bn_bwd_finalize', (1, 64, None, 1024, None))[3] == 1024
    arr, n = (ctypes.c_int * 4)(), ctypes.c_int(0)
    out = m('p2r_stgcn_tconv_forward', (2, 16, 20, 3, None, None, None, None, None, None, arr, ctypes.byref(n)))
    assert out[10] is arr


@pytest.mark.parametrize("name,V", [('p2r_stgcn_tconv_weight_grad', 65), ('p2r_stgcn_tconv_weight_grad_dz', 20)])
def test_what_the_helper_passes_on(name, V):
    x = torch.arange(8, dtype=torch.float32)              # a CPU tensor: the entry point returns before it reads anything
    stream = ctypes.c_void_p(0)
    if name == 'p2r_stgcn_tconv_weight_grad':
        args = (2, 16, V, True, x, None, None, None, 256, None, None)
    else:
        args = (2, 16, V, True, x, None, None, None, None, None, 256, None, None)
    with _Recorder(name) as rec:
        with pytest.raises(RuntimeError) as e:
            _lib.launch_on(name, stream, *args)
        assert name in str(e.value) and str(EINVAL) in str(e.value)
        assert str(e.value) == f"libp2r_hip: {name} failed with status {EINVAL}"
        (got, kwargs), = rec.calls
    assert getattr(_lib.lib(), name) is rec.orig                             # restored
    assert kwargs == {} and len(got) == len(args) + 1 and got[-1] is stream
    for a in (got[0], got[1], got[2], got[3]):
        assert isinstance(a, int)
    assert got[:4] == (2, 16, V, 1) and got[3] == 1
    assert type(got[4]) is int and got[4] == x.data_ptr()
    assert not any(torch.is_tensor(a) for a in got)
    for a in got[5:8]:
        assert a is None or getattr(a, 'value', a) in (None, 0)             # bench.py's `_null`
    # the raw style still works next to it (tests and tools call the library this way)
    n = None
    assert getattr(_lib.lib(), name)(2, 16, V, 3, _lib.ptr(x), *([n] * (len(args) - 5 - 3)), 256, n, n, stream) == EINVAL
