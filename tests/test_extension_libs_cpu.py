"""CPU: the extension libraries next to libp2r_hip.so as a set.  Each has a source, a header, a name in the Makefile's
EXTS list and one `_lib.Library` object in the module that calls it; this file checks that the three lists agree, that
every library exports exactly what its header declares and nothing another library exports, and that the object every
module launches through refuses a bad call before it reaches the library and calls whatever the library object holds."""
import ctypes
import glob
import importlib
import os
import re
import subprocess

import pytest

from pose2room_amd import _lib

MODULES = {          # name in the Makefile's list -> the module that binds it
    'ap_eval': 'pose2room_amd.net_utils.ap_device', 'mm_eval': 'pose2room_amd.net_utils.mm_device',
    'vote_labels': 'pose2room_amd.net_utils.vote_labels', 'parse': 'pose2room_amd.net_utils.parse_device',
    'scene': 'pose2room_amd.net_utils.scene_device', 'sample_build': 'pose2room_amd.net_utils.sample_build',
    'grad_guard': 'pose2room_amd.p2rnet.grad_guard', 'consensus': 'pose2room_amd.net_utils.consensus_device',
    'occupancy': 'pose2room_amd.net_utils.occupancy_device',
    'recording_repair': 'pose2room_amd.net_utils.recording_repair',
    'interaction': 'pose2room_amd.net_utils.interaction_device',
}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__)))
EINVAL = -22


def _module(name):
    return importlib.import_module(MODULES[name])


def _makefile_exts():
    with open(os.path.join(ROOT, 'pose2room_amd', 'csrc', 'Makefile')) as f:
        m = re.search(r"^EXTS\s*:=\s*(.*)$", f.read(), flags=re.M)
    assert m is not None, "the Makefile has no EXTS list"
    return m.group(1).split()


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("p2r_")}


_exports = {}


def _exports_of(path):          # one nm run per library for the whole file
    if path not in _exports:
        _exports[path] = _exported(path)
    return _exports[path]


# ---- 1. one list in three places ---------------------------------------------------------------------------------------------
def test_headers_makefile_list_and_modules_agree():
    exts = _makefile_exts()
    assert len(exts) == len(set(exts)) == 11 and sorted(exts) == sorted(MODULES)
    headers = {os.path.basename(p) for p in glob.glob(os.path.join(ROOT, 'include', 'p2r_*.h'))}
    assert headers == {'p2r_hip.h'} | {f'p2r_{e}.h' for e in exts}
    for e in exts:
        mod = _module(e)
        assert os.path.basename(mod.LIB_PATH) == f'libp2r_{e}.so'
        assert mod.HEADER_PATH == os.path.join(ROOT, 'include', f'p2r_{e}.h')
        assert os.path.dirname(mod.LIB_PATH) == os.path.dirname(_lib.LIB_PATH)
        assert isinstance(mod._library, _lib.Library)
        assert (mod._library.header_path, mod._library.lib_path) == (mod.HEADER_PATH, mod.LIB_PATH)
        assert mod.lib == mod._library.lib


def test_only_the_loader_opens_libraries():
    """no module outside _lib.py loads a library or sets argtypes itself"""
    pkg = os.path.join(ROOT, 'pose2room_amd')
    for path in glob.glob(os.path.join(pkg, '**', '*.py'), recursive=True):
        if os.path.samefile(path, _lib.__file__):
            continue
        with open(path) as f:
            text = f.read()
        assert 'CDLL(' not in text and not re.search(r"\.argtypes\s*=[^=]", text), path


# ---- 2. what the libraries export ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODULES))
def test_library_exports_exactly_what_its_header_declares(name):
    mod = _module(name)
    protos = mod._library.prototypes()
    assert sorted(protos) == _lib.declared_symbols(mod.HEADER_PATH) and protos
    assert _exports_of(mod.LIB_PATH) == set(protos)


def test_exports_are_pairwise_disjoint_over_all_twelve_libraries():
    paths = [_lib.LIB_PATH] + [_module(e).LIB_PATH for e in sorted(MODULES)]
    assert len(set(paths)) == 12
    assert _exports_of(_lib.LIB_PATH) == set(_lib.prototypes())
    for i, a in enumerate(paths):
        for b in paths[i + 1:]:
            assert not _exports_of(a) & _exports_of(b), (a, b)


# ---- 3. the binding ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODULES))
def test_lib_binds_every_entry_point_from_the_header_once(name):
    mod = _module(name)
    l = mod.lib()
    assert l is mod.lib() is mod._library.lib() and isinstance(l, ctypes.CDLL)
    protos = _lib.prototypes(mod.HEADER_PATH)           # parsed afresh: the object's own parse is not the witness
    for entry, p in protos.items():
        fn = getattr(l, entry)
        assert fn.argtypes == p.argtypes and fn.restype is p.restype
    assert mod._library.prototypes() is mod._library.prototypes()
    with open(mod.HEADER_PATH) as f:
        structs = re.findall(r"\}\s*(\w+)\s*;", re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S))
    for s in structs:
        cls = mod._library.struct(s)
        assert cls is mod._library.struct(s) and issubclass(cls, ctypes.Structure)
        assert [f[0] for f in cls._fields_] == [f[0] for f in _lib.struct(s, mod.HEADER_PATH)._fields_]


def test_module_level_structs_come_from_the_object():
    from pose2room_amd.net_utils import sample_build, vote_labels
    from pose2room_amd.p2rnet import grad_guard
    assert sample_build._Recordings is sample_build._library.struct('p2r_recordings')
    assert sample_build._Plan is sample_build._library.struct('p2r_sample_plan')
    assert vote_labels._Boxes is vote_labels._library.struct('p2r_contact_boxes')
    assert grad_guard.entry_type() is grad_guard._library.struct('p2r_grad_entry') is grad_guard.entry_type()


# ---- 4. marshalling: refused before anything is called; needs no device ---------------------------------------------------------
_NODES = (2, 4, None, None, None, None, 0.5, None, None, None, None, None, None)            # p2r_scene_nodes
_MEASURE = (None, 0, 1.0, 0, 0, None, None, None, None, None, None, None, None, None, None)     # p2r_grad_measure


@pytest.mark.parametrize("name,entry,args", [
    ('scene', 'p2r_scene_nodes', _NODES + (None,)),                           # one too many (ctypes would pass it on)
    ('scene', 'p2r_scene_nodes', _NODES[:-1]),                                # one too few
    ('scene', 'p2r_scene_nodes', (2.0,) + _NODES[1:]),                        # a float where the header says int
    ('scene', 'p2r_scene_nodes', _NODES[:2] + (1.5,) + _NODES[3:]),           # a float where the header says pointer
    ('scene', 'p2r_scene_nodes', _NODES[:6] + ("0.5",) + _NODES[7:]),         # a string where the header says double
    ('grad_guard', 'p2r_grad_measure', _MEASURE + (None,)),
    ('grad_guard', 'p2r_grad_measure', _MEASURE[:-1]),
    ('grad_guard', 'p2r_grad_measure', _MEASURE[:1] + (1.0,) + _MEASURE[2:]),     # n
    ('grad_guard', 'p2r_grad_measure', ("table",) + _MEASURE[1:]),                # a string for the table
    ('grad_guard', 'p2r_grad_measure', _MEASURE[:5] + (1.5,) + _MEASURE[6:]),     # a float for part_sumsq
], ids=["nodes-surplus", "nodes-missing", "nodes-float-for-int", "nodes-float-for-pointer", "nodes-str-for-double",
        "measure-surplus", "measure-missing", "measure-float-for-int", "measure-str-for-pointer",
        "measure-float-for-pointer"])
def test_marshal_refuses_before_anything_is_called(name, entry, args):
    library = _module(name)._library
    l, calls = library.lib(), []
    orig = getattr(l, entry)
    setattr(l, entry, lambda *a: calls.append(a) or 0)
    try:
        with pytest.raises(TypeError) as e:
            library.marshal(entry, args)
        assert entry in str(e.value)
        with pytest.raises(TypeError):
            library.launch_on(entry, ctypes.c_void_p(0), *args)
        assert calls == []
    finally:
        setattr(l, entry, orig)


def test_marshal_passes_what_the_header_allows():
    import torch
    scene, gg = _module('scene')._library, _module('grad_guard')._library
    assert scene.marshal('p2r_scene_nodes', _NODES) == list(_NODES)
    x = torch.zeros(8)
    out = scene.marshal('p2r_scene_nodes', (True, 4, x) + _NODES[3:6] + (1,) + _NODES[7:])      # an int for the double
    assert out[0] == 1 and type(out[0]) is int and out[2] == x.data_ptr() and out[6] == 1
    table = (gg.struct('p2r_grad_entry') * 2)()
    n = ctypes.c_int(0)
    out = gg.marshal('p2r_grad_measure', (table, 2, 0.5, 0, 2, x, ctypes.byref(n), x.data_ptr()) + _MEASURE[8:])
    assert out[0] is table and out[5] == out[7] == x.data_ptr() and out[2] == 0.5
    with pytest.raises(_lib.P2RLibraryError, match="p2r_bn_apply is not declared in p2r_scene.h"):
        scene.marshal('p2r_bn_apply', ())
    with pytest.raises(TypeError, match="takes no stream"):
        _module('consensus')._library.launch_on('p2r_consensus_workspace_bytes', ctypes.c_void_p(0), 1, 1, 1)


# ---- 5. a launch calls what the library object holds at that moment ---------------------------------------------------------------
class _Recorder(object):
    """replaces an entry point on a library object the way bench.py's LaunchTimer and the GPU tests' counters do"""

    def __init__(self, l, name, status=0):
        self.l, self.name, self.status, self.calls = l, name, status, []
        self.orig = getattr(l, name)

    def __enter__(self):
        def wrapper(*args, **kwargs):
            self.calls.append((args, kwargs))
            return self.status
        setattr(self.l, self.name, wrapper)
        return self

    def __exit__(self, *exc):
        setattr(self.l, self.name, self.orig)


def test_launch_calls_the_attribute_the_library_object_holds():
    import torch
    sd = _module('scene')
    joints = torch.zeros(2, 3, 5, 3)                # a CPU tensor: the recorder returns before anything reads it
    count, index, rank = torch.zeros(2, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.int32), None
    stream = ctypes.c_void_p(0)
    orig = sd.lib().p2r_unique_frames
    with _Recorder(sd.lib(), 'p2r_unique_frames') as rec:
        sd._library.launch_on('p2r_unique_frames', stream, joints, 2, 3, 5, 3, count, index, rank)
        (got, kwargs), = rec.calls
    assert sd.lib().p2r_unique_frames is orig                                    # restored
    assert kwargs == {} and got == (joints.data_ptr(), 2, 3, 5, 3, count.data_ptr(), index.data_ptr(), None, stream)
    assert got[-1] is stream and all(type(a) is int for a in got[:7])
    # a non-zero status is check()'s error, with its text
    with _Recorder(sd.lib(), 'p2r_unique_frames', status=EINVAL) as rec:
        with pytest.raises(RuntimeError) as e:
            sd._library.launch_on('p2r_unique_frames', stream, joints, 2, 3, 5, 3, count, index, rank)
        assert len(rec.calls) == 1
    assert str(e.value) == f"libp2r_hip: p2r_unique_frames failed with status {EINVAL}"
    with pytest.raises(RuntimeError) as e2:
        _lib.check(EINVAL, 'p2r_unique_frames')
    assert str(e2.value) == str(e.value)
    # the entry point itself refuses these sizes before it touches a device: the real one is back in place
    assert sd.lib().p2r_unique_frames(None, 2, 0, 5, 3, None, None, None, stream) == EINVAL


# ---- 6. the parser names the header it reads; an explicit path is read at every call ---------------------------------------------
def test_parse_error_names_the_header_being_parsed(tmp_path):
    header = tmp_path / "p2r_other.h"
    header.write_text("int p2r_widget(int n, size_t bytes, void *stream);\n")
    for parse in (lambda: _lib.prototypes(header_path=str(header)), lambda: _lib.struct('p2r_thing', str(header)),
                  lambda: _lib.Library(str(header), str(tmp_path / "libp2r_other.so")).prototypes()):
        with pytest.raises(_lib.P2RLibraryError) as e:
            parse()
        assert "p2r_other.h" in str(e.value) and "p2r_hip.h" not in str(e.value) and "p2r_widget" in str(e.value)
    header.write_text("typedef struct { const float *x; int k; } p2r_thing;\nint p2r_widget(int n, void *stream);\n")
    assert _lib.prototypes(header_path=str(header))['p2r_widget'].kinds == 'i'          # read again, not cached by path
    assert [f[0] for f in _lib.struct('p2r_thing', str(header))._fields_] == ['x', 'k']
    assert _lib.declared_symbols(str(header)) == ['p2r_widget']
    # a Library keeps what it read; its missing library is an error that names the file
    library = _lib.Library(str(header), str(tmp_path / "libp2r_other_absent.so"))
    protos = library.prototypes()
    header.write_text("int p2r_gadget(int n, void *stream);\n")
    assert library.prototypes() is protos and sorted(protos) == ['p2r_widget']
    with pytest.raises(_lib.P2RLibraryError, match="libp2r_other_absent.so is missing.*no CPU fallback"):
        library.lib()
