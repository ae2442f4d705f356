"""The ctypes binding of include/multiply_hip.h (multiply_amd/hip.py): tensors become device pointers in ONE place (DevPtr), every
status is read by an errcheck, and every launch in the package passes as many arguments as the header declares."""
import ast
import ctypes as C
import glob
import os
import re
import types

import pytest
import torch

from multiply_amd import hip

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOS = hip.header_prototypes()
MODULES = sorted(glob.glob(os.path.join(REPO, "multiply_amd", "*.py")))


def _trees():
    for path in MODULES:
        with open(path) as f:
            yield os.path.basename(path), ast.parse(f.read())


def _functions(tree):
    return [n for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))]


def _direct_calls(tree):
    return [n for n in ast.walk(tree)
            if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr in PROTOS]


def _variable_calls(tree):
    """(call, candidate entry points) of the launches made through a variable: `fn(...)` where the enclosing function picks `fn`
    among entry points it names, and `getattr(lib, name)(...)` / `sizes(...)` with the names of train._FUSED_KINDS"""
    from multiply_amd import train
    size_names = [k[0] for k in train._FUSED_KINDS.values()]
    pack_names = [k[1] for k in train._FUSED_KINDS.values()]
    out = []
    for fn in _functions(tree):
        called = {id(n.func) for n in ast.walk(fn) if isinstance(n, ast.Call)}
        named = sorted({n.attr for n in ast.walk(fn)
                        if isinstance(n, ast.Attribute) and n.attr in PROTOS and id(n) not in called})
        for n in ast.walk(fn):
            if not isinstance(n, ast.Call):
                continue
            f = n.func
            if isinstance(f, ast.Name) and f.id == "fn" and named:
                out.append((n, named))
            elif isinstance(f, ast.Name) and f.id == "sizes":
                out.append((n, size_names))
            elif isinstance(f, ast.Call) and isinstance(f.func, ast.Name) and f.func.id == "getattr" \
                    and ast.unparse(f.args[0]) in ("L", "lib()", "hip.lib()"):
                which = ast.unparse(f.args[1])
                assert which in ("sizes", "self._pack"), which
                out.append((n, size_names if which == "sizes" else pack_names))
    return out


# ------------------------------------------------------------------------------------------------ argument counts
def test_every_launch_passes_as_many_arguments_as_the_header_declares():
    n_sites = 0
    for mod, tree in _trees():
        for call in _direct_calls(tree):
            if any(isinstance(a, ast.Starred) for a in call.args):       # a table of tensors spread over the pointer arguments
                assert mod == "parallel.py" and call.func.attr == "mp_composite", (mod, ast.unparse(call))
                n_sites += 1
                continue
            assert not call.keywords, (mod, ast.unparse(call))
            assert len(call.args) == len(PROTOS[call.func.attr][1]), (mod, call.lineno, call.func.attr)
            n_sites += 1
        for call, names in _variable_calls(tree):
            assert len(names) >= 2 and all(n in PROTOS for n in names), (mod, call.lineno, names)
            arities = {len(PROTOS[n][1]) for n in names}
            assert arities == {len(call.args)} and not call.keywords, (mod, call.lineno, names, arities)
            n_sites += 1
    assert n_sites >= 100, n_sites                                       # the walk found the package's launches


def test_variable_launches_are_all_recognised():
    """gemm_nt / gemm_tn, the f16 / f16x2 pick (twice) and the getattr(lib, ...) launches of the fused kernels' tables"""
    found = {mod: len(_variable_calls(tree)) for mod, tree in _trees()}
    assert found["train.py"] >= 6 and found["hip.py"] >= 1 and found["ray_sampler.py"] >= 1, found


# ------------------------------------------------------------------------------------------------ pointer arguments
class _OnDevice(torch.Tensor):
    """a host tensor that claims to be device-resident (DevPtr's rule is tested without a device)"""
    is_cuda = property(lambda self: True)


def test_pointer_argument_accepts_device_tensors_only():
    t = torch.zeros(4, 4)
    with pytest.raises(AssertionError, match="device-resident contiguous"):
        hip.DevPtr.from_param(t)                                          # host tensor
    d = t.as_subclass(_OnDevice)
    assert hip.DevPtr.from_param(d).value == t.data_ptr()
    assert hip.DevPtr.from_param(d[1:]).value == t.data_ptr() + 16        # a contiguous view: its own first element
    with pytest.raises(AssertionError, match="device-resident contiguous"):
        hip.DevPtr.from_param(d.t())                                      # not contiguous
    with pytest.raises(AssertionError):
        hip.ptr(t)                                                        # the legacy helper: the same rule


def test_pointer_argument_passes_everything_else_through():
    assert hip.DevPtr.from_param(None) is None                            # NULL
    p = C.c_void_p(0x1000)
    assert hip.DevPtr.from_param(p) is p
    net = hip.MpNet()
    assert hip.DevPtr.from_param(C.byref(net)) is not None
    arr = (C.c_float * 3)(1.0, 2.0, 3.0)
    assert hip.DevPtr.from_param(arr) is arr
    hip.DevPtr.from_param(0x2000)                                         # a plain address
    with pytest.raises(TypeError):
        hip.DevPtr.from_param(1.5)


def test_header_prototypes_use_the_pointer_argument_type():
    rt, at = PROTOS["mp_knn_build"]
    assert rt is C.c_int and at == [hip.DevPtr] * 5
    assert issubclass(hip.DevPtr, C.c_void_p)
    assert PROTOS["mp_obb"][1] == [hip.DevPtr, C.c_float, hip.DevPtr, hip.DevPtr]


# ------------------------------------------------------------------------------------------------ status check
def test_errcheck_returns_zero_and_raises_with_the_entry_points_name():
    fn = types.SimpleNamespace(__name__="mp_composite")
    assert hip._errcheck(0, fn, ()) == 0
    with pytest.raises(RuntimeError, match=r"^mp_composite failed with code 7$"):
        hip._errcheck(7, fn, ())
    with pytest.raises(RuntimeError, match=r"mp_composite failed with code -3"):
        hip._errcheck(-3, fn, ())
    hip.check(hip._errcheck(0, fn, ()), "mp_composite")                   # a legacy check(L.mp_x(...), "mp_x") keeps working


def _header_parameters():
    with open(hip.HEADER_PATH) as f:
        txt = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    return {name: [a.strip() for a in args.split(",")]
            for name, args in re.findall(r"\b(mp_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", txt)}


def test_value_returning_entry_points_are_the_only_ones_without_errcheck():
    params = _header_parameters()
    assert set(params) == set(PROTOS)
    for name in hip.VALUE_RETURNING:
        assert name in PROTOS, name
        assert not any("*" in a and re.search(r"\bstream$", a) for a in params[name]), name
    assert PROTOS["mp_arch"][0] is C.c_char_p
    lib = types.SimpleNamespace(**{name: types.SimpleNamespace(__name__=name) for name in PROTOS})
    hip._declare_prototypes(lib)
    for name, (rt, at) in PROTOS.items():
        fn = getattr(lib, name)
        assert fn.restype is rt and fn.argtypes == at
        assert (getattr(fn, "errcheck", None) is hip._errcheck) == (name not in hip.VALUE_RETURNING), name
        if re.search(r"\bvoid\s*\*\s*stream$", params[name][-1]):
            assert fn.errcheck is hip._errcheck and rt is C.c_int, name
    assert len(PROTOS) - len(hip.VALUE_RETURNING) >= 90


# ------------------------------------------------------------------------------------------------ no launch boilerplate
def test_launches_carry_no_pointer_float_or_check_wrappers():
    wrappers = {"hip.ptr", "ptr", "_p", "hip.check", "check", "_chk", "C.c_float", "ctypes.c_float"}

    def name_of(f):
        try:
            return ast.unparse(f)
        except Exception:
            return ""
    for mod, tree in _trees():
        launches = _direct_calls(tree) + [c for c, _ in _variable_calls(tree)]
        for call in launches:
            for arg in call.args:
                for n in ast.walk(arg):
                    if isinstance(n, ast.Call):
                        assert name_of(n.func) not in wrappers, (mod, call.lineno, ast.unparse(n))
        launch_ids = {id(c) for c in launches}
        for n in ast.walk(tree):                                          # ... and no launch's status goes through check(..)
            if isinstance(n, ast.Call) and name_of(n.func) in ("hip.check", "check", "_chk"):
                assert not any(id(a) in launch_ids for a in n.args), (mod, n.lineno)
    from multiply_amd import train
    for mod, tree in _trees():                                            # train keeps the names for callers outside the package only
        assert not [n.lineno for n in ast.walk(tree) if isinstance(n, ast.Call) and name_of(n.func) in ("_p", "_chk")], mod
    assert train._p is hip.ptr and train._chk is hip.check
    assert callable(hip.ptr) and callable(hip.check) and callable(train.off)          # struct fields, offset pointers, tools
