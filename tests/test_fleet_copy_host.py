"""CPU-only checks of cssm_fleet_copy_series (include/cssm_pf.h, EXTENSION): the binding against the header, the two constants, and the
refusal of null arguments, which is documented as happening before either fleet is looked at -- so it needs no device: the non-null
"fleets" below are addresses that must never be read.  Everything that needs a fleet is in tests/test_gpu_fleet_copy.py.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from composablestatespacemodels_amd import _abi, load_library
from composablestatespacemodels_amd.filter import NativePfFleet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cssm_fleet_copy_series"


def _header():
    return open(os.path.join(ROOT, "include", "cssm_pf.h")).read()


def test_the_call_is_bound_exported_and_declared_as_bound():
    lib = load_library()
    sig = {s[0]: s for s in _abi.SYMBOLS}
    assert NAME in sig and hasattr(lib, NAME)
    m = re.search(r"\bint " + NAME + r"\(([^)]*)\);", _header())
    assert m, f"{NAME} is not declared in include/cssm_pf.h"
    ctype = {"cssm_fleet*": C.c_void_p, "const uint64_t*": C.POINTER(C.c_uint64), "int": C.c_int, "int*": C.POINTER(C.c_int)}
    args = [" ".join(a.split()[:-1]) for a in m.group(1).replace("\n", " ").split(",")]
    assert args == ["cssm_fleet*", "cssm_fleet*", "const uint64_t*", "int", "int*"]      # (map: signed entries in the section's index type)
    assert [ctype[a] for a in args] == list(sig[NAME][2])
    assert sig[NAME][1] is C.c_int


def test_the_constants_have_the_headers_values():
    h = _header()
    keep = re.search(r"#define CSSM_FLEET_COPY_KEEP \((-?\d+)\)", h)
    keys = re.search(r"#define CSSM_FLEET_COPY_KEYS (\d+)\b", h)
    assert keep and keys
    assert _abi.CSSM_FLEET_COPY_KEEP == int(keep.group(1)) == -1
    assert _abi.CSSM_FLEET_COPY_KEYS == int(keys.group(1)) == 1


@pytest.mark.parametrize("null", ["dst", "src", "map", "rc_out"])
def test_a_null_argument_is_refused_without_a_device(null):
    lib = load_library()
    mp = np.zeros(4, dtype=np.int64)
    rc = np.full(4, 77, dtype=np.int32)
    zeros = C.create_string_buffer(1 << 16)               # not a fleet, and never read: the refusal comes before either fleet is looked at
    never_read = C.cast(zeros, C.c_void_p)                # (readable zeroed memory, so that a reordered check fails an assertion, not the process)
    args = {"dst": never_read, "src": never_read, "map": mp.ctypes.data_as(C.POINTER(C.c_uint64)), "rc_out": rc.ctypes.data_as(C.POINTER(C.c_int))}
    args[null] = None
    got = lib.cssm_fleet_copy_series(args["dst"], args["src"], args["map"], 0, args["rc_out"])
    assert got == _abi.CSSM_EINVAL_ARG
    assert "null argument" in _abi.last_error()
    assert (rc == 77).all()


def test_copy_series_refuses_a_map_of_another_length_before_any_call():
    f = NativePfFleet.__new__(NativePfFleet)   # (no device: the check precedes the library call)
    f.S = 3
    with pytest.raises(ValueError, match="one map entry per series"):
        NativePfFleet.copy_series(f, [0, 1])
