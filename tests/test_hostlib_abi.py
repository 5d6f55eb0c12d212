"""plastid_amd/_hostlib.py -- the ctypes view of the host library -- against the C code it binds: every ``pb_*`` function
defined in csrc/bam_stager.cpp and csrc/host_shims.h is in ``SIGNATURES`` (and nothing else is), resolves in the built
library, takes as many arguments as the table says and returns the kind of value the table says -- a pointer or an
``int64_t`` bound as ``int`` comes back truncated.  No GPU needed."""
import ctypes
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plastid_amd import _hostlib  # noqa: E402
from plastid_amd.exceptions import EngineError  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "plastid_amd", "csrc")
DEFINITION = re.compile(r"^((?:const )?\w+ \*?)\s*(pb_\w+)\(([^)]*)\)\s*\{", re.M)


def definitions():
    """``{name: (return type, [parameters])}`` of the extern "C" definitions."""
    out = {}
    for f in ("bam_stager.cpp", "host_shims.h"):
        for ret, name, params in DEFINITION.findall(open(os.path.join(CSRC, f)).read()):
            assert name not in out, name
            params = " ".join(params.split())
            out[name] = (ret.strip(), [] if params in ("", "void") else params.split(","))
    return out


DEFINED = definitions()


def test_the_table_lists_the_functions_the_c_code_defines_and_the_library_exports_them():
    assert len(DEFINED) >= 70
    assert set(DEFINED) == set(_hostlib.SIGNATURES), set(DEFINED) ^ set(_hostlib.SIGNATURES)
    lib = _hostlib.load()
    for name in DEFINED:
        assert hasattr(lib, name), "library does not export %s" % name


@pytest.mark.parametrize("name", sorted(DEFINED))
def test_argument_count_and_return_type(name):
    ret, params = DEFINED[name]
    restype, argtypes = _hostlib.SIGNATURES[name]
    assert len(argtypes) == len(params), (name, params)
    if "*" in ret:
        assert restype in (ctypes.c_void_p, ctypes.c_char_p), (name, ret)
    else:
        assert restype is {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "void": None, "int": ctypes.c_int}[ret], (name, ret)


def test_a_library_that_lacks_a_symbol_fails_at_load(monkeypatch):
    monkeypatch.setattr(_hostlib, "_lib", None)
    monkeypatch.setattr(_hostlib, "SIGNATURES", dict(_hostlib.SIGNATURES, pb_not_in_the_library=(ctypes.c_int, [])))
    with pytest.raises(EngineError, match=r"pb_not_in_the_library.*python -m plastid_amd\.build --force"):
        _hostlib.load()
    assert _hostlib._lib is None
