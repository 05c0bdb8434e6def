"""ctypes binding of libdawn_hip.so.  include/dawn_hip.h is the one definition of the C ABI: :func:`lib` reads every function's
argument and return types from it (abi.py); to add an entry point, declare it there.  The struct mirrors (here, ctx.py, bundle.py) stay
hand-written -- their pointer fields say which are host arrays, which the header cannot -- and tests/test_cabi_cpu.py checks each
against the header's layout.

The library is mandatory: there is NO CPU / eager fallback on the product path.  Import of this module
never fails (so that host-side logic stays testable without a GPU), but :func:`lib` raises loudly when
the shared object or the header is missing or cannot be loaded."""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

from . import abi

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("DAWN_HIP_LIB", str(_HERE / "libdawn_hip.so")))
HEADER_PATH = Path(os.environ.get("DAWN_HIP_HEADER", str(_HERE.parent / "include" / "dawn_hip.h")))

c_f = C.c_void_p          # device pointers travel as void*
_i, _f = C.c_int, C.c_float


class ConvDesc(C.Structure):
    """Mirror of ``dawn_conv_desc`` (include/dawn_hip.h)."""
    _fields_ = [
        ("in0", c_f), ("in1", c_f),
        ("C0", _i), ("C1", _i), ("ld0", _i), ("ld1", _i),
        ("F", _i), ("Hi", _i), ("Wi", _i), ("Ho", _i), ("Wo", _i),
        ("KH", _i), ("KW", _i), ("stride", _i), ("pad", _i),
        ("mode", _i),
        ("w", c_f), ("bias", c_f),
        ("N", _i),
        ("row_mean", c_f), ("row_rstd", c_f),
        ("ch_a", c_f), ("ch_b", c_f),
        ("pro_act", _i),
        ("pro_add", c_f), ("ld_add", _i),
        ("res", c_f), ("ld_res", _i),
        ("tr", c_f), ("ld_tr", _i),
        ("tr_a", c_f), ("tr_b", c_f),
        ("out", c_f), ("ld_out", _i),
        ("gn_part", c_f),
        ("w_bf3", c_f),
        ("gn_rows", C.POINTER(C.c_int)),
        ("policy", _i),
        ("ln_eps", _f),
        ("sk_ws", c_f), ("sk_ws_bytes", C.c_size_t),
        ("w_wino", c_f),
        ("gn_gamma", c_f), ("gn_beta", c_f), ("gn_fs", c_f), ("gn_fsh", c_f),
        ("gn_count", C.c_double), ("gn_eps", _f),
        ("gn_a", c_f), ("gn_b", c_f),
        ("gn_ticket", c_f),
        ("w_wino4", c_f),
        ("border", _i),
    ]


class DawnHipError(RuntimeError):
    pass


def _declared():
    """(DAWN_ABI_VERSION, {name: (restype, argtypes)}) as the header declares them."""
    if not HEADER_PATH.exists():
        raise DawnHipError(f"{HEADER_PATH} not found: the binding reads every signature from it (DAWN_HIP_HEADER names another place)")
    text = HEADER_PATH.read_text()
    return abi.defines(text).get("DAWN_ABI_VERSION"), abi.functions(text)


# name -> argtypes of every function include/dawn_hip.h declares, the ones lib() binds
try:
    SIGNATURES = {name: argtypes for name, (_, argtypes) in _declared()[1].items()}
except (DawnHipError, abi.HeaderError):     # importing never fails: lib() raises it again
    SIGNATURES = {}

_lib = None


def lib() -> C.CDLL:
    """Load libdawn_hip.so once and give every function the header declares its argtypes and restype; raise (never fall back) if
    the library or the header is absent, or if the library was built from a header with another DAWN_ABI_VERSION."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise DawnHipError(
                f"{LIB_PATH} not found: the HIP extension is mandatory (no CPU fallback). "
                "Build it with `python -c 'import __graft_entry__ as g; g.build()'` or ./build_lib.sh")
        want, functions = _declared()
        L = C.CDLL(str(LIB_PATH))
        L.dawn_abi_version.restype = C.c_int
        got = L.dawn_abi_version()
        if want != got:
            raise DawnHipError(f"{LIB_PATH} has ABI version {got}, {HEADER_PATH} declares DAWN_ABI_VERSION {want}: rebuild the library")
        for name, (restype, argtypes) in functions.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise DawnHipError(f"{what} failed with code {rc}: {lib().dawn_last_error().decode()}")
