"""ctypes binding of csrc/libaft_hip.so -- the stub a maintainer of the reference would add
to call the C ABI of include/adafortitran_amd.h from Python.

There is NO fallback: if the shared library is missing or a symbol is absent this module
raises, and every caller on a HIP device fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # imported first on purpose: binds libamdhip64.so.7 to the runtime torch already uses

from . import _abi

# AFT_LIB_PATH: explicit override for A/B-ing kernel variants (tools/); default = the in-tree build
_LIB_PATH = os.environ.get("AFT_LIB_PATH") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc",
                                                           "libaft_hip.so")
_lib = None


class AftError(RuntimeError):
    pass


def lib_path() -> str:
    return _LIB_PATH


def load():
    """Load the library once and type its entry points."""
    global _lib
    if _lib is None:
        _lib = load_path(_LIB_PATH)
    return _lib


def load_path(path: str):
    """Load and type one build of the library (the product uses exactly one, `load()`; tools/ab_kernels.py loads
    several variants side by side to time them in one process)."""
    if not os.path.exists(path):
        raise AftError(
            f"{path} is missing: build it with `python -m adafortitran_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU or PyTorch fallback for the HIP path.")
    lib = C.CDLL(path)
    for name, (restype, argtypes) in _abi.SIGNATURES.items():       # one table types the whole ABI (tests check it against the header)
        fn = getattr(lib, name, None)
        if fn is None:
            raise AftError(f"{path} does not export {name}")
        fn.restype, fn.argtypes = restype, argtypes
    if lib.aft_version() != _abi.AFT_ABI_VERSION:
        raise AftError(f"ABI mismatch: library {lib.aft_version()} vs binding {_abi.AFT_ABI_VERSION}")
    return lib


def check(rc: int, lib=None) -> None:
    """0 -> ok; argument/shape codes -> ValueError (the reference's convention for bad input,
    fortitran.py:157-158, linear.py:79-83); HIP failures -> RuntimeError.  ``lib``: the build the call was made through
    (``load_path``) when it is not the product's -- the error text is that build's."""
    if rc == _abi.AFT_OK:
        return
    msg = (lib or load()).aft_last_error().decode(errors="replace")
    if rc in (_abi.AFT_ERR_ARG, _abi.AFT_ERR_SHAPE):
        raise ValueError(msg)
    raise AftError(msg)


def set_switch(name: str, value) -> None:
    """A run-time switch (csrc/switches.h declares them; header: aft_set_switch).  The library reads the switches from the environment
    once, when it is loaded; afterwards they change only through this call (``value`` None = unset) -- never through os.environ.
    A name that is not a switch raises ValueError."""
    check(load().aft_set_switch(name.encode(), None if value is None else str(value).encode()))


def get_switch(name: str):
    """Current value of a switch (str) or None when it is unset; ValueError when ``name`` is not a switch."""
    buf = C.create_string_buffer(256)
    rc = load().aft_get_switch(name.encode(), buf, 256)
    if rc < 0:
        raise ValueError(f"{name} is not a switch of the library (adafortitran_amd/csrc/switches.h lists them)")
    return buf.value.decode() if rc else None


class switch:
    """``with _lib.switch("AFT_LANES", 1): ...`` -- set a switch for a block and restore what it was."""

    def __init__(self, name: str, value) -> None:
        self.name, self.value = name, value

    def __enter__(self):
        self.old = get_switch(self.name)
        set_switch(self.name, self.value)
        return self

    def __exit__(self, *exc):
        set_switch(self.name, self.old)
        return False


def current_stream_ptr(device) -> int:
    return int(torch.cuda.current_stream(device).cuda_stream)
