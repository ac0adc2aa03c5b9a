"""ctypes binding of the in-tree HIP library (``libpbx_hip.so``).

The library must be loaded *after* ``import torch`` so that it binds to the
HIP runtime torch already loaded (same ``libamdhip64.so.7`` soname).  Every
launcher returns a ``hipError_t``; a non-zero code raises.  On a GPU box a
missing library is an error, never a silent fallback to eager ops.
"""
from __future__ import annotations

import ctypes
import glob
import os
import re
from typing import Dict, Optional

import torch

from .build import CSRC, HIP_LIB as _BUILT_HIP_LIB, HIP_LIB_EXACT as _BUILT_HIP_LIB_EXACT, HOST_LIB

GELU_MODES = ("fitted", "exact")


def _default_lib() -> str:
    mode = os.environ.get("PBX_GELU", "fitted")
    if mode not in GELU_MODES:
        raise ValueError(f"PBX_GELU={mode!r}: expected one of {GELU_MODES}")
    return _BUILT_HIP_LIB_EXACT if mode == "exact" else _BUILT_HIP_LIB


# The GELU core of the fused kernels: "fitted" (libpbx_hip.so, the default) or "exact" (libpbx_hip_exact.so,
# the erf form of the reference's nn.GELU()), chosen by PBX_GELU / set_gelu() before the first kernel launch.
# PBX_HIP_LIB: load any other build of the kernel library (A/B comparisons of kernel variants).
HIP_LIB = os.environ.get("PBX_HIP_LIB") or _default_lib()


def gelu_mode() -> str:
    return "exact" if HIP_LIB == _BUILT_HIP_LIB_EXACT else ("fitted" if HIP_LIB == _BUILT_HIP_LIB else "custom")


def set_gelu(mode: str) -> None:
    """Select the fused kernels' GELU core ("fitted" | "exact") for this process.  Must precede the first
    kernel launch (the library is loaded once); a later call with another mode raises."""
    global HIP_LIB
    if mode not in GELU_MODES:
        raise ValueError(f"gelu mode {mode!r}: expected one of {GELU_MODES}")
    want = _BUILT_HIP_LIB_EXACT if mode == "exact" else _BUILT_HIP_LIB
    if want == HIP_LIB:
        return
    if _lib is not None:
        raise HipError(f"set_gelu({mode!r}): the kernel library ({HIP_LIB}) is already loaded")
    HIP_LIB = want
    os.environ["PBX_GELU"] = mode     # child processes (DP ranks spawned later) inherit the choice


class HipError(RuntimeError):
    pass


# The C prototypes are the ABI: every ``PBX_EXPORT int name(params)`` of csrc/*.hip is a launcher, and its
# ctypes signature is derived from the declared parameter types (adding a launcher needs no Python declaration).
_CTYPES = {"int": ctypes.c_int, "long": ctypes.c_long, "long long": ctypes.c_longlong,
           "unsigned long long": ctypes.c_ulonglong, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
_TYPE_WORDS = {w for t in _CTYPES for w in t.split()} | {"signed", "short", "char", "double", "void"}
_COMMENT = re.compile(r"//[^\n]*|/\*.*?\*/", re.S)
_PROTO = re.compile(r"\bPBX_EXPORT\b([^(;{}]*)\(([^)]*)\)\s*(.)", re.S)


def parse_launchers(text: str, where: str) -> Dict[str, list]:
    """name -> ctypes argtypes of every ``PBX_EXPORT int name(params)`` in one source text.  A pointer or a
    ``hipStream_t`` is a ``c_void_p``; any other type outside ``_CTYPES`` is an error naming the function,
    never a guess: an unsupported prototype fails at import on the CPU, not as a bad call on the GPU."""
    text = _COMMENT.sub(" ", text)
    table: Dict[str, list] = {}
    for m in _PROTO.finditer(text):
        head, params, after = m.group(1).split(), m.group(2), m.group(3)
        name = head[-1] if head else "?"
        err = f"{where}: PBX_EXPORT {name}: "
        if head[:-1] != ["int"]:
            raise HipError(err + f"return type {' '.join(head[:-1])!r}: launchers return int (hipError_t)")
        if "(" in params or after not in "{;":
            raise HipError(err + "parentheses in the parameter list (function pointers, macros) are not supported")
        args = []
        for p in ([] if params.strip() in ("", "void") else params.split(",")):
            words = [w for w in p.split() if w not in ("const", "__restrict__")]
            if "*" in p or "hipStream_t" in words:
                args.append(ctypes.c_void_p)
                continue
            ctype = _CTYPES.get(" ".join(words[:-1]))      # the last word is the parameter's name
            if ctype is None or words[-1] in _TYPE_WORDS:
                raise HipError(err + f"parameter {' '.join(p.split())!r}: unsupported type")
            args.append(ctype)
        table[name] = args
    if len(table) != len(re.findall(r"\bPBX_EXPORT\b", text)):
        raise HipError(f"{where}: a PBX_EXPORT use is not of the form `PBX_EXPORT int name(params)`")
    return table


_TABLE: Optional[Dict[str, list]] = None


def launchers() -> Dict[str, list]:
    """The launcher table of ``csrc/*.hip``, parsed at the first ``lib()`` or ``call()``."""
    global _TABLE
    if _TABLE is None:
        table: Dict[str, list] = {}
        for f in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
            with open(f) as fh:
                table.update(parse_launchers(fh.read(), os.path.basename(f)))
        _TABLE = table
    return _TABLE


_lib: Optional[ctypes.CDLL] = None
_host: Optional[ctypes.CDLL] = None


def available() -> bool:
    return os.path.exists(HIP_LIB)


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(HIP_LIB):
            raise HipError(f"HIP kernel library not built: {HIP_LIB}. "
                           f"Run `python -m proteinbert_pytorch_replication_amd.ops.build`.")
        _ = torch.cuda.is_available()  # make sure torch's HIP runtime is loaded first
        _lib = ctypes.CDLL(HIP_LIB, mode=ctypes.RTLD_LOCAL)
        for name, args in launchers().items():
            fn = getattr(_lib, name, None)
            if fn is None:       # an older A/B build (PBX_HIP_LIB) without this launcher: call() raises
                continue
            fn.argtypes, fn.restype = args, ctypes.c_int
    return _lib


def host_lib() -> ctypes.CDLL:
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB):
            raise HipError(f"host library not built: {HOST_LIB}")
        _host = ctypes.CDLL(HOST_LIB, mode=ctypes.RTLD_LOCAL)
    return _host


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_ptr(device: Optional[torch.device] = None) -> int:
    """Raw hipStream_t of the current stream (the step issues ~200 launches: the torch.cuda.Stream
    wrapper object per launch cost ~8 us of host time each)."""
    if _raw_stream is not None:
        idx = device.index if device is not None and device.index is not None else torch.cuda.current_device()
        return _raw_stream(idx)
    return torch.cuda.current_stream(device).cuda_stream


_FN = {}


def call(name: str, *args) -> None:
    fn = _FN.get(name)
    if fn is None:
        if name not in launchers():   # untyped, ctypes would pass Python ints as 32-bit C ints and truncate pointers
            raise HipError(f"{name}: no PBX_EXPORT launcher of that name in {CSRC}")
        fn = getattr(lib(), name, None)
        if fn is None:
            raise HipError(f"{name}: not exported by {HIP_LIB}")
        _FN[name] = fn
    rc = fn(*args)
    if rc != 0:
        raise HipError(f"{name} failed with hipError {rc}")


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()
