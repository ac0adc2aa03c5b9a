"""The kernel launchers' ctypes signatures come from the ``PBX_EXPORT`` prototypes (``ops/_lib.py``).

CPU half: reads sources only, never loads a library -- every prototype parses, and every ``_lib.call`` /
``lib().pbx_*`` site in the tree passes as many arguments as its prototype declares (a miscount would pass a
device pointer as a 32-bit int: a fault on the GPU, so it is caught here first).  GPU half: the loaded
``libpbx_hip.so`` and the parsed table name the same launchers."""
import ast
import ctypes
import glob
import os
import re
import shutil
import subprocess

import pytest

from proteinbert_pytorch_replication_amd.ops import _lib
from proteinbert_pytorch_replication_amd.ops.build import CSRC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOWN_CTYPES = {ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_int64,
                ctypes.c_float}


def test_every_export_is_parsed_with_known_types():
    uses = 0
    for f in glob.glob(os.path.join(CSRC, "*.hip")):
        with open(f) as fh:
            uses += len(re.findall(r"\bPBX_EXPORT\b", fh.read()))
    table = _lib.launchers()
    assert uses > 0 and len(table) == uses
    for name, args in table.items():
        assert name.startswith("pbx_"), name
        assert all(a in KNOWN_CTYPES for a in args), (name, args)


def _call_sites():
    """(file:line, launcher name, positional argument nodes) of every ``_lib.call("<literal>", ...)`` and
    ``lib().pbx_*(...)`` in the package, the tests, the tools and bench.py."""
    files = [os.path.join(ROOT, "bench.py")]
    for d in ("proteinbert_pytorch_replication_amd", "tests", "tools"):
        files += glob.glob(os.path.join(ROOT, d, "**", "*.py"), recursive=True)
    sites = []
    for f in files:
        with open(f) as fh:
            tree = ast.parse(fh.read(), f)
        for n in ast.walk(tree):
            if not (isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute)):
                continue
            where, fn = f"{os.path.relpath(f, ROOT)}:{n.lineno}", n.func
            if (fn.attr == "call" and isinstance(fn.value, ast.Name) and fn.value.id == "_lib" and n.args
                    and isinstance(n.args[0], ast.Constant) and isinstance(n.args[0].value, str)):
                sites.append((where, n.args[0].value, n.args[1:]))
            elif fn.attr.startswith("pbx_") and isinstance(fn.value, ast.Call):
                inner = fn.value.func
                if (inner.attr if isinstance(inner, ast.Attribute) else getattr(inner, "id", None)) == "lib":
                    sites.append((where, fn.attr, n.args))
    return sites


def test_every_call_site_matches_its_prototype():
    table = _lib.launchers()
    sites = _call_sites()
    assert {"pbx_gemm", "pbx_local_head3_a", "pbx_local_head3_tiles"} <= {name for _, name, _ in sites}
    for where, name, args in sites:
        assert name in table, f"{where}: {name} is not a PBX_EXPORT launcher"
        plain, want = [a for a in args if not isinstance(a, ast.Starred)], len(table[name])
        if len(plain) < len(args):
            assert len(plain) <= want, f"{where}: {name} takes {want} arguments"
        else:
            assert len(args) == want, f"{where}: {name} takes {want} arguments, {len(args)} passed"


@pytest.mark.parametrize("proto", [
    "PBX_EXPORT int pbx_bad(const float* x, double scale, hipStream_t st) { return 0; }",
    "PBX_EXPORT void pbx_bad(const float* x, hipStream_t st) {}",
    "PBX_EXPORT int pbx_bad(const float* x, int (*cb)(int), hipStream_t st) { return 0; }",
], ids=["double_param", "void_return", "parenthesised_param"])
def test_parser_rejects_unsupported_prototype(proto):
    good = "PBX_EXPORT int pbx_good(const float* __restrict__ x,\n    long long n, // count\n    hipStream_t st);\n"
    assert _lib.parse_launchers(good, "t.hip") == {"pbx_good": [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]}
    with pytest.raises(_lib.HipError, match=r"t\.hip.*pbx_bad"):
        _lib.parse_launchers(good + proto, "t.hip")


def test_unknown_launcher_raises_before_any_library_is_loaded(monkeypatch):
    def no_load():
        raise AssertionError("the library must not be loaded for an unknown launcher")
    monkeypatch.setattr(_lib, "lib", no_load)
    name = "pbx_no_such_launcher"
    with pytest.raises(_lib.HipError, match=name):
        _lib.call(name)
    assert name not in _lib._FN


@pytest.mark.gpu
def test_loaded_library_and_table_agree():
    lib = _lib.lib()
    table = _lib.launchers()
    for name, args in table.items():
        fn = getattr(lib, name, None)
        assert fn is not None, f"{name}: not exported by {_lib.HIP_LIB}"
        assert list(fn.argtypes) == args and fn.restype is ctypes.c_int, name
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin")
    if nm is None:
        pytest.skip("no nm: the library's dynamic symbols were not compared with the table (the first half passed)")
    out = subprocess.run([nm, "-D", "--defined-only", _lib.HIP_LIB], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("pbx_")}
    assert exported and exported <= set(table), sorted(exported - set(table))
