"""CPU checks of the drop-in boundary: the in-tree HIP library loads and exports every symbol that
include/rgbid.h declares (no compute call is made: there is no GPU in the authoring container)."""
import ctypes
import os
import re

from rgbid import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(rgbid_[a-z0-9_]+)\s*\(", txt)))


C_INTEGERS = {"int": (4, True), "int32_t": (4, True), "unsigned": (4, False), "unsigned int": (4, False), "uint32_t": (4, False),
              "long long": (8, True), "int64_t": (8, True), "unsigned long long": (8, False), "uint64_t": (8, False), "size_t": (8, False)}


def _prototypes(header):
    """the `int rgbid_...(...);` prototypes of a C99 header -> {name: [class of each parameter]}: "pointer" (a pointer or an array),
    ("integer", bytes, signed), "float", "double", "struct" (a typedef'd struct by value); a parameter of none of these is an error"""
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    txt = re.sub(r"^[ \t]*#.*$", "", txt, flags=re.M)
    structs = set(re.findall(r"\}\s*(rgbid_\w+)\s*;", txt)) | set(re.findall(r"typedef\s+struct\s+\w+\s+(rgbid_\w+)\s*;", txt))
    out = {}
    for name, params in re.findall(r"\bint\s+(rgbid_\w+)\s*\(([^)]*)\)\s*;", txt):
        classes = []
        for p in [q.strip() for q in params.split(",")]:
            if p == "void" and "," not in params:
                continue
            if "*" in p or "[" in p:
                classes.append("pointer")
                continue
            kind = " ".join(w for w in p.split()[:-1] if w != "const")      # the last word is the parameter's name
            if kind in C_INTEGERS:
                classes.append(("integer",) + C_INTEGERS[kind])
            elif kind in ("float", "double"):
                classes.append(kind)
            elif kind in structs or re.fullmatch(r"rgbid_\w+", kind):
                classes.append("struct")
            else:
                raise AssertionError(f"{header}: {name}: cannot classify the parameter {p!r}")
        out[name] = classes
    return out


def _ctype_class(t):
    """the same classes for a ctypes type of a signature table"""
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, (ctypes._Pointer, ctypes.Array)):
        return "pointer"
    if issubclass(t, ctypes.Structure):
        return "struct"
    if t is ctypes.c_float or t is ctypes.c_double:
        return "float" if t is ctypes.c_float else "double"
    code = getattr(t, "_type_", None)
    if isinstance(code, str) and code in "bhilqBHILQ":
        return ("integer", ctypes.sizeof(t), code.islower())
    raise AssertionError(f"cannot classify the ctypes type {t!r}")


def _signature_mismatches(tables):
    """every (function, parameter index, header's class, table's class) at which {function: tuple of ctypes} departs from the headers"""
    declared = {}
    for path in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if re.fullmatch(r"rgbid_\w+\.h", path):
            declared.update(_prototypes(path))
    bad = []
    for name, types in tables.items():
        if name not in declared:
            bad.append((name, None, "no prototype", None))
            continue
        have = [_ctype_class(t) for t in types]
        if len(have) != len(declared[name]):
            bad.append((name, None, len(declared[name]), len(have)))
        bad += [(name, i, want, got) for i, (want, got) in enumerate(zip(declared[name], have)) if want != got]
    return bad


def _handle_modules():
    """the modules of the package that subclass CtxHandle, by name"""
    import importlib
    pkg = os.path.join(ROOT, "rgbid-slam_amd", "rgbid")
    names = sorted(f[:-3] for f in os.listdir(pkg) if f.endswith(".py") and re.search(r"^class\s+\w+\(_lib\.CtxHandle\)", open(os.path.join(pkg, f)).read(), re.M))
    return {n: importlib.import_module("rgbid." + n) for n in names}


# the modules on the per-frame path or over other libraries: they keep their own bindings (they hold no signature table)
OWN_BINDINGS = ["batched.py", "device.py", "dist.py", "engine.py", "host.py", "kfalign.py", "sequence.py"]


def test_signature_tables_match_the_headers():
    """every binding's table of C functions (SIGNATURES: name -> tuple of ctypes) has, for each function, as many parameters as the
    prototype in include/rgbid_*.h and the prototype's class of each: a pointer, an integer of that width and signedness, float, double, a
    struct by value.  A c_uint where the header says unsigned long long loads, passes every other CPU test and hands a kernel a wrong
    count; here it fails.  EXPORTS is the table's names."""
    mods = _handle_modules()
    assert len(mods) >= 17, sorted(mods)
    tables, without = {}, []
    for name, mod in mods.items():
        if not hasattr(mod, "SIGNATURES"):
            without.append(name + ".py")
            continue
        exports = [n for k, v in vars(mod).items() if k.endswith("EXPORTS") for n in v]      # tsdf lists one per header
        assert set(exports) == set(mod.SIGNATURES) and set(mod.EXPORTS) <= set(mod.SIGNATURES), name
        assert all(isinstance(t, tuple) for t in mod.SIGNATURES.values()), name
        tables.update(mod.SIGNATURES)
    assert without == ["engine.py", "kfalign.py"] and set(without) <= set(OWN_BINDINGS), without
    assert len(tables) >= 115, len(tables)
    bad = _signature_mismatches(tables)
    assert not bad, bad
    # the guard bites: a 64-bit count declared as 32 bits, a dropped parameter and an unknown function are each reported
    wrong = dict(tables)
    wrong["rgbid_meshdist_create"] = tables["rgbid_meshdist_create"][:2] + (ctypes.c_uint,) + tables["rgbid_meshdist_create"][3:]
    wrong["rgbid_mesh_timing"] = tables["rgbid_mesh_timing"][:-1]
    wrong["rgbid_mesh_nothing"] = ()
    assert set(_signature_mismatches(wrong)) == {("rgbid_meshdist_create", 2, ("integer", 8, False), ("integer", 4, False)), ("rgbid_mesh_timing", None, 3, 2),
                                                 ("rgbid_mesh_nothing", None, "no prototype", None)}


def test_library_exports_every_declared_symbol():
    _lib.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared("rgbid.h")
    names += _declared("rgbid_engine.h")
    names += _declared("rgbid_kfalign.h")
    batched = _declared("rgbid_batched.h")
    from rgbid import batched as BT
    assert set(batched) == set(BT.BATCHED_EXPORTS), set(batched) ^ set(BT.BATCHED_EXPORTS)
    names += batched
    assert len(names) >= 90
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing
    # the Python binding's own list must not drift from the header
    assert set(_lib.EXPORTS) <= set(names)


def test_version_and_error_strings():
    L = _lib.lib()
    assert b"gfx950" in L.rgbid_version()
    assert L.rgbid_error_string(0) == b"ok"
    assert b"invalid" in L.rgbid_error_string(-1)


def test_no_device_is_a_loud_error():
    """Without a HIP device the context cannot be created: the product never falls back to a CPU path."""
    import torch
    if torch.cuda.is_available():
        return
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.rgbid_ctx_create(ctypes.byref(h), 0, None) != 0
    assert not h.value


def test_lattice_geometry_host_logic():
    """rgbid_error_lattice_size is pure host logic (sigmaFuncs.cu:712-741): check against the oracle on CPU."""
    from rgbid import device
    from oracle import oracle as O
    import numpy as np
    for rows, cols, ns in [(480, 640, 10000), (240, 320, 10000), (120, 160, 10000), (960, 1280, 10000), (480, 640, 9999999),
                           (61, 83, 100), (64, 64, 1000), (480, 640, 1), (30, 40, 300)]:
        a = np.zeros((rows, cols), np.float32)
        e, geo = O.error_lattice(a, a, ns)
        assert device.error_lattice_size(rows, cols, ns) == (e.size, geo[0], geo[1], geo[2])


def test_host_library_exports_every_declared_symbol():
    """librgbid_host.so (C++ VisodoTracker / KeyframeAlign / settings / SE(3)) exports all of include/rgbid_host.h."""
    from rgbid import host
    L = host.lib()
    names = _declared("rgbid_host.h")
    assert len(names) >= 15
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing


def test_dist_library_exports_every_declared_symbol():
    """librgbid_dist.so (multi-GPU helpers over librccl, include/rgbid_dist.h) loads without a GPU and exports every declared symbol"""
    import pytest
    from rgbid import dist as D
    if not os.path.exists(D.DIST_LIB_PATH) and not os.path.exists("/opt/rocm/include/rccl/rccl.h"):
        pytest.skip("librgbid_dist.so is not built on hosts without RCCL (csrc/Makefile says so); every other library is")
    L = D.dlib()
    names = [n for n in _declared("rgbid_dist.h") if n.startswith("rgbid_dist_")]
    assert len(names) == 15 and set(names) == set(D.DIST_EXPORTS), names
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing
    # the 392-byte record of SURVEY 8e, as the Python harness mirrors it
    assert D.GATHER_DTYPE.itemsize == 392 and D.GATHER_DTYPE.fields["R"][1] == 8 and D.GATHER_DTYPE.fields["cov"][1] == 104


def test_headers_are_valid_c(tmp_path):
    """every C-ABI header compiles as C99 on its own (no C++-isms leaked into the boundary)"""
    import subprocess
    for h in ("rgbid.h", "rgbid_batched.h", "rgbid_engine.h", "rgbid_dist.h", "rgbid_host.h"):
        src = tmp_path / (h + ".c")
        src.write_text(f'#include "{h}"\nint main(void) {{ return 0; }}\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


def test_python_engine_config_matches_the_library():
    """the ctypes mirror of rgbid_engine_config has the size the library was built with (fields are only appended; a stale mirror or a stale library is an error
    the engine constructors report instead of corrupting memory)"""
    import ctypes as C
    from rgbid import engine as E
    L = _lib.lib()
    L.rgbid_engine_config_size.restype = C.c_size_t
    assert L.rgbid_engine_config_size() == C.sizeof(E.EngineConfig)


def test_handles_share_one_host_plumbing():
    """csrc/hip_host.h is the only place that wraps a HIP call into an early return or allocates device / pinned memory, and rgbid/_lib.py
    (CtxHandle) the only lifetime code of the context-bound wrappers: a new feature file takes both from there instead of bringing a copy"""
    import glob
    csrc = os.path.join(ROOT, "rgbid-slam_amd", "csrc")
    macros, allocs = [], []
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h"))):
        name = os.path.basename(path)
        text = open(path).read()
        macros += [(name, m.group(1)) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+).*$", text, re.M) if "HIP" in m.group(0)]
        if name != "hip_host.h":
            allocs += [(name, m) for m in re.findall(r"\b(hipMalloc|hipHostMalloc|hipMallocPitch|hipMallocAsync|hipMallocManaged)\s*\(", text)]
    assert macros == [("hip_host.h", "RGBID_HIP")], macros
    assert not allocs, allocs
    pkg = os.path.join(ROOT, "rgbid-slam_amd", "rgbid")
    dels = sorted(f for f in os.listdir(pkg) if f.endswith(".py") and re.search(r"def\s+__del__", open(os.path.join(pkg, f)).read()))
    assert dels == ["_lib.py", "device.py", "host.py"], dels
    # the Python side of a binding comes from rgbid/_args.py (checks) and rgbid/_lib.py (signature tables, handle helpers) alone
    src = {f: open(os.path.join(pkg, f)).read() for f in sorted(os.listdir(pkg)) if f.endswith(".py")}
    integer_tests = [f for f, text in src.items() if re.search(r"isinstance\(\w+, bool\) or not isinstance\(\w+, \(int, np\.integer\)\)", text)]
    assert integer_tests == ["_args.py"], integer_tests
    binders = [f for f, text in src.items() if re.search(r"\.argtypes\s*=", text)]
    assert set(binders) <= {"_lib.py"} | set(OWN_BINDINGS) and "_lib.py" in binders, binders
    features = {f[:-3] for f in src if not f.startswith("_") and f not in OWN_BINDINGS}      # those keep their private helpers to themselves and to tum.py
    aliases = {f: dict(re.findall(r"^\s*from \. import (\w+) as (\w+)$", text, re.M)) for f, text in src.items()}
    reach = []
    for f, text in src.items():
        names = {alias: mod for mod, alias in aliases[f].items() if mod in features}
        names.update({m: m for m in re.findall(r"^\s*from \. import (\w+)$", text, re.M) if m in features})
        reach += [(f, m.group(0)) for m in re.finditer(r"\b(\w+)\._[a-z]\w*", text) if names.get(m.group(1), f[:-3]) != f[:-3]]
        reach += [(f, m.group(0)) for m in re.finditer(r"^\s*from \.(\w+) import (.*)$", text, re.M)
                  if m.group(1) in features and re.search(r"(^|,\s*)_[a-z]", m.group(2))]
    assert not reach, reach
