"""The C-ABI shared library loads and exports every symbol include/lidarslam_amd.h declares
(no compute calls without a GPU), and fails loudly -- never falls back -- when no device exists.
The front end's one signature table (lidarslam_amd/_abi.py) and its struct mirrors are held to the header."""
import copy
import ctypes as C
import glob
import importlib.util
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    src = open(os.path.join(ROOT, "include", "lidarslam_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(lsa_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_are_exported(L):
    lib = L.lib()
    names = declared_functions()
    assert len(names) > 50
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, f"declared in the header but not exported: {missing}"


def test_binding_table_matches_header(L):
    assert sorted(L.ABI_SYMBOLS) == declared_functions()


def test_point_layout_is_the_reference_lidarpoint(L):
    # slam_lib/include/LidarSlam/LidarPoint.h:31-64: float[4] @0, double time @16, float intensity @24,
    # u16 laser_id @28, u8 device_id @30, u8 label @31
    d = L.POINT_DTYPE
    assert d.itemsize == 32
    assert [d.fields[n][1] for n in ("x", "y", "z", "w", "time", "intensity", "laser_id", "device_id", "label")] == [0, 4, 8, 12, 16, 24, 28, 30, 31]


def test_param_struct_sizes(L):
    assert C.sizeof(L.ExtractParams) == 36
    assert C.sizeof(L.MatchParams) == 64
    p = L.ExtractParams()
    assert (p.neighbor_width, p.min_distance_to_sensor, p.edge_intensity_gap_threshold) == (4, 1.5, 50.0)
    m = L.MatchParams.ego_motion()
    assert (m.single_edge_per_ring, m.edge_nb_neighbors, m.edge_min_nb_neighbors, m.plane_nb_neighbors) == (1, 8, 3, 5)
    m = L.MatchParams.localization()
    assert (m.single_edge_per_ring, m.edge_nb_neighbors, m.edge_min_nb_neighbors) == (0, 10, 4)


def test_no_cpu_fallback(L):
    """Without a HIP device the product must refuse to run (no silent CPU path)."""
    lib = L.lib()
    if lib.lsa_device_count() > 0:
        return  # on a GPU box this property is exercised by the gpu tests actually running
    h = C.c_void_p()
    assert lib.lsa_ctx_create(0, C.byref(h)) == -1  # LSA_E_NO_DEVICE
    assert not h.value
    s = C.c_void_p()
    assert lib.lsa_slam_create(0, C.byref(s)) == -1
    try:
        L.Slam(0)
    except L.LsaError as e:
        assert "no CPU fallback" in str(e) or "no usable HIP device" in str(e)
    else:
        raise AssertionError("Slam() must raise without a GPU")


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "lidarslam_amd")
    for base, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".h", ".hip")):
                txt = open(os.path.join(base, f), errors="ignore").read()
                assert "oracle/" not in txt.replace("oracle/`` is test", "").replace("under ``oracle/``", "") or f == "__init__.py", f
                assert "import oracle" not in txt and "from oracle" not in txt, f
                assert "orc_" not in txt, f


def test_synthetic_generator_is_deterministic(L):
    a, sa = L.synth_frame(8, 1000, 2)
    b, sb = L.synth_frame(8, 1000, 2)
    c, _ = L.synth_frame(8, 1001, 2)
    assert a.tobytes() == b.tobytes() and sa == sb == 300000
    assert a.tobytes() != c.tobytes()
    # firing order: rings interleaved inside a column, time offsets in [-0.1, 0)
    assert a["time"].min() >= -0.1 and a["time"].max() < 0 and np.all(np.diff(a["time"]) >= 0)
    assert set(np.unique(a["laser_id"])) <= set(range(8))
    T = L.synth_pose(10)
    assert abs(T[0, 3] - 5.0) < 0.01 and np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3))


# ---- the signature table against the header's prototypes

C_KINDS = {
    "int": "int", "int32_t": "int", "unsigned": "unsigned", "unsigned int": "unsigned", "uint32_t": "unsigned", "float": "float",
    "double": "double", "uint64_t": "u64", "unsigned long long": "u64", "long long": "long long", "size_t": "size_t", "void": "void",
}


def c_kind(decl, named):
    """The kind of a C parameter (named) or result type; None for a type this classifier does not know."""
    if "*" in decl or "[" in decl or "(" in decl:
        return "pointer"
    words = [w for w in decl.split() if w != "const"]
    if named:
        words = words[:-1]
    return C_KINDS.get(" ".join(words))


def split_parameters(text):
    out, depth, cur = [], 0, ""
    for ch in text:
        depth += ch == "("
        depth -= ch == ")"
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    return out + [cur.strip()]


def header_prototypes():
    """name -> (kind of the result, [kind of each parameter]) of every function include/lidarslam_amd.h declares"""
    src = open(os.path.join(ROOT, "include", "lidarslam_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    src = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*$", "", src, flags=re.M)
    src = re.sub(r'extern\s+"C"\s*\{', "", src)
    while re.search(r"\{[^{}]*\}", src):
        src = re.sub(r"\{[^{}]*\}", "", src)  # struct and enum bodies
    out = {}
    for stmt in src.split(";"):
        stmt = " ".join(stmt.split())
        if "(" not in stmt or stmt.startswith("typedef"):
            continue
        m = re.match(r"^(.*?)\b(lsa_\w+) ?\((.*)\)$", stmt)
        assert m, f"not a prototype: {stmt!r}"
        result, name, params = m.group(1).strip(), m.group(2), m.group(3).strip()
        assert name not in out, f"{name} is declared twice"
        out[name] = (c_kind(result, False), [] if params == "void" else [c_kind(p, True) for p in split_parameters(params)], stmt)
    return out


def ctypes_kinds(t):
    """The kinds of C type a ctypes type (or None as a restype) passes for; empty for one this classifier does not know."""
    if t is None:
        return {"void"}
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, (C._Pointer, C._CFuncPtr)):
        return {"pointer"}
    kinds = set()
    for kind, types in (("int", [C.c_int]), ("unsigned", [C.c_uint]), ("float", [C.c_float]), ("double", [C.c_double]),
                        ("u64", [C.c_uint64, C.c_ulonglong]), ("long long", [C.c_longlong, C.c_int64]), ("size_t", [C.c_size_t])):
        if t in types:
            kinds.add(kind)
    return kinds


def signature_mismatches(table, protos):
    """One line per function whose table entry is not the header's prototype; each begins with the function's name."""
    bad = [f"{n}: in the table, not in the header" for n in table if n not in protos]
    for name, (result, params, stmt) in protos.items():
        if name not in table:
            bad.append(f"{name}: in the header, not in the table")
            continue
        restype, argtypes = table[name]
        if result is None or None in params:
            bad.append(f"{name}: a C type the classifier does not know in {stmt!r}")
        elif result == "void" and restype is not None or result != "void" and result not in ctypes_kinds(restype):
            bad.append(f"{name}: returns {result}, the table says {restype}")
        elif len(argtypes) != len(params):
            bad.append(f"{name}: {len(params)} parameters, the table has {len(argtypes)}")
        else:
            bad += [f"{name}: parameter {i} is {k}, the table says {t}" for i, (k, t) in enumerate(zip(params, argtypes)) if t is None or k not in ctypes_kinds(t)]
    return bad


def test_signature_table_is_the_headers_prototypes(L):
    protos = header_prototypes()
    assert sorted(protos) == declared_functions() == sorted(L.SIGNATURES) and len(protos) > 50
    assert signature_mismatches(L.SIGNATURES, protos) == []


def test_signature_check_reports_doctored_entries(L):
    protos = header_prototypes()
    table = copy.deepcopy(dict(L.SIGNATURES))

    def doctor(name, edit):
        restype, argtypes = table[name]
        table[name] = edit(restype, list(argtypes))

    def swapped(r, a):
        i, d = a.index(C.c_int), a.index(C.c_double)
        a[i], a[d] = a[d], a[i]
        return r, a

    doctor("lsa_pgo_assemble_priors", lambda r, a: (r, a[:-1]))  # one parameter dropped
    doctor("lsa_place_select_host", swapped)  # an int and a double swapped
    doctor("lsa_download_target", lambda r, a: (r, a[:3] + [C.c_int] + a[4:]))  # a pointer made c_int
    doctor("lsa_ctx_destroy", lambda r, a: (C.c_int, a))  # a void result left at c_int
    reported = {line.split(":")[0] for line in signature_mismatches(table, protos)}
    assert reported == {"lsa_pgo_assemble_priors", "lsa_place_select_host", "lsa_download_target", "lsa_ctx_destroy"}


def test_signatures_are_assigned_in_one_file_only():
    stray = []
    for path in sorted(glob.glob(os.path.join(ROOT, "lidarslam_amd", "*.py"))):
        if os.path.basename(path) != "_abi.py":
            stray += [f"{os.path.basename(path)}:{i + 1}" for i, line in enumerate(open(path)) if re.search(r"\.(argtypes|restype)\s*=", line)]
    assert not stray, f"signature assignments outside lidarslam_amd/_abi.py: {stray}"


# ---- the struct mirrors against the compiler's layout of the header's structs


def mirrored_structs(L):
    """header struct -> (size, {field: (offset, size)}) as ctypes and numpy lay the front end's mirrors out"""
    structures = {
        "lsa_extract_params_t": L.ExtractParams, "lsa_match_params_t": L.MatchParams, "lsa_kernel_stat_t": L.KernelStat,
        "lsa_icp_link_t": L.IcpLink, "lsa_solve_result_t": L.SolveResult, "lsa_sensor_terms_t": L.SensorTerms,
        "lsa_loop_closure_params_t": L.LoopClosureParams, "lsa_loop_closure_result_t": L.LoopClosureResultStruct,
        "lsa_place_params_t": L.PlaceParams, "lsa_place_search_t": L.PlaceSearch, "lsa_place_candidate_t": L.PlaceCandidateStruct,
        "lsa_pgo_params_t": L.PoseGraphParams, "lsa_pgo_result_t": L.PoseGraphResultStruct,
    }
    dtypes = {"lsa_point_t": L.POINT_DTYPE, "lsa_pgo_edge_t": L.PGO_EDGE_DTYPE, "lsa_pgo_prior_t": L.PGO_PRIOR_DTYPE}
    out = {c: (C.sizeof(s), {f[0]: (getattr(s, f[0]).offset, getattr(s, f[0]).size) for f in s._fields_}) for c, s in structures.items()}
    out.update({c: (d.itemsize, {f: (d.fields[f][1], d.fields[f][0].itemsize) for f in d.names}) for c, d in dtypes.items()})
    # the callers of lsa_upload_wire_frame / lsa_upload_robosense_frame build the layout as c_int32 * 7, in this order
    wire = ["point_step", "off_x", "off_y", "off_z", "off_intensity", "off_ring", "off_time"]
    out["lsa_wire_layout_t"] = (C.sizeof(C.c_int32 * 7), {f: (i * C.sizeof(C.c_int32), C.sizeof(C.c_int32)) for i, f in enumerate(wire)})
    return out


def test_struct_mirrors_have_the_compilers_layout(tmp_path, L):
    if shutil.which("g++") is None:
        pytest.skip("no g++ to lay the header's structs out")
    mirrors = mirrored_structs(L)
    assert len(mirrors) == 17
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "lidarslam_amd.h"', "int main()", "{"]
    for c, (_, fields) in mirrors.items():
        lines.append(f'  std::printf("{c} . 0 %zu\\n", sizeof({c}));')
        lines += [f'  std::printf("{c} {f} %zu %zu\\n", offsetof({c}, {f}), sizeof((({c}*)0)->{f}));' for f in fields]
    lines += ["  return 0;", "}", ""]
    (tmp_path / "layout.cpp").write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-invalid-offsetof", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "layout.cpp"), "-o", exe])
    compiled = {}
    for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines():
        c, f, offset, size = line.split()
        compiled.setdefault(c, [0, {}])
        if f == ".":
            compiled[c][0] = int(size)
        else:
            compiled[c][1][f] = (int(offset), int(size))
    for c, (size, fields) in mirrors.items():
        assert (size, fields) == tuple(compiled[c]), c


# ---- what `import lidarslam_amd` exposes


def test_frontend_surface_is_the_recorded_one(L):
    """tests/golden/frontend_surface.json (make_frontend_surface.py): every recorded name still resolves, the functions and the
    members of Context, Slam, RollingGrid, DeviceGrid and Sensors have the recorded signatures, and no member left or arrived."""
    golden = os.path.join(ROOT, "tests", "golden")
    spec = importlib.util.spec_from_file_location("make_frontend_surface", os.path.join(golden, "make_frontend_surface.py"))
    recorder = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(recorder)
    with open(os.path.join(golden, "frontend_surface.json")) as f:
        recorded = json.load(f)
    now = recorder.surface(L)
    assert len(recorded["names"]) > 80 and len(recorded["functions"]) > 30 and sorted(recorded["classes"]) == sorted(recorder.CLASSES)
    assert not set(recorded["names"]) - set(now["names"])
    assert {n: now["functions"].get(n) for n in recorded["functions"]} == recorded["functions"]
    assert now["classes"] == recorded["classes"]
