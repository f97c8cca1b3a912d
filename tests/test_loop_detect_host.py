"""Loop detection over a whole log, the host statement (lsa_place_detect_host, lidarslam_amd/csrc/host/lsa_place.cpp): for
every query of a set what L.place_select returns from the table of L.place_distance -- checked against exactly that loop
written in Python, exactly; every refusal; and the statement with the shared gates (lsa_place_select.h) in a stand-alone
program under Address + UB sanitizer.  No device."""
import ctypes as C
import os
import platform
import shutil
import subprocess

import numpy as np
import pytest
from loop_detect_cases import SHAPES, TABLES, TRAJECTORIES, by_definition, descriptors, distance_table, grid, trajectory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGS = [1, 2, 3, 40]


@pytest.mark.parametrize("rings,sectors", SHAPES)
def test_detection_is_the_loop_over_distance_and_select(L, rings, sectors):
    seen = {"none": 0, "fewer": 0, "full": 0, "candidates": 0}
    for kind in TABLES:
        for n in LOGS:
            D = descriptors(kind, n, rings, sectors)
            table = distance_table(L, D, rings, sectors)
            for path in TRAJECTORIES:
                P, t = trajectory(path, n)
                for case in grid(n, 12 if n == 40 else 6):
                    if not (case["first_query"] <= (n - 1 if case["last_query"] < 0 else case["last_query"])):
                        continue
                    want, counts = by_definition(L, table, P, t, sectors, **case)
                    got = L.place_detect_host(D, P, t, rings=rings, sectors=sectors, **case)
                    assert got == want, (kind, n, path, case, got[:4], want[:4])
                    assert [g[0] for g in got] == sorted(g[0] for g in got)
                    seen["none"] += sum(c == 0 for c in counts)
                    seen["fewer"] += sum(0 < c < case["per_query"] for c in counts)
                    seen["full"] += sum(c == case["per_query"] for c in counts)
                    seen["candidates"] += len(got)
    # the cases together reach every kind of answer
    assert seen["none"] > 0 and seen["fewer"] > 0 and seen["full"] > 0 and seen["candidates"] > 1000, seen
    # every distance ties: the lowest admissible frames
    P, t = trajectory("forward_back", 40)
    got = L.place_detect_host(descriptors("identical", 40, rings, sectors), P, t, rings=rings, sectors=sectors, min_travelled=3.0, exclusion_half_window=2, per_query=3)
    assert [g[1] for g in got if g[0] == 39] == [0, 3, 6]


def test_refusals_write_nothing(L):
    n, rings, sectors = 6, 3, 7
    D = descriptors("random", n, rings, sectors)
    P, t = trajectory("forward_back", n)
    rows = np.ascontiguousarray(np.concatenate([P.reshape(-1, 16), t.reshape(-1, 1)], axis=1))
    lib = L.lib()

    def call(capacity=None, descriptors_=D, rows_=rows, n_=n, have_out=True, **fields):
        d = L.LoopDetect(rings=rings, sectors=sectors)
        for k, v in fields.items():
            target = d if k in ("first_query", "last_query", "query_stride", "per_query") else (d.search if hasattr(d.search, k) and k != "descriptor" else d.search.descriptor)
            setattr(target, k, v)
        out = (L.LoopCandidateStruct * 200)()
        C.memset(out, 0x5A, C.sizeof(out))
        before = bytes(out)
        rc = lib.lsa_place_detect_host(C.byref(d), None if descriptors_ is None else L.ptr(descriptors_), None if rows_ is None else L.ptr(rows_), n_,
                                       out if have_out else None, 200 if capacity is None else capacity)
        return rc, bytes(out) == before

    assert call()[0] >= 0
    bad = [
        dict(query_stride=0), dict(query_stride=-1), dict(first_query=-1), dict(first_query=4, last_query=3), dict(last_query=n), dict(first_query=n),
        dict(per_query=0), dict(per_query=17), dict(per_query=-1), dict(rings=0), dict(rings=33), dict(sectors=121), dict(type_mask=0), dict(max_range=-1.0),
        dict(min_travelled=-1.0), dict(min_travelled=float("nan")), dict(exclusion_half_window=-1), dict(max_distance=float("nan")),
        dict(max_descriptor_distance=float("nan")), dict(capacity=n - 1), dict(capacity=-1), dict(per_query=3, capacity=3 * n - 1), dict(n_=0), dict(n_=-1),
        dict(descriptors_=None), dict(rows_=None), dict(have_out=False),
    ]
    for case in bad:
        rc, untouched = call(**case)
        assert rc == L.E_ARG and untouched, case
    # capacity is held to queries * per_query, not to what is found: exactly enough is enough
    assert call(per_query=3, capacity=3 * n)[0] >= 0
    assert call(query_stride=4, per_query=2, capacity=4)[0] >= 0 and call(query_stride=4, per_query=2, capacity=3)[0] == L.E_ARG
    # the front end refuses what it cannot size, with the same code
    for case in [dict(query_stride=0), dict(first_query=3, last_query=2), dict(last_query=n), dict(per_query=17)]:
        with pytest.raises(L.LsaError) as e:
            L.place_detect_host(D, P, t, rings=rings, sectors=sectors, **case)
        assert e.value.code == L.E_ARG
    with pytest.raises(L.LsaError) as e:
        L.place_detect_host(D[:, :-1], P, t, rings=rings, sectors=sectors)
    assert e.value.code == L.E_ARG


def test_defaults_and_struct_layout(tmp_path, L):
    d = L.LoopDetect()
    lib_d = L.LoopDetect(first_query=9, last_query=9, query_stride=9, per_query=9, min_travelled=1.0)
    L.lib().lsa_loop_detect_init(C.byref(lib_d))
    assert bytes(d) == bytes(lib_d)
    assert (d.first_query, d.last_query, d.query_stride, d.per_query, d.search.min_travelled, d.search.exclusion_half_window) == (0, -1, 1, 1, 20.0, 5)
    if shutil.which("g++") is None:
        pytest.skip("no g++ to lay the header's structs out")
    mirrors = {"lsa_loop_detect_t": L.LoopDetect, "lsa_loop_candidate_t": L.LoopCandidateStruct, "lsa_loop_report_t": L.LoopReportStruct}
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "lidarslam_amd.h"', "int main()", "{"]
    want = []
    for c, s in mirrors.items():
        lines.append(f'  std::printf("{c} . 0 %zu\\n", sizeof({c}));')
        want.append(f"{c} . 0 {C.sizeof(s)}")
        for f, _ in s._fields_:
            lines.append(f'  std::printf("{c} {f} %zu %zu\\n", offsetof({c}, {f}), sizeof((({c}*)0)->{f}));')
            want.append(f"{c} {f} {getattr(s, f).offset} {getattr(s, f).size}")
    lines += ["  return 0;", "}", ""]
    (tmp_path / "layout.cpp").write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-invalid-offsetof", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "layout.cpp"), "-o", exe])
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines() == want


def test_the_host_statement_is_clean_under_sanitizers(tmp_path):
    exe = str(tmp_path / "drv")
    host = os.path.join(ROOT, "lidarslam_amd", "csrc", "host")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off"] + flags + ["-I" + host, os.path.join(ROOT, "tests", "loop_detect_sanitize.cpp"),
                                                                             os.path.join(host, "lsa_place.cpp"), "-o", exe]
    # whether this compiler has the sanitizers' runtime at all is decided on a program of one line; the build proper is then
    # asserted: an error in the driver or in the code under test is a failure, never a skip
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-std=c++17"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this compiler has no runtime for -fsanitize=address,undefined")
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    # the sanitizers' fixed shadow layout does not hold an executable placed by high-entropy ASLR: the driver runs with its
    # own address space unrandomized
    norand = ["setarch", platform.machine(), "-R"]
    if shutil.which("setarch") is None or subprocess.run(norand + ["true"], capture_output=True).returncode != 0:
        norand = []
    run = subprocess.run(norand + [exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.startswith("ok"), (run.stdout[-1500:], run.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr
