"""The host statement of place recognition against the maps (L.map_descriptor, L.map_place_select:
lidarslam_amd/csrc/host/lsa_place.cpp over lsa_scan_descriptor.h): the descriptor of a map as seen from a viewpoint against
L.scan_descriptor of points translated here in numpy by the rule, the selection against brute force, the recognition on the
oracle's maps that DESIGN.md 3.12 reports, the statement under the sanitizers in a stand-alone program, and the example.
No device."""
import ctypes as C
import math
import os
import platform
import shutil
import subprocess

import numpy as np
import pytest

from test_cpp_api import build_example

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# rings, sectors, the other parameters
SHAPES = [
    (1, 1, {}),
    (3, 7, dict(min_range=2.5, max_range=50.0, height_offset=1.25)),
    (20, 60, {}),
    (32, 120, dict(height_offset=-1.0)),
]


def translated(xyz, v):
    """the rule: x = float32(float64(p.x) - v.x), likewise y and z"""
    return (np.asarray(xyz, np.float32).astype(np.float64) - np.asarray(v, np.float64)).astype(np.float32)


def cloud_around(rng, v, n):
    """n points as a map holds them (float32) around the viewpoint: radii up to 99 m, a good part beyond max_range"""
    v = np.asarray(v, np.float64)
    return (v + np.column_stack([rng.uniform(-70, 70, n), rng.uniform(-70, 70, n), rng.uniform(-4, 6, n)])).astype(np.float32)


@pytest.mark.parametrize("rings,sectors,extra", SHAPES)
def test_map_descriptor_is_the_frame_descriptor_of_the_translated_points(L, rings, sectors, extra):
    rng = np.random.default_rng(20261020 + rings)
    p = dict(rings=rings, sectors=sectors, **extra)
    occupied = 0
    for v in ([0.0, 0.0, 0.0], [12.5, -7.25, 0.5], [0.1, 0.2, -0.3], [1e5, -1e5, 30.0], [-99999.9, 0.3, 1e5]):
        xyz = cloud_around(rng, v, 1500)
        xyz[0::50, 0] = np.nan
        xyz[1::50, 1] = np.nan
        xyz[2::50, 2] = np.nan
        got = L.map_descriptor(xyz, v, **p)
        want = L.scan_descriptor(translated(xyz, v), **p)
        assert got.dtype == np.float32 and got.size == rings * sectors + sectors
        assert got.tobytes() == want.tobytes(), (rings, sectors, v)
        occupied += int((got > 0).sum())
        # the order is irrelevant: a cell holds a maximum
        assert L.map_descriptor(xyz[rng.permutation(xyz.shape[0])], v, **p).tobytes() == got.tobytes()
        # a POINT_DTYPE array is taken as it is
        pts = np.zeros(xyz.shape[0], L.POINT_DTYPE)
        pts["x"], pts["y"], pts["z"], pts["intensity"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], 7.0
        assert L.map_descriptor(pts, v, **p).tobytes() == got.tobytes()
        # a viewpoint out of reach of everything: all zero; so are no points and nothing but NaNs
        away = np.asarray(v, np.float64) + [1e4, 0.0, 0.0]
        assert not L.map_descriptor(xyz, away, **p).any()
        assert not L.map_descriptor(np.zeros((0, 3), np.float32), v, **p).any()
        assert not L.map_descriptor(np.full((5, 3), np.nan, np.float32), v, **p).any()
    assert occupied > 0
    # 1e5 m from the origin a float32 coordinate has 1/128 m to give; the difference is formed in double and rounded to
    # float32 once, so what the descriptor sees is within half a unit in the last place of the exact frame coordinate
    v = np.array([1e5, -1e5, 30.0])
    xyz = cloud_around(rng, v, 200)
    exact = xyz.astype(np.float64) - v
    assert np.all(np.abs(translated(xyz, v).astype(np.float64) - exact) <= np.abs(exact) * 2.0 ** -24)


def test_map_descriptor_known_cell_and_refusals(L):
    p = dict(rings=20, sectors=60, min_range=1.5, max_range=61.5, height_offset=2.0)
    # seen from (100, 200, 10): r = 24 m at 100 degrees and 1.5 m above the viewpoint: ring 7, sector 46 (test_place_host.py)
    a = np.deg2rad(100.0)
    d = L.map_descriptor(np.array([[100.0 + 24.0 * np.cos(a), 200.0 + 24.0 * np.sin(a), 11.5]], np.float32), [100.0, 200.0, 10.0], **p)
    cells = d[:1200].reshape(20, 60)
    assert cells[7, 46] == 3.5 and np.count_nonzero(cells) == 1 and d[1200 + 46] == 3.5
    xyz = np.zeros((1, 3), np.float32)
    for bad in (dict(rings=0), dict(sectors=121), dict(type_mask=0), dict(max_range=0.0), dict(height_offset=float("nan"))):
        with pytest.raises(L.LsaError) as e:
            L.map_descriptor(xyz, [0, 0, 0], **bad)
        assert e.value.code == L.E_ARG, bad
    for v in ([np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [0, 0]):
        with pytest.raises(L.LsaError) as e:
            L.map_descriptor(xyz, v)
        assert e.value.code == L.E_ARG, v


# ---- the selection against brute force ---------------------------------------------------------------------------------------
def brute_select(distance, shift, vp, sectors, gate, radius, near, max_distance, capacity):
    ok = []
    for i in range(len(distance)):
        if np.isnan(distance[i]):
            continue
        if gate > 0 and not (float(distance[i]) <= gate):
            continue
        if max_distance > 0 and not (math.sqrt(float(((vp[i] - near) ** 2).sum())) <= max_distance):
            continue
        ok.append(i)
    ok.sort(key=lambda i: (distance[i], i))
    out = []
    while ok and len(out) < capacity:
        i = ok.pop(0)
        yaw = shift[i] * 2 * math.pi / sectors
        yaw = yaw - 2 * math.pi if yaw > math.pi else yaw
        out.append((i, distance[i], int(shift[i]), yaw))
        if radius > 0:
            ok = [j for j in ok if not (math.sqrt(float(((vp[j] - vp[i]) ** 2).sum())) <= radius)]
    return out


def test_select_follows_brute_force(L):
    rng = np.random.default_rng(11)
    n = 60
    a = np.linspace(0, 2 * np.pi, n)
    vp = np.column_stack([20 * np.sin(a), 20 * (1 - np.cos(a)), rng.normal(0, 0.05, n)])  # a loop: the ends lie next to each other
    vp[41] = vp[40]                                                                        # two viewpoints at one position
    distance = rng.uniform(0.05, 0.9, n).astype(np.float32)
    distance[[3, 4, 10, 11, 12, 40, 41]] = np.float32(0.05)  # ties on distance: the lower index, and the radius around it
    distance[[0, 58]] = np.float32(0.01)                      # the best at both ends of the loop, 2.1 m apart
    distance[25] = np.nan
    shift = rng.integers(0, 60, n).astype(np.int32)
    cases = 0
    for gate in (0.0, 0.05, 0.3):
        for radius in (0.0, -1.0, 1.0, 2.5, 6.0, 100.0):
            for near, max_distance in (((0, 0, 0), 0.0), ((0, 0, 0), 8.0), ((0.0, 40.0, 0.0), 10.0), ((500.0, 0, 0), 1.0)):
                for capacity in (0, 1, 4, 100):
                    got = L.map_place_select(distance, shift, vp, capacity=capacity, max_descriptor_distance=gate, exclusion_radius=radius, near_xyz=near,
                                             max_distance=max_distance)
                    want = brute_select(distance, shift, vp, 60, gate, radius, np.array(near, np.float64), max_distance, capacity)
                    assert [c[:4] for c in got] == want, (gate, radius, near, max_distance, capacity, got, want)
                    for i, _, _, yaw, guess in got:
                        T = np.eye(4)
                        T[:2, :2] = [[math.cos(yaw), -math.sin(yaw)], [math.sin(yaw), math.cos(yaw)]]
                        T[:3, 3] = vp[i]
                        assert np.array_equal(guess, T)  # Translation(v) * Rz(yaw), to the bit
                    cases += len(want) > 0
    assert cases > 100
    # what the cases are meant to show, on the brute-force statement
    first = brute_select(distance, shift, vp, 60, 0.0, 2.5, np.zeros(3), 0.0, 5)
    assert [c[0] for c in first] == [0, 3, 10, 12, 40]  # 58 falls to 0's radius, 4 to 3's, 11 to 10's (12 is 4.2 m from 10), 41 to 40's
    assert [c[0] for c in brute_select(distance, shift, vp, 60, 0.0, 0.0, np.zeros(3), 0.0, 3)] == [0, 58, 3]
    assert all(c[0] != 25 for c in brute_select(distance, shift, vp, 60, 0.0, 0.0, np.zeros(3), 0.0, 100))
    # the yaw is wrapped to (-pi, pi]
    assert L.map_place_select([0.5], [30], [[0, 0, 0]], capacity=1)[0][3] == 30 * 2 * math.pi / 60
    assert L.map_place_select([0.5], [31], [[0, 0, 0]], capacity=1)[0][3] == 31 * 2 * math.pi / 60 - 2 * math.pi
    # refusals
    for bad in (dict(capacity=-1), dict(sectors=0), dict(sectors=121), dict(exclusion_radius=float("nan")), dict(max_descriptor_distance=float("inf")),
                dict(max_distance=float("nan")), dict(max_distance=1.0, near_xyz=(0.0, float("nan"), 0.0)), dict(rings=0)):
        with pytest.raises(L.LsaError) as e:
            L.map_place_select(distance, shift, vp, **bad)
        assert e.value.code == L.E_ARG, bad
    broken = vp.copy()
    broken[7, 1] = np.inf
    for args in ((distance, shift, broken), (distance[:-1], shift, vp), (distance[:0], shift[:0], vp[:0])):
        with pytest.raises(L.LsaError) as e:
            L.map_place_select(*args)
        assert e.value.code == L.E_ARG
    assert L.map_place_select(distance, shift, vp, max_distance=0.0, near_xyz=(0.0, float("nan"), 0.0), capacity=1)[0][0] == 0  # near_xyz is not read


def test_struct_mirrors_have_the_compilers_layout(tmp_path, L):
    if shutil.which("g++") is None:
        pytest.skip("no g++ to lay the header's structs out")
    mirrors = {"lsa_map_place_search_t": L.MapPlaceSearch, "lsa_map_place_candidate_t": L.MapPlaceCandidateStruct, "lsa_map_place_summary_t": L.MapPlaceSummaryStruct}
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "lidarslam_amd.h"', "int main()", "{"]
    for c, s in mirrors.items():
        lines.append(f'  std::printf("{c} . 0 %zu\\n", sizeof({c}));')
        lines += [f'  std::printf("{c} {f[0]} %zu %zu\\n", offsetof({c}, {f[0]}), sizeof((({c}*)0)->{f[0]}));' for f in s._fields_]
    lines += ["  return 0;", "}", ""]
    (tmp_path / "layout.cpp").write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-invalid-offsetof", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "layout.cpp"), "-o", exe])
    seen = 0
    for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines():
        c, f, offset, size = line.split()
        if f == ".":
            assert C.sizeof(mirrors[c]) == int(size), c
        else:
            assert (getattr(mirrors[c], f).offset, getattr(mirrors[c], f).size) == (int(offset), int(size)), (c, f)
        seen += 1
    assert seen == 3 + sum(len(s._fields_) for s in mirrors.values())
    d = L.MapPlaceSearch()
    assert (d.exclusion_radius, d.max_distance, d.max_descriptor_distance, d.descriptor.rings, d.descriptor.sectors) == (5.0, 0.0, 0.0, 20, 60)
    c = L.MapPlaceSearch.__new__(L.MapPlaceSearch)
    L.lib().lsa_map_place_search_init(C.byref(c))
    assert bytes(c) == bytes(d)


# ---- the recognition DESIGN.md 3.12 reports, on the oracle's maps -------------------------------------------------------------
MODEL, MAPPED = 16, 30


def turned(pts, quarter):
    """the cloud as the sensor sees it with the base turned by +90 degrees about z (exactly: x' = y, y' = -x)"""
    if not quarter:
        return pts
    out = pts.copy()
    out["x"], out["y"] = pts["y"], -pts["x"]
    return out


@pytest.fixture(scope="module")
def oracle_maps(L, O):
    """Slam(EgoMotion=3) of the oracle over frames 0..29 of seed 1000: its EDGE and PLANE maps and the 30 poses"""
    s = O.Slam(EgoMotion=3)
    poses = []
    for f in range(MAPPED):
        pts, stamp = L.synth_frame(MODEL, 1000, f)
        s.add_frame(pts, stamp, f)
        poses.append(s.world_transform().copy())
    return np.concatenate([s.map(L.EDGE), s.map(L.PLANE)]), np.array(poses)


def test_recognition_on_the_oracles_maps(L, O, oracle_maps):
    """Viewpoints at the 30 logged positions (0.5 m apart); queries the oracle extractor's keypoints of every frame of seed 1001
    -- another scan of the same places -- with the base turned by 0 and by 90 degrees.  The winner lies within 1.0 m of the
    query's logged position (0.59 m, one frame, was measured, plus most of a viewpoint spacing) and within one sector of the
    turn.  Measured over these 60 queries: the winner at most 0.897 m off (query 1 turned, viewpoint 0; 0.593 m otherwise)
    and at most 1 sector off; its distance 0.065..0.195, the largest distance of a table 0.23..0.35."""
    points, poses = oracle_maps
    assert points.size > 10000
    vp = poses[:, :3, 3].copy()
    assert 0.4 < np.linalg.norm(np.diff(vp, axis=0), axis=1).mean() < 0.6
    table = np.array([L.map_descriptor(points, v) for v in vp])
    ex = O.Extractor()
    worst_off, worst_sectors, winners = 0.0, 0, []
    for quarter in (0, 1):
        for q in range(MAPPED):
            ex.compute(turned(L.synth_frame(MODEL, 1001, q)[0], quarter))
            query = L.scan_descriptor(np.concatenate([ex.keypoints(L.EDGE), ex.keypoints(L.PLANE)]))
            pairs = [L.place_distance(query, d) for d in table]
            (w, distance, shift, yaw, guess), = L.map_place_select([d for d, _ in pairs], [s for _, s in pairs], vp, capacity=1)
            off = float(np.linalg.norm(vp[w] - vp[q]))
            sectors_off = min((shift - 15 * quarter) % 60, (15 * quarter - shift) % 60)
            winners.append((quarter, q, w, round(off, 3), shift, float(distance), float(max(d for d, _ in pairs))))
            worst_off, worst_sectors = max(worst_off, off), max(worst_sectors, sectors_off)
            assert np.array_equal(guess[:3, 3], vp[w])
    print("winners (turn, query, viewpoint, metres off, shift, distance, largest distance):")
    for w in winners:
        print("  ", w)
    print("worst:", worst_off, "m,", worst_sectors, "sectors")
    assert worst_off <= 1.0 and worst_sectors <= 1


# ---- the statement under the sanitizers, in a program of its own; the example --------------------------------------------------
def test_the_host_statement_is_clean_under_sanitizers(tmp_path):
    exe = str(tmp_path / "drv")
    host = os.path.join(ROOT, "lidarslam_amd", "csrc", "host")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off"] + flags + ["-I" + host, os.path.join(ROOT, "tests", "map_place_sanitize.cpp"),
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


def test_the_example_compiles_links_and_refuses_to_run_without_a_gpu(tmp_path, L):
    exe = build_example(tmp_path, "slam_relocalization")
    if L.lib().lsa_device_count() == 0:
        r = subprocess.run([exe, str(tmp_path / "maps_")], capture_output=True, text=True)
        assert r.returncode == 1 and "no usable HIP device" in r.stderr
