"""The definition of the dense map's normals (DenseMapHost.normals, lidarslam_amd/_dense_map.py) on the cases of
tests/dense_normals_cases.py, with the oracle's eigen33 as the eigen step -- the one tests/test_gpu_numerics.py holds equal to
the device template bit for bit.  No GPU."""
import os
import platform
import shutil
import subprocess

import numpy as np
import pytest

import dense_normals_cases as N
from numerics_cases import C_LAM, C_ROOT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eig(O):
    return lambda cov: O.numerics(3, cov)


def normals(h, eig, **q):
    return h.normals(eig=eig, **q)


def unit_z(n):
    return (n["normal_x"] == 0).all() and (n["normal_y"] == 0).all() and (np.abs(n["normal_z"]) == 1).all()


# ---- 1. exact scenes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,full,counts", [(1, 9, {4, 6, 9}), (2, 25, {9, 12, 15, 16, 20, 25})])
def test_a_full_plane_has_exactly_its_axis_as_normal_and_no_curvature(L, eig, r, full, counts):
    h, _ = N.host_case("plane")
    n = normals(h, eig, radius_leaves=r)
    assert n.dtype == L.dense_normal_dtype and n.dtype.itemsize == 20 and len(n) == 81
    idx = N.indices_of(h.get()[1])
    assert (n["neighbors"] == N.brute_force_neighbors(idx, r)).all() and set(n["neighbors"].tolist()) == counts
    inner = (np.abs(idx[:, :2]) <= 4 - r).all(axis=1)
    assert (n["neighbors"][inner] == full).all() and inner.sum() == (9 - 2 * r) ** 2
    nan = N.no_normal(n)
    assert (nan == (n["neighbors"] < 5)).all() and nan.sum() == (4 if r == 1 else 0)  # the corners at r = 1 see 4 voxels
    assert unit_z(n[~nan]) and (n["curvature"][~nan] == 0).all() and not np.signbit(n["curvature"][~nan]).any()


def test_a_collinear_row_is_finite_or_the_nan_never_garbage(eig):
    h, queries = N.host_case("row")
    for q in queries:
        n = normals(h, eig, **q)
        r = q["radius_leaves"]
        assert (n["neighbors"] == N.brute_force_neighbors(N.indices_of(h.get()[1]), r)).all() and n["neighbors"].max() == 2 * r + 1
        nan = N.no_normal(n)  # (asserts: all four floats or none, and no other NaN)
        assert (nan[n["neighbors"] < 3]).all()
        fit = n[~nan]
        # a normal of a row along x is a unit vector across it, and a line has no surface variation
        length = np.sqrt(fit["normal_x"].astype(np.float64) ** 2 + fit["normal_y"].astype(np.float64) ** 2 + fit["normal_z"].astype(np.float64) ** 2)
        assert (np.abs(length - 1) < 1e-6).all() and (np.abs(fit["normal_x"]) < 1e-6).all() and (fit["curvature"] == 0).all()


def test_too_few_neighbours_give_the_quiet_nan(eig):
    h, queries = N.host_case("lone")
    for q in queries:
        n = normals(h, eig, **q)
        assert len(n) == 1 and n["neighbors"][0] == 1 and (N.float_bits(n) == 0x7FC00000).all()
    h, _ = N.host_case("plus")
    centre = int(np.flatnonzero((N.indices_of(h.get()[1]) == 0).all(axis=1))[0])
    at4, at5, at6 = (normals(h, eig, radius_leaves=1, min_neighbors=m) for m in (4, 5, 6))
    assert at5["neighbors"][centre] == 5 and sorted(at5["neighbors"].tolist()) == [4, 4, 4, 4, 5]
    assert N.no_normal(at6).all()  # k = min_neighbors - 1 at the centre
    assert N.no_normal(at5).tolist() == [i != centre for i in range(5)] and unit_z(at5[centre:centre + 1])  # k = min_neighbors
    assert not N.no_normal(at4).any()


def test_full_blocks_find_every_cell(eig):
    h, _ = N.host_case("blocks")
    idx = N.indices_of(h.get()[1])
    for r, cells in ((1, 27), (2, 125)):
        n = normals(h, eig, radius_leaves=r, min_neighbors=cells)
        inner = (np.abs(idx) <= 3 - r).all(axis=1)
        assert (n["neighbors"] == N.brute_force_neighbors(idx, r)).all() and (n["neighbors"][inner] == cells).all()
        assert (N.no_normal(n) == ~inner).all() and (n["curvature"][inner] > 0.05).all()  # a filled block is no surface


# ---- 2. orientation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 2])
def test_the_viewpoint_decides_exactly_the_sign(eig, r):
    h, _ = N.host_case("oriented")
    sources = h.sources()
    assert sorted(set(sources.tolist())) == [0, 1, 2, 3]
    plain = normals(h, eig, radius_leaves=r)
    above, below, level = (normals(h, eig, radius_leaves=r, viewpoints=[v]) for v in (N.ABOVE, N.BELOW, N.LEVEL))
    fit = ~N.no_normal(plain)
    assert fit.sum() >= 77 and (above["normal_z"][fit] == 1).all() and (below["normal_z"][fit] == -1).all()
    for a in N.FLOATS[:2]:  # a zero is negated too: the two differ in the sign bit of every component
        assert (np.signbit(above[a][fit]) != np.signbit(below[a][fit])).all() and (above[a][fit] == 0).all()
    assert (above["curvature"] == below["curvature"])[fit].all() and (above["neighbors"] == plain["neighbors"]).all()
    assert level.tobytes() == plain.tobytes()  # dot == 0 keeps eigen33's own sign
    # entries for the ordinals 1 and 2: source 0 is clamped to the first, source 3 to the last
    clamped = normals(h, eig, radius_leaves=r, viewpoints=[N.ABOVE, N.BELOW], first_frame=1)
    assert (clamped["normal_z"][fit] == np.where(sources <= 1, 1.0, -1.0)[fit]).all()
    other = normals(h, eig, radius_leaves=r, viewpoints=[N.BELOW, N.ABOVE], first_frame=1)
    assert (other["normal_z"][fit] == -clamped["normal_z"][fit]).all()
    assert normals(h, eig, radius_leaves=r, viewpoints=np.zeros((0, 3), np.float32)).tobytes() == plain.tobytes()


# ---- 3. against numpy.linalg.eigh on the statement's own covariances ---------------------------------------------------------
@pytest.mark.parametrize("r", [1, 2])
def test_normals_of_a_noisy_oblique_plane_against_eigh(L, eig, r):
    """Gate: (l1 - l0) >= 0.05 * l2.  Bound: |sin(angle)| <= 4 * 2^-24 + (C_LAM u S + C_ROOT u S min(S / gap, u^-1/2)) / gap, the
    eigenvector bound of tests/numerics_cases.py plus the narrowing of three components to float.  The gate may leave out at
    most 5 % of the fitted voxels."""
    h = L.DenseMapHost(N.OBLIQUE_LEAF)
    h.insert(N.oblique_plane(), 0)
    assert h.skipped == 0 and h.size() > 2000
    pts, vox = h.get()
    n = normals(h, eig, radius_leaves=r)
    k, s, S = L.dense_normal_sums(pts, vox["key"], r)
    assert (n["neighbors"] == k).all()
    fit = ~N.no_normal(n)
    assert (fit == (k >= 5)).all() and fit.sum() > 0.98 * len(n)
    cov = L.dense_normal_covariances(k[fit], s[fit], S[fit])
    E = L.eigh_eig(cov)
    lam, ref = E[:, :3], E[:, 3:6]
    gap, size = lam[:, 1] - lam[:, 0], lam[:, 2]
    gated = gap >= 0.05 * size
    share = 1.0 - gated.sum() / fit.sum()
    print(f"r = {r}: {fit.sum()} fitted voxels, the gate leaves out {100 * share:.3f} %")
    assert share <= 0.05
    u = 2.0**-53
    bound = 4 * 2.0**-24 + (C_LAM * u * size + C_ROOT * u * size * np.minimum(size / gap, u**-0.5)) / gap
    got = np.stack([n[a][fit].astype(np.float64) for a in N.FLOATS[:3]], axis=1)
    sin = np.linalg.norm(np.cross(got, ref), axis=1)
    print(f"largest |sin| over its bound: {np.max(sin[gated] / bound[gated]):.3g}")
    assert (sin[gated] <= bound[gated]).all()
    # and the fallback without an eigen step is that eigh, up to sign
    loose = h.normals(radius_leaves=r)
    lo = np.stack([loose[a][fit].astype(np.float64) for a in N.FLOATS[:3]], axis=1)
    assert (np.linalg.norm(np.cross(lo, ref), axis=1) <= 4 * 2.0**-24).all() and (loose["neighbors"] == k).all()
    # curvature is the surface variation of those eigenvalues
    assert np.allclose(n["curvature"][fit], np.abs(lam[:, 0] / lam.sum(axis=1)), rtol=1e-5, atol=1e-9)


# ---- 4. the predicate ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,filt", [("low_frames", dict(min_frames=2)), ("seen_through", dict(max_miss_ratio=1.0))])
def test_what_the_export_leaves_out_does_not_bend_the_wall(L, eig, name, filt):
    leaf, steps, _, _ = N.CASES[name]()
    h = N.play(L.DenseMapHost(leaf), steps)
    bare = N.play(L.DenseMapHost(leaf), N.CASES[name](with_cluster=False)[1])
    assert h.size() == len(N.WALL) + len(N.CLUSTER) and bare.size() == len(N.WALL) == len(h.get(**filt)[1])
    for r in (1, 2):
        q = dict(radius_leaves=r, min_neighbors=4)  # (a corner of the wall sees 4 voxels at r = 1)
        filtered, never, everything = normals(h, eig, **q, **filt), normals(bare, eig, **q, **filt), normals(h, eig, **q)
        assert filtered.tobytes() == never.tobytes() and not N.no_normal(filtered).any()
        wall = np.isin(h.get()[1]["key"], bare.get()[1]["key"])
        assert wall.sum() == len(N.WALL) and everything[wall].tobytes() != filtered.tobytes()
        assert (everything["neighbors"][wall] > filtered["neighbors"]).sum() >= 9


# ---- 5. the index edge --------------------------------------------------------------------------------------------------------
def test_cells_past_the_index_range_are_skipped_not_wrapped(eig):
    h, queries = N.host_case("index_edge")
    idx = N.indices_of(h.get()[1])
    assert idx.min() == N.LO and idx.max() == N.HI and len(idx) == 6 * 18 - 0
    for q in queries:
        n = normals(h, eig, **q)
        assert (n["neighbors"] == N.brute_force_neighbors(idx, q["radius_leaves"])).all() and n["neighbors"].max() == 18
        assert not N.no_normal(n).any()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(eig):
    h, _ = N.host_case("plane")
    before = (h.get()[0].tobytes(), h.get()[1].tobytes())
    for bad in (dict(radius_leaves=0), dict(radius_leaves=3), dict(min_neighbors=2), dict(radius_leaves=1, min_neighbors=28), dict(min_neighbors=126),
                dict(min_frames=0), dict(viewpoints=[0.0, 0.0, 1.0]), dict(viewpoints=np.zeros((2, 4), np.float32))):
        with pytest.raises(ValueError):
            normals(h, eig, **bad)
    normals(h, eig, radius_leaves=1, min_neighbors=27), normals(h, eig, min_neighbors=125)
    assert (h.get()[0].tobytes(), h.get()[1].tobytes()) == before


# ---- the file's host code ------------------------------------------------------------------------------------------------------
def test_the_pcd_writer_and_the_normals_reader_are_clean_under_sanitizers(tmp_path):
    """the generalised writer and lsa_pcd_read_normals in a stand-alone program with its own main (tests/pcd_normals_sanitize.cpp),
    built for the CPU with Address + UB sanitizer: the three formats, a truncated data section, a header lacking one normal
    field.  Nothing loaded into Python runs under a sanitizer."""
    exe = str(tmp_path / "drv")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__"] + flags + [
        os.path.join(ROOT, "tests", "pcd_normals_sanitize.cpp"), os.path.join(ROOT, "lidarslam_amd", "csrc", "host", "lsa_pcd.cpp"), "-o", exe]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-std=c++17"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this compiler has no runtime for -fsanitize=address,undefined")
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    # (as tests/test_lm_step_reference.py: the sanitizers' shadow layout wants the address space unrandomized)
    norand = ["setarch", platform.machine(), "-R"]
    if shutil.which("setarch") is None or subprocess.run(norand + ["true"], capture_output=True).returncode != 0:
        norand = []
    files = tmp_path / "files"
    files.mkdir()
    run = subprocess.run(norand + [exe, str(files)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.startswith("ok"), (run.stdout[-1500:], run.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr


def test_plain_files_read_back_and_the_normals_reader_refuses_them(L, tmp_path):
    """through the library itself, no GPU (files WITH normals are written by the device map's calls alone: the sanitizer driver
    above and tests/test_gpu_dense_normals.py read those back): a plain file reads back as before, and read_pcd_normals
    refuses it and names the file and the field"""
    pts = N.oblique_plane(500)
    assert (pts["w"] == 1.0).all()
    for fmt in (L.PCD_ASCII, L.PCD_BINARY, L.PCD_BINARY_COMPRESSED):
        path = str(tmp_path / f"plain{fmt}.pcd")
        assert L.write_pcd(path, pts, fmt)
        assert L.read_pcd(path).tobytes() == pts.tobytes()
        with pytest.raises(L.LsaError) as e:
            L.read_pcd_normals(path)
        assert path in str(e.value) and "normal_x" in str(e.value)


def test_the_record_dtype_has_the_compilers_layout_of_the_headers_struct(L, tmp_path):
    """dense_normal_dtype against lsa_dense_normal_t as g++ lays it out: size, and offset and size of every field, in order"""
    if shutil.which("g++") is None:
        pytest.skip("no g++ to lay the header's struct out")
    fields = ["nx", "ny", "nz", "curvature", "neighbors"]
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "lidarslam_amd.h"', "int main()", "{", '  std::printf("%zu\\n", sizeof(lsa_dense_normal_t));']
    lines += [f'  std::printf("%zu %zu\\n", offsetof(lsa_dense_normal_t, {f}), sizeof(((lsa_dense_normal_t*)0)->{f}));' for f in fields]
    lines += ["  return 0;", "}", ""]
    (tmp_path / "layout.cpp").write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "layout.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    d = L.dense_normal_dtype
    assert int(out[0]) == d.itemsize == 20 and list(d.names) == ["normal_x", "normal_y", "normal_z", "curvature", "neighbors"]
    compiled = [(int(out[1 + 2 * i]), int(out[2 + 2 * i])) for i in range(5)]
    assert compiled == [(d.fields[n][1], d.fields[n][0].itemsize) for n in d.names] == [(0, 4), (4, 4), (8, 4), (12, 4), (16, 4)]
    assert [d.fields[n][0].kind for n in d.names] == ["f", "f", "f", "f", "u"]
