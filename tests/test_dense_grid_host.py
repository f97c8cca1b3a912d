"""The definition of the dense map's floor plan (DenseMapHost.grid, dense_grid): what each scene of tests/dense_grid_cases.py must
give, written out by hand; a window is the crop of the whole; the order of the points and a whole-cell translation change
nothing but the origin; the filter agrees with a pruned map; refusals; the files.  No GPU and no native library."""
import os
import platform
import shutil
import subprocess

import numpy as np
import pytest

import dense_grid_cases as G
from dense_map_cases import cloud
from lidarslam_amd import _dense_map as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = np.uint32(D.DENSE_GRID_ABSENT)


def grid_of(name, q=0):
    h, queries = G.host_case(name)
    return h.grid(**queries[q])


def record(cells, y, x):
    c = cells[y, x]
    f = [None if np.float32(c[k]).view(np.uint32) == NAN else float(c[k]) for k in G.FLOATS]
    return (f[0], f[1], f[2], int(c["floor_voxels"]), int(c["obstacle_voxels"]))


def test_a_wall_whose_foot_was_never_seen_is_occupied_by_the_neighbours_ground():
    info, cells, state = grid_of("wall")
    assert (int(info["cx0"]), int(info["cy0"]), int(info["width"]), int(info["height"])) == (0, 0, 6, 3)
    assert float(info["resolution"]) == 0.25 and float(info["origin_x"]) == 0.0 and float(info["origin_y"]) == 0.0
    assert state.dtype == np.int8 and state.tolist() == [[0, 0, 0, 100, 0, 0]] * 3
    for y in range(3):
        assert record(cells, y, 3) == (G.Z(2), G.Z(0), G.Z(5), 0, 4)
        assert record(cells, y, 2) == (G.Z(0), G.Z(0), None, 1, 0)
    # without a neighbourhood the wall stands on itself: its lowest voxel is its floor
    _, cells0, state0 = grid_of("wall", 1)
    assert state0.tolist() == state.tolist() and record(cells0, 1, 3) == (G.Z(2), G.Z(2), G.Z(5), 1, 3)


def test_a_pole_and_min_obstacle_voxels():
    _, cells, state = grid_of("pole")
    want = np.zeros((5, 5), int)
    want[2, 2] = want[0, 0] = 100
    assert state.tolist() == want.tolist()
    assert record(cells, 2, 2) == (G.Z(0), G.Z(0), G.Z(6), 1, 6) and record(cells, 0, 0) == (G.Z(0), G.Z(0), G.Z(2), 1, 1)
    _, cells2, state2 = grid_of("pole", 1)  # two obstacle voxels at least: the stub is free, its record is as it was
    want[0, 0] = 0
    assert state2.tolist() == want.tolist() and cells2.tobytes() == cells.tobytes()
    assert (grid_of("pole", 2)[2] == 0).all()  # seven: nothing is occupied, the floor was seen everywhere


def test_a_slab_above_max_height_is_free_over_seen_floor_and_unknown_over_unseen():
    info, cells, state = grid_of("slab")
    assert (int(info["width"]), int(info["height"])) == (10, 3)
    for y in range(3):
        assert state[y].tolist() == [0, -1, -1, -1, -1, -1, -1, -1, 0, 0]
        assert record(cells, y, 0) == (G.Z(0), G.Z(0), None, 1, 0)  # driven under
        assert record(cells, y, 1) == (G.Z(10), G.Z(0), None, 0, 0) and record(cells, y, 2) == record(cells, y, 1)  # a crown over unseen ground
        assert record(cells, y, 5) == (None, None, None, 0, 0)  # no column within two cells
        assert record(cells, y, 3) == record(cells, y, 6) == (None, G.Z(10), None, 0, 0)  # a ground from the neighbours, no column
        assert record(cells, y, 8) == (G.Z(10), G.Z(10), None, 1, 0)  # far from any floor the slab is its own ground
    # max_height is inclusive: at exactly 2.5 the slab is an obstacle, one double below it is not
    _, cells_in, state_in = grid_of("slab", 1)
    assert state_in[1].tolist() == [100, 100, 100, -1, -1, -1, -1, -1, 0, 0] and record(cells_in, 1, 1) == (G.Z(10), G.Z(0), G.Z(10), 0, 1)
    assert grid_of("slab", 2)[2].tobytes() == state.tobytes()


def test_a_kerb_of_exactly_min_height_is_floor_and_one_float_above_it_an_obstacle():
    for q in (0, 1):
        _, cells, state = grid_of("kerb", q)
        assert state.tolist() == [[0, 0, 100, 0]]
        assert record(cells, 0, 1) == (G.Z(0), G.Z(0), None, 2, 0)
        assert record(cells, 0, 2) == (G.Z(0), G.Z(0), G.KERB_UP, 1, 1)
    assert G.KERB_UP > G.Z(1) and np.float64(G.Z(1)) - np.float64(G.Z(0)) == G.KERB_MIN


def test_a_ramp_is_free_until_the_neighbourhood_is_wider_than_its_slope_allows():
    z = (np.float32(0.03125) + np.float32(G.RAMP_STEP) * np.arange(12, dtype=np.float32)).astype(np.float64)
    _, cells, state = grid_of("ramp")
    assert (state == 0).all() and cells["elevation"][0].tolist() == z.tolist()
    assert cells["ground"][0].tolist() == [z[max(i - 2, 0)] for i in range(12)]  # 0.125 below: floor
    _, cells4, state4 = grid_of("ramp", 1)  # radius 4: 0.25 below from cell 4 on
    assert state4[0].tolist() == [0] * 4 + [100] * 8 and cells4["ground"][0].tolist() == [z[max(i - 4, 0)] for i in range(12)]
    assert cells4["obstacle_voxels"][0].tolist() == [0] * 4 + [1] * 8 and cells4["top"][0, 4:].tolist() == z[4:].tolist()
    _, cells0, state0 = grid_of("ramp", 2)
    assert (state0 == 0).all() and cells0["ground"].tobytes() == cells0["elevation"].tobytes()


def test_a_car_the_miss_ratio_filters_out_leaves_its_cell_free():
    h, queries = G.host_case("car")
    assert h.misses().max() == 5 and (h.misses() > 0).sum() == 1
    info, cells, state = h.grid(**queries[0])
    assert (int(info["cx0"]), int(info["cy0"]), int(info["width"]), int(info["height"])) == (0, -1, 9, 3) and float(info["origin_y"]) == -0.25
    want = np.zeros((3, 9), int)
    want[1, 8] = 100
    assert state.tolist() == want.tolist() and record(cells, 1, 4) == (G.Z(0), G.Z(0), None, 1, 0)
    _, cells_all, state_all = h.grid(**queries[1])
    want[1, 4] = 100
    assert state_all.tolist() == want.tolist() and record(cells_all, 1, 4) == (G.Z(0), G.Z(0), G.Z(2), 1, 1)
    assert h.grid(**queries[2])[2].tobytes() == state.tobytes()  # seen in one frame alone: min_frames 2 leaves it out too


def test_cells_are_floor_divisions_on_both_sides_of_zero():
    h, queries = G.host_case("both_sides")
    # ix -4..3: cells of 3 hold [-4], [-3 -2 -1], [0 1 2], [3]; iy -1 is cell -1 and iy 0 is cell 0 whatever the cell's size
    want = {1: (-4, [[1] * 8] * 2), 2: (-2, [[2] * 4] * 2), 3: (-2, [[1, 3, 3, 1]] * 2)}
    for q in queries:
        c = q["cell_leaves"]
        info, cells, state = h.grid(**q)
        cx0, floor = want[c]
        assert (int(info["cy0"]), int(info["height"])) == (-1, 2)
        assert int(info["cx0"]) == cx0 and cells["floor_voxels"].tolist() == floor, c
        assert float(info["origin_x"]) == cx0 * c * 0.25 and float(info["resolution"]) == c * 0.25 and (state == 0).all()


def test_signed_zeros_rank_as_their_codes():
    _, cells, state = grid_of("signed_zero")
    assert cells.shape == (1, 1) and G.float_bits(cells)[0, 0].tolist() == [0x80000000, 0x80000000, int(NAN)]
    assert record(cells, 0, 0)[3:] == (2, 0) and state.tolist() == [[0]]
    _, cells, state = grid_of("signed_zero_top")
    assert G.float_bits(cells)[0, 0].tolist() == [np.float32(-1.0).view(np.uint32), np.float32(-1.0).view(np.uint32), 0]
    assert record(cells, 0, 0)[3:] == (1, 2) and state.tolist() == [[100]]


def test_ground_radius_0_15_and_16():
    h, queries = G.host_case("radius")
    assert h.grid(**queries[0])[2].tolist() == [[0] + [-1] * 15 + [100, 0]]  # 16 reaches cell 16, not cell 17
    assert h.grid(**queries[1])[2].tolist() == [[0] + [-1] * 15 + [0, 0]]
    _, cells, state = h.grid(**queries[2])  # 15: cell 16 takes cell 17's elevation -- its own -- and cell 1 has cell 0's ground
    assert state.tolist() == [[0] + [-1] * 15 + [0, 0]] and record(cells, 0, 15) == (None, G.Z(0), None, 0, 0) and record(cells, 0, 16)[1] == G.Z(4)


def test_shapes_of_the_one_cell_and_the_wide_grids():
    h, queries = G.host_case("one_cell")
    for q in queries:
        info, cells, state = h.grid(**q)
        c = q["cell_leaves"]
        assert cells.shape == (1, 1) and state.tolist() == [[0]] and (int(info["cx0"]), int(info["cy0"])) == (-3 // c, 5 // c)
    for n in G.WIDTHS:
        h, queries = G.host_case(f"wide{n}")
        info, cells, state = h.grid(**queries[0])
        assert cells.shape == (3, n) and int(info["cx0"]) == -(n // 2) and (state[1, ::7] == 100).all() and (state == 100).sum() == len(range(0, n, 7))


def test_an_empty_map_and_a_window_without_a_cell():
    h = D.DenseMapHost(0.25)
    info, cells, state = h.grid()
    assert cells.shape == state.shape == (0, 0) and info["width"] == info["height"] == 0 and float(info["resolution"]) == 0.5
    # a window is answered whatever the map holds
    info, cells, state = h.grid(window=(0.0, 0.0, 0.9, 0.4))
    assert cells.shape == (1, 2) and (state == -1).all() and (G.float_bits(cells) == NAN).all()
    edge = float(D.DENSE_INDEX_RANGE) * 0.25
    for w in ((edge, 0.0, edge + 5.0, 1.0), (0.0, -edge - 9.0, 1.0, -edge - 0.25)):
        info, cells, state = h.grid(window=w)
        assert cells.shape == (0, 0) and info["width"] == info["height"] == 0
    info, cells, _ = h.grid(cell_leaves=1, window=(edge - 0.25, -edge - 9.0, edge + 5.0, -edge))  # clamped to the last and the first index
    assert cells.shape == (1, 1) and (int(info["cx0"]), int(info["cy0"])) == (D.DENSE_INDEX_RANGE - 1, -D.DENSE_INDEX_RANGE)
    h.insert(G.at([[0, 0, 0]]), 0)
    assert h.grid(min_frames=2)[1].shape == (0, 0)  # no voxel that counts


def test_a_window_is_the_crop_of_the_whole():
    h, _ = G.host_case("scattered")
    for q in G.SCATTERED_QUERIES:
        around = h.grid(window=G.WINDOWS["around"], **q)
        whole = h.grid(**q)
        cells, state = G.crop(around, whole[0])
        assert whole[1].tobytes() == cells.tobytes() and whole[2].tobytes() == state.tobytes()
        assert q.get("cell_leaves", 2) > 3 or ((state == 100).sum() > 5 and (state == 0).sum() > 20 and (state == -1).sum() > 0)
        for name, w in G.WINDOWS.items():
            part = h.grid(window=w, **q)
            if name == "outside":
                assert (part[2] == -1).all() and part[1].size > 0
                continue
            cells, state = G.crop(around, part[0])
            assert part[1].tobytes() == cells.tobytes() and part[2].tobytes() == state.tobytes(), name
        assert h.grid(window=G.WINDOWS["point"], **q)[1].shape == (1, 1)


def test_the_order_of_the_points_changes_nothing():
    leaf, pts = G.scattered()
    rng = np.random.default_rng(1)
    a, b = D.DenseMapHost(leaf), D.DenseMapHost(leaf)
    a.insert(pts, 0)
    b.insert(pts[rng.permutation(len(pts))], 0)
    for q in G.SCATTERED_QUERIES:
        G.same_grid(a.grid(**q), b.grid(**q))
    # and dense_grid does not mind the order of the export it is given
    p, v = a.get()
    order = rng.permutation(len(v))
    G.same_grid(D.dense_grid(p[order], v["key"][order], leaf, cell_leaves=3), a.grid(cell_leaves=3))


def test_a_whole_cell_translation_shifts_the_grid_and_nothing_else():
    leaf, pts = G.scattered()
    for a in ("x", "y"):
        pts[a] = np.round(pts[a] * 1024) / 1024  # multiples of 2^-10 below 8: the sums below are exact
    for q in G.SCATTERED_QUERIES[:3]:
        c = q.get("cell_leaves", 2)
        moved = pts.copy()
        moved["x"] += np.float32(7 * c * leaf)
        moved["y"] -= np.float32(3 * c * leaf)
        a, b = D.DenseMapHost(leaf), D.DenseMapHost(leaf)
        a.insert(pts, 0), b.insert(moved, 0)
        (ia, ca, sa), (ib, cb, sb) = a.grid(**q), b.grid(**q)
        assert ca.tobytes() == cb.tobytes() and sa.tobytes() == sb.tobytes()
        assert (int(ib["cx0"]) - int(ia["cx0"]), int(ib["cy0"]) - int(ia["cy0"])) == (7, -3) and ib["width"] == ia["width"] and ib["height"] == ia["height"]
        assert float(ib["origin_x"]) - float(ia["origin_x"]) == 7 * c * leaf and float(ia["origin_y"]) - float(ib["origin_y"]) == 3 * c * leaf


def test_the_filter_agrees_with_a_map_pruned_by_it():
    for name, q in (("car", dict(cell_leaves=1, max_miss_ratio=1.0)), ("car", dict(cell_leaves=1, min_frames=2)), ("car", dict(cell_leaves=2, min_frames=2, max_miss_ratio=0.5)),
                    ("scattered", dict(min_frames=2)), ("scattered", dict(min_frames=0, max_miss_ratio=-1.0)), ("scattered", dict(min_frames=-3, max_miss_ratio=-0.5))):
        h, _ = G.host_case(name)
        filtered = h.grid(**q)
        h.prune(q.get("min_frames", 1), q.get("max_miss_ratio", -1.0))
        G.same_grid(h.grid(**{k: v for k, v in q.items() if k == "cell_leaves"}), filtered)


def test_every_refusal():
    h, _ = G.host_case("pole")
    bad = [dict(cell_leaves=0), dict(cell_leaves=65), dict(ground_radius=-1), dict(ground_radius=17), dict(min_height=-0.1), dict(min_height=2.0), dict(min_height=3.0),
           dict(max_height=np.inf), dict(min_height=np.nan), dict(min_obstacle_voxels=0), dict(window=(1.0, 0.0, 0.5, 1.0)), dict(window=(0.0, 1.0, 1.0, 0.5)),
           dict(window=(0.0, 0.0, np.inf, 1.0)), dict(window=(np.nan, 0.0, 1.0, 1.0)), dict(window=(0.0, 0.0, 1.0))]
    for q in bad:
        with pytest.raises(ValueError):
            h.grid(**q)
    with pytest.raises(OverflowError):
        h.grid(cell_leaves=1, max_cells=24)
    assert h.grid(cell_leaves=1, max_cells=25)[1].shape == (5, 5)
    far = D.DenseMapHost(0.25)
    far.insert(G.far_apart(), 0)
    with pytest.raises(OverflowError):
        far.grid()
    assert far.grid(window=(0.0, 0.0, 1.0, 1.0))[1].shape == (3, 3)


def test_files_read_back_with_the_rows_flipped(tmp_path):
    h, queries = G.host_case("car")  # asymmetric: the wall voxel is in the last column of the middle row; make the rows differ too
    h.insert(G.at([[1, 1, 3]]), 6)
    info, cells, state = h.grid(**queries[0])
    assert state[2, 1] == 100 and state[0, 1] == 0
    prefix = str(tmp_path / "plan")
    assert D.write_occupancy_pgm(prefix, info, state) == 27
    data = open(prefix + ".pgm", "rb").read()
    assert data.startswith(b"P5\n9 3\n255\n") and len(data) == len(b"P5\n9 3\n255\n") + 27
    pixels = np.frombuffer(data[-27:], np.uint8).reshape(3, 9)
    assert pixels[0, 1] == 0 and pixels[2, 1] == 254 and pixels[1, 8] == 0  # image row 0 is the grid's last row
    assert sorted(set(pixels.reshape(-1).tolist())) == [0, 254]
    back, resolution, origin = D.read_occupancy_pgm(prefix)
    assert back.dtype == np.int8 and back.tobytes() == state.tobytes() and resolution == float(info["resolution"]) == 0.25
    assert origin == (float(info["origin_x"]), float(info["origin_y"])) == (0.0, -0.25)
    text = open(prefix + ".yaml").read()
    assert text == "image: plan.pgm\nresolution: 0.25\norigin: [0, -0.25, 0]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n"
    # unknown cells
    h2, q2 = G.host_case("slab")
    info, _, state = h2.grid(**q2[0])
    D.write_occupancy_pgm(prefix, info, state)
    assert D.read_occupancy_pgm(prefix)[0].tobytes() == state.tobytes() and 205 in open(prefix + ".pgm", "rb").read()[-30:]
    assert D.write_occupancy_pgm(str(tmp_path / "none"), *D.DenseMapHost(0.25).grid()[::2]) == 0 and not (tmp_path / "none.pgm").exists()
    (tmp_path / "bad.pgm").write_bytes(b"P5\n2 2\n255\n\x00\x01\x02\x03")
    (tmp_path / "bad.yaml").write_text("image: bad.pgm\nnegate: 0\n")
    with pytest.raises(ValueError):
        D.read_occupancy_pgm(str(tmp_path / "bad"))


def test_codes_decode_to_the_floats_they_came_from():
    v = np.array([0.0, -0.0, 1.5, -1.5, 3e38, -3e38, 1e-45, -1e-45], np.float32)
    assert D.dense_order_decode(D.dense_intensity_code(v)).view(np.uint32).tolist() == v.view(np.uint32).tolist()
    assert cloud([[0, 0, 0]]).size == 1


# ---- the file's host code ------------------------------------------------------------------------------------------------------
def test_the_occupancy_writer_is_clean_under_sanitizers(tmp_path):
    """the writer of <prefix>.pgm / .yaml in a stand-alone program with its own main (tests/occupancy_sanitize.cpp), built for the
    CPU with Address + UB sanitizer: grids of 1 x 1, 3 x 2 and 257 x 129 cells from buffers of exactly their size, the row
    flip, the refusals.  Nothing loaded into Python runs under a sanitizer."""
    exe = str(tmp_path / "drv")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off"] + flags + [
        os.path.join(ROOT, "tests", "occupancy_sanitize.cpp"), os.path.join(ROOT, "lidarslam_amd", "csrc", "host", "lsa_occupancy.cpp"), "-o", exe]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-std=c++17"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this compiler has no runtime for -fsanitize=address,undefined")
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    # (as tests/test_dense_normals_host.py: the sanitizers' shadow layout wants the address space unrandomized)
    norand = ["setarch", platform.machine(), "-R"]
    if shutil.which("setarch") is None or subprocess.run(norand + ["true"], capture_output=True).returncode != 0:
        norand = []
    files = tmp_path / "files"
    files.mkdir()
    run = subprocess.run(norand + [exe, str(files)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.startswith("ok"), (run.stdout[-1500:], run.stderr[-3000:])
    # and the files are the ones the Python statement writes
    state = np.fromfile(str(files / "grid3.pgm"), np.uint8)[-6:].reshape(2, 3)
    assert set(state.reshape(-1).tolist()) == {0, 254, 205}
