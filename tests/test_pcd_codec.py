"""The host PCD codec (lsa_pcd_info / lsa_pcd_read / lsa_pcd_write, lsa_lzf_*) against the independent reader, writer and
LZF decoder of tests/pcd_cases.py.  No GPU."""
import os

import numpy as np
import pytest

import pcd_cases as P


@pytest.fixture(scope="module")
def cloud(L):
    """Several thousand synthetic points with the values a text or a narrowing path gets wrong."""
    rng = np.random.default_rng(7)
    n = 5003
    p = np.zeros(n, L.POINT_DTYPE)
    for f in ("x", "y", "z"):
        p[f] = (rng.standard_normal(n) * 40).astype(np.float32)
    p["w"] = 1.0
    p["time"] = rng.uniform(-0.1, 1.7e9, n) + rng.uniform(0, 1, n) * 1e-7  # needs all of a double
    p["intensity"] = rng.uniform(0, 255, n).astype(np.float32)
    p["laser_id"] = rng.integers(0, 128, n)
    p["device_id"] = rng.integers(0, 256, n)
    p["label"] = rng.integers(0, 256, n)
    p["x"][0], p["y"][0] = -0.0, 0.0
    p["x"][1] = np.float32(1e-45)                       # smallest denormal
    p["y"][1] = -np.frombuffer(np.uint32(0x007FFFFF).tobytes(), np.float32)[0]  # largest denormal
    p["z"][1] = np.finfo(np.float32).max
    p["intensity"][2] = np.finfo(np.float32).tiny
    p["laser_id"][3] = 65535
    p["time"][4] = np.nextafter(1.0, 2.0)
    p["time"][5] = -0.0
    p["time"][6] = 5e-324
    p["time"][7] = 1697529600.123456789
    p["x"][8] = np.float32(0.1)
    p["x"][9] = np.float32(16777217.0)
    return p


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_written_files_read_back_bit_for_bit_in_the_helper(L, cloud, tmp_path, fmt):
    path = str(tmp_path / "cloud.pcd")
    assert L.write_pcd(path, cloud, fmt)
    assert L.pcd_info(path) == (cloud.size, fmt)
    fields, cols, name = P.read(path)
    assert name == P.FORMATS[fmt]
    assert [(f[0], f[1], f[2], f[3]) for f in fields] == [(f[0], f[1], f[2], 1) for f in P.POINT_FIELDS]
    for f, _, _ in P.POINT_FIELDS:
        got = np.ascontiguousarray(cols[f][:, 0])
        assert got.dtype == cloud.dtype[f]
        assert got.tobytes() == np.ascontiguousarray(cloud[f]).tobytes(), f
    # and through the library's own reader
    back = L.read_pcd(path)
    assert P.same_bits(back, cloud)


def test_an_empty_cloud_writes_no_file(L, cloud, tmp_path):
    path = str(tmp_path / "empty.pcd")
    assert L.lib().lsa_pcd_write(path.encode(), None, 0, 1) == -3  # savePointCloudToPCD's result for an empty cloud
    assert not os.path.exists(path)
    assert L.write_pcd(path, cloud[:0]) is False
    assert L.lib().lsa_pcd_write(path.encode(), L.ptr(cloud), 4, 7) == -4
    assert not os.path.exists(path)


def foreign_columns(cloud):
    """what a file of another producer may hold: permuted fields, an extra one, other types, a vector field, no time"""
    n = cloud.size
    rng = np.random.default_rng(11)
    columns = {
        "x": cloud["x"].astype(np.float64) + 1e-9,  # F 8: rounds to float on the way in
        "y": cloud["y"].astype(np.float64),
        "z": cloud["z"].astype(np.float64) * (1 + 1e-12),
        "intensity": rng.integers(0, 256, n),       # U 1
        "laser_id": rng.integers(-3, 128, n),       # I 4: negative values wrap as C++ converts them
        "device_id": rng.integers(0, 70000, n),     # U 4: narrowed to a byte
        "label": rng.integers(0, 4, n),             # I 1
        "normal_x": rng.standard_normal(n),         # not a LidarPoint field
        "rgb": rng.standard_normal((n, 3)),         # COUNT 3, ignored by its width
    }
    fields = [("rgb", "F", 4, 3), ("label", "I", 1, 1), ("z", "F", 8, 1), ("normal_x", "F", 4, 1), ("intensity", "U", 1, 1), ("x", "F", 8, 1),
              ("device_id", "U", 4, 1), ("y", "F", 8, 1), ("laser_id", "I", 4, 1)]
    return columns, fields


@pytest.mark.parametrize("fmt", P.FORMATS)
def test_foreign_layouts_read_as_the_helper_decodes_them(L, cloud, tmp_path, fmt):
    columns, fields = foreign_columns(cloud[:1501])
    path = str(tmp_path / "foreign.pcd")
    P.write(path, columns, fields, fmt)
    expected = P.read_points(path, L.POINT_DTYPE)
    assert not expected["time"].any() and (expected["w"] == 1).all()  # no time field: 0
    assert expected["laser_id"].max() > 65000                        # the negative ring numbers wrapped
    got = L.read_pcd(path)
    for f in L.POINT_DTYPE.names:
        assert np.ascontiguousarray(got[f]).tobytes() == np.ascontiguousarray(expected[f]).tobytes(), f


@pytest.mark.parametrize("fmt", P.FORMATS)
def test_helper_written_lidar_points_read_back(L, cloud, tmp_path, fmt):
    path = str(tmp_path / "points.pcd")
    P.write_points(path, cloud[:2000], fmt)
    assert P.same_bits(L.read_pcd(path), cloud[:2000])


def test_count_on_a_used_field_is_not_taken(L, cloud, tmp_path):
    n = 100
    path = str(tmp_path / "count.pcd")
    P.write(path, {"x": np.ones((n, 2)), "y": cloud["y"][:n]}, [("x", "F", 4, 2), ("y", "F", 4, 1)], "binary")
    got = L.read_pcd(path)
    assert not got["x"].any() and got["y"].tobytes() == cloud["y"][:n].tobytes()


LZF_INPUTS = {
    "empty": b"",
    "one byte": b"\x07",
    "zero columns": bytes(100000),
    "random": np.random.default_rng(3).integers(0, 256, 70001, dtype=np.uint8).tobytes(),
    "a run longer than the longest reference": b"ab" + b"\x55" * 1000 + b"cd",
    "a period longer than the longest distance": np.random.default_rng(4).integers(0, 256, 9000, dtype=np.uint8).tobytes() * 3,
    "columns of points": np.tile(np.arange(256, dtype=np.uint8), 40).tobytes() + bytes(5000) + np.repeat(np.arange(64, dtype=np.uint8), 64).tobytes(),
}


@pytest.mark.parametrize("name", list(LZF_INPUTS))
def test_compressed_streams_decode_in_the_helper(L, name):
    data = LZF_INPUTS[name]
    z = L.lzf_compress(data)
    assert P.lzf_decode(z) == data
    assert L.lzf_decompress(z, len(data)) == data
    if name in ("zero columns", "a run longer than the longest reference", "columns of points"):
        assert len(z) < len(data) // 4, (len(z), len(data))  # it does compress


def test_hand_made_streams_decode_in_the_library(L):
    # a literal run of 3; a short reference (length 3, distance 3); a literal; a long reference of 7 + 20 + 2 bytes at
    # distance 1 (overlapping: a run); a reference at the longest distance there is room for
    stream = bytes([2]) + b"abc" + bytes([(1 << 5) | 0, 2]) + bytes([0]) + b"z" + bytes([(7 << 5) | 0, 20, 0])
    expected = b"abc" + b"abc" + b"z" + b"z" * 29
    assert P.lzf_decode(stream) == expected
    assert L.lzf_decompress(stream, len(expected)) == expected
    head = np.random.default_rng(5).integers(0, 256, 8192, dtype=np.uint8).tobytes()
    stream = P.lzf_literals(head) + bytes([(5 << 5) | 31, 255])  # length 7, distance 8192
    expected = head + head[:7]
    assert P.lzf_decode(stream) == expected
    assert L.lzf_decompress(stream, len(expected)) == expected
    # 32 literals, the longest run
    stream = bytes([31]) + bytes(range(32))
    assert L.lzf_decompress(stream, 32) == bytes(range(32))
    # malformed: a reference before the start, a run past the end, more output than room
    for bad, room in ((bytes([(1 << 5) | 0, 5]), 64), (bytes([5]) + b"ab", 64), (bytes([3]) + b"abcd", 3)):
        with pytest.raises(L.LsaError):
            L.lzf_decompress(bad, room)


def malformed_files(tmp, cloud):
    """name -> path of a file whose header or data section is broken, one for every case the reader must refuse"""
    good = os.path.join(tmp, "good.pcd")
    P.write_points(good, cloud[:50], "binary")
    blob = open(good, "rb").read()
    head, data = blob[: blob.index(b"DATA binary\n") + 12], blob[blob.index(b"DATA binary\n") + 12 :]
    out = {}

    def put(name, content):
        out[name] = os.path.join(tmp, name.replace(" ", "_") + ".pcd")
        open(out[name], "wb").write(content)

    put("sizes do not add up", head.replace(b"SIZE 4 4 4 8 4 2 1 1", b"SIZE 4 4 4 8 4 2 1") + data)
    put("types do not add up", head.replace(b"TYPE F F F F F U U U", b"TYPE F F F F F U U U U") + data)
    put("points is not width times height", head.replace(b"POINTS 50", b"POINTS 49") + data)
    put("truncated binary data", head + data[:-5])
    put("no data entry", head.replace(b"DATA binary\n", b""))
    put("bad size", head.replace(b"SIZE 4 4 4 8", b"SIZE 4 3 4 8") + data)
    put("unknown format", head.replace(b"DATA binary", b"DATA zipped") + data)
    asc = os.path.join(tmp, "asc.pcd")
    P.write_points(asc, cloud[:50], "ascii")
    rows = open(asc, "rb").read()
    put("truncated ascii data", rows[: rows.rindex(b"\n", 0, len(rows) - 1) - 20])
    comp = os.path.join(tmp, "comp.pcd")
    P.write_points(comp, cloud[:50], "binary_compressed")
    blob = open(comp, "rb").read()
    at = blob.index(b"DATA binary_compressed\n") + 23
    csize = int(np.frombuffer(blob, "<u4", 1, at)[0])
    put("truncated compressed data", blob[:-9])
    put("lzf stream of the wrong length", blob[:at] + np.array([csize - 33, 50 * 28], "<u4").tobytes() + blob[at + 8 : at + 8 + csize - 33])
    put("every count zero", head.replace(b"COUNT 1 1 1 1 1 1 1 1", b"COUNT 0 0 0 0 0 0 0 0") + data)
    huge = head.replace(b"WIDTH 50", b"WIDTH 2000000000").replace(b"POINTS 50", b"POINTS 2000000000")
    put("points beyond the binary file", huge + data)
    put("points beyond the ascii file", huge.replace(b"DATA binary", b"DATA ascii") + b"1 2 3\n")
    put("points beyond the compressed file", huge.replace(b"DATA binary", b"DATA binary_compressed") + np.array([4, 4], "<u4").tobytes() + b"\x03abcd")
    put("raw size is not points times record", blob[:at] + np.array([csize, 50 * 28 - 1], "<u4").tobytes() + blob[at + 8 :])
    return out


CASES = ["sizes do not add up", "types do not add up", "points is not width times height", "truncated binary data", "no data entry", "bad size", "unknown format",
         "truncated ascii data", "truncated compressed data", "lzf stream of the wrong length", "raw size is not points times record",
         "every count zero", "points beyond the binary file", "points beyond the ascii file", "points beyond the compressed file"]


@pytest.mark.parametrize("case", CASES)
def test_malformed_files_are_refused_by_name(L, cloud, tmp_path, case):
    path = malformed_files(str(tmp_path), cloud)[case]
    out = np.zeros(64, L.POINT_DTYPE)
    lib = L.lib()
    n, fmt = np.zeros(1, np.int32), np.zeros(1, np.int32)
    rc_info = lib.lsa_pcd_info(path.encode(), n.ctypes.data_as(__import__("ctypes").POINTER(__import__("ctypes").c_int)), fmt.ctypes.data_as(__import__("ctypes").POINTER(__import__("ctypes").c_int)))
    rc = lib.lsa_pcd_read(path.encode(), L.ptr(out), out.size)
    assert rc == -3, (case, rc)  # LSA_E_ARG
    message = lib.lsa_pcd_last_error().decode()
    assert os.path.basename(path) in message, message
    if "truncated" not in case and "lzf" not in case and "raw size" not in case and "beyond" not in case:
        assert rc_info == -3  # the header alone gives it away
    assert any(ch.isdigit() for ch in message.split(os.path.basename(path))[1][:6]), message  # file:line


def test_ascii_rows_that_end_with_the_file_are_read(L, cloud, tmp_path):
    """no line end behind the last row: the text ends in a digit, and parsing stops there"""
    path = str(tmp_path / "rows.pcd")
    P.write_points(path, cloud[:300], "ascii")
    blob = open(path, "rb").read()
    assert blob.endswith(b"\n") and blob[-2:-1].isdigit()
    open(path, "wb").write(blob[:-1])
    assert P.same_bits(L.read_pcd(path), cloud[:300])


def test_a_missing_file_is_an_error(L, tmp_path):
    with pytest.raises(L.LsaError):
        L.read_pcd(str(tmp_path / "nothing.pcd"))
