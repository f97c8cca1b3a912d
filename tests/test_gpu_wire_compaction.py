"""The frame converters' compaction (lsa_wire.hip on lsa_compact.h) at sizes the other converter tests do not reach: past
256 chunks of 1024, where a scatter block adds up the counts of the chunks in front of it in strides of 256."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNK = 1024


def same_points(a, b):
    """field by field (the identity transform used to read the frame back turns -0.0 into +0.0)"""
    return a.size == b.size and all(np.array_equal(a[f], b[f]) for f in a.dtype.names)


def test_polydata_compaction_at_wavefront_chunk_and_stride_borders(O, L):
    """lsa_upload_polydata_frame against O.polydata_to_point_cloud (numpy) on plain random arrays: frames of one point, around
    a wavefront (64), around a chunk (1024), one point into the 257th chunk (the last block sums 256 counts, one a thread)
    and one point into the 258th (the first thread takes a second stride); nothing dropped, points dropped here and there
    and at every chunk's end, everything dropped but the very last point.  Stamp, number kept, all-valid flag and the
    points, field by field."""
    rng = np.random.default_rng(23)
    eye = np.eye(4)
    ctx = L.Context(0)
    try:
        for n in (1, 63, 64, 65, 1023, 1024, 1025, 256 * CHUNK + 1, 257 * CHUNK + 1):
            full = rng.standard_normal((n, 3)).astype(np.float32) * 20
            t = 1e3 + rng.random(n) * 0.1
            lid = rng.integers(0, 128, n).astype(np.uint16)
            inten = (rng.random(n) * 255).astype(np.float32)
            for pattern in ("none", "sprinkled", "all but the last"):
                xyz = full.copy()
                if pattern == "sprinkled":
                    xyz[5::97] = 0
                    xyz[CHUNK - 1 :: CHUNK] = 0
                elif pattern == "all but the last":
                    xyz[:-1] = 0
                want, want_stamp, all_valid = O.polydata_to_point_cloud(xyz, t, lid, inten)
                dropped = n - want.size
                if pattern == "none":
                    assert dropped == 0 and all_valid
                elif pattern == "sprinkled" and n > 1:
                    assert 0 < dropped < n
                elif pattern == "all but the last":
                    assert want.size == 1
                got_stamp, kept, ok = ctx.upload_polydata_frame(xyz, t, lid, inten)
                assert (got_stamp, kept, ok) == (want_stamp, want.size, all_valid), (n, pattern)
                assert same_points(ctx.transform_frame(eye), want), (n, pattern)
    finally:
        ctx.close()


def test_robosense_compaction_past_256_chunks(O, L):
    """lsa_upload_robosense_frame against O.robosense_to_lidar on 128 x 2049 records (257 chunks): 5 % NaN records, 10 %
    second returns, and around the border between chunks 255 and 256 (counted from 0)
      "run"   2500 records of inf across it (they reach the end of the cloud: the last chunk keeps nothing),
      "pair"  a first return in the last record of chunk 255 and its second return in the first record of chunk 256, behind
              2500 records of inf (the pair cannot lie inside the run, so the two are two clouds).
    Number kept and the points, field by field."""
    rng = np.random.default_rng(29)
    eye = np.eye(4)
    height, width = 128, 2049
    n = height * width
    border = 256 * CHUNK
    assert n == border + 128
    dtype = np.dtype({"names": ["x", "y", "z", "intensity"], "formats": ["<f4"] * 4, "offsets": [0, 4, 8, 16], "itemsize": 32})  # pcl::PointXYZI
    layout = (32, 0, 4, 8, 16)
    base = np.zeros(n, dtype)
    for c in "xyz":
        base[c] = rng.standard_normal(n).astype(np.float32) * 20
    base["intensity"] = (rng.random(n) * 255).astype(np.float32)
    base["x"][rng.random(n) < 0.05] = np.nan
    dup = np.nonzero(rng.random(n) < 0.1)[0]
    dup = dup[dup > 0]
    for c in "xyz":
        base[c][dup] = base[c][dup - 1]  # dual return mode: the second return equals the first
    ctx = L.Context(0)
    try:
        for case in ("run", "pair"):
            rec = base.copy()
            if case == "run":
                rec["y"][n - 2500 :] = np.inf
            else:
                rec["y"][border - 1 - 2500 : border - 1] = np.inf
                for c in "xyz":
                    rec[c][border - 1] = np.float32(7.5)
                    rec[c][border] = np.float32(7.5)
            want = O.robosense_to_lidar(rec, width, height, layout, None, 2, 600.0)
            if case == "pair":
                # the case is what it says: the oracle keeps the first return and drops the second
                assert np.count_nonzero((want["x"] == 7.5) & (want["y"] == 7.5) & (want["z"] == 7.5)) == 1
            kept = ctx.upload_robosense_frame(rec, width, height, layout, None, 2, 600.0)
            assert kept == want.size and 0.5 * n < kept < n, case
            assert same_points(ctx.transform_frame(eye), want), case
    finally:
        ctx.close()
