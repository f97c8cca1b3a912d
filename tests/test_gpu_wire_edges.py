"""The three frame converters (lsa_wire.hip) on every input edge of tests/wire_cases.py, held to the plain statements of the
driver nodes there.  Every case runs on two contexts: one whose azimuthal resolution is unset before every upload (a
Velodyne frame is then converted by the host twin, and the other two converters read the frame back for the resolution
estimate), one whose resolution was set beforehand, so that even a one-point frame takes the device path.  Both results,
read with lsa_download_frame, equal the statement byte for byte: -0.0, NaN payloads as the record held them, laser id,
device id, label 0, w = 1.  One exception, the time of a Velodyne frame without a usable time field: the device's arc
tangent is the portable one and the node's is libm's, so |t - t_ref| <= 2e-8 * 600 / rpm seconds for every finite time (2.6
times the 7.6e-9 s that two float arc tangents one ulp off at pi come to), and NaN exactly where the statement has NaN."""
import numpy as np
import pytest

import wire_cases as W

pytestmark = pytest.mark.gpu

AZ_RES = np.float32(2 * np.pi / 1800)


def assert_frame(got, want, what, time_bound=None):
    """byte for byte; time_bound: the time within the bound where finite, NaN exactly where `want` has NaN"""
    assert got.size == want.size, (what, got.size, want.size)
    if time_bound is not None:
        t, tw = got["time"], want["time"]
        assert np.array_equal(np.isnan(t), np.isnan(tw)), (what, "NaN times", int(np.isnan(t).sum()), int(np.isnan(tw).sum()))
        ok = ~np.isnan(tw)
        off = np.abs(t[ok] - tw[ok])
        assert off.size == 0 or off.max() <= time_bound, (what, "time", float(off.max()), time_bound, int((off > time_bound).sum()))
        got = got.copy()
        got["time"] = tw
    if got.tobytes() != want.tobytes():
        for f in got.dtype.names:
            bits = "u%d" % got.dtype[f].itemsize
            bad = np.nonzero(got[f].view(bits) != want[f].view(bits))[0]
            assert bad.size == 0, (what, f, bad.size, bad[:5], got[f][bad[:5]], want[f][bad[:5]])
        raise AssertionError((what, "padding differs"))


@pytest.fixture
def contexts(L):
    """(resolution unset before every upload, resolution set beforehand)"""
    fresh, preset = L.Context(0), L.Context(0)
    preset.azimuthal_resolution = AZ_RES
    yield fresh, preset
    fresh.close()
    preset.close()


def plain_frame(L, f):
    """a well-formed scan of the product's own generator with its rings made equally long (RoboSense wants a grid), ring-major"""
    pts, _ = L.synth_frame(16, 1000, f)
    per = int(np.bincount(pts["laser_id"], minlength=16).min())
    rows = [pts[pts["laser_id"] == r][:per] for r in range(16)]
    return np.concatenate(rows), per


def keypoints_of(L, cloud, az):
    ctx = L.Context(0)
    try:
        ctx.azimuthal_resolution = az
        ctx.upload_frame(cloud)
        return ctx.extract_keypoints().tolist()
    finally:
        ctx.close()


def check_keypoints(L, ctx, want, what):
    """the converted frame yields the keypoints of the statement's cloud uploaded as it is"""
    counts = ctx.extract_keypoints().tolist()
    assert sum(counts) > 0 and counts == keypoints_of(L, want, ctx.azimuthal_resolution), (what, counts)


def test_velodyne_records_on_every_edge(L, contexts):
    fresh, preset = contexts
    compared = expected = 0
    for case in W.velodyne_cases():
        for rpm, first in W.ADVANCEMENT_SETTINGS if not case.time_valid else W.ADVANCEMENT_SETTINGS[:1]:
            want, valid, _ = W.velodyne_node(case.records, case.layout, case.mapping, case.device_id, rpm, first)
            assert valid == case.time_valid and want.size == case.n
            bound = None if valid else 2e-8 * 600.0 / rpm
            expected += 2 * case.n
            for ctx, path in ((fresh, "host"), (preset, "device")):
                if ctx is fresh:
                    ctx.azimuthal_resolution = 0.0  # the host twin converts the frame
                ctx.upload_wire_frame(case.records, case.layout, case.mapping, case.device_id, rpm, first)
                got = ctx.download_frame()
                assert_frame(got, want, (case.name, rpm, first, path), bound)
                compared += got.size
        if case.time_valid and case.host_path:
            # laser ids the ring bucketing cannot hold: the extraction refuses the frame, and walks no slot nobody filled
            with pytest.raises(L.LsaError, match="laser_id >= 512"):
                preset.extract_keypoints()
    assert compared == expected > 390000  # no case compares fewer points than the frame holds
    # after the family: a plain well-formed frame still converts, on both contexts, and yields keypoints
    fresh.azimuthal_resolution = 0.0  # estimated from the plain frame, not left over from an edge case
    for f, ctx in enumerate((fresh, preset)):
        pts, _ = plain_frame(L, f)
        rec = W.pack_records(W.VELODYNE_LAYOUT, pts["x"], pts["y"], pts["z"], pts["intensity"], pts["laser_id"], pts["time"].astype(np.float32))
        want, valid, _ = W.velodyne_node(rec, W.VELODYNE_LAYOUT)
        assert valid
        ctx.upload_wire_frame(rec, W.VELODYNE_LAYOUT)
        assert_frame(ctx.download_frame(), want, "plain frame")
        check_keypoints(L, ctx, want, "plain frame")


def test_polydata_arrays_on_every_edge(L, contexts):
    fresh, preset = contexts
    for case in W.polydata_cases():
        want, want_stamp, want_valid = W.polydata_filter(case.xyz, case.time, case.laser_id, case.intensity, case.mapping, case.factor)
        for ctx in contexts:
            if ctx is fresh:
                ctx.azimuthal_resolution = 0.0
            stamp, kept, valid = ctx.upload_polydata_frame(case.xyz, case.time, case.laser_id, case.intensity, case.mapping, case.factor)
            assert (stamp, kept, valid) == (want_stamp, want.size, want_valid), case.name
            assert_frame(ctx.download_frame(), want, case.name)
    fresh.azimuthal_resolution = 0.0  # estimated from the plain frame, not left over from an edge case
    for f, ctx in enumerate((fresh, preset)):
        pts, _ = plain_frame(L, f)
        xyz = np.stack([pts["x"], pts["y"], pts["z"]], axis=1)
        t = 100.0 + pts["time"]
        want, want_stamp, want_valid = W.polydata_filter(xyz, t, pts["laser_id"], pts["intensity"])
        assert ctx.upload_polydata_frame(xyz, t, pts["laser_id"], pts["intensity"]) == (want_stamp, want.size, want_valid)
        assert_frame(ctx.download_frame(), want, "plain frame")
        check_keypoints(L, ctx, want, "plain frame")


def test_robosense_clouds_on_every_edge(L, contexts):
    fresh, preset = contexts
    for case in W.robosense_cases():
        want = W.robosense_node(case.records, case.width, case.height, case.layout, case.mapping, case.device_id, case.rpm)
        for ctx in contexts:
            if ctx is fresh:
                ctx.azimuthal_resolution = 0.0
            kept = ctx.upload_robosense_frame(case.records, case.width, case.height, case.layout, case.mapping, case.device_id, case.rpm)
            assert kept == want.size, case.name
            if kept == 0:
                with pytest.raises(L.LsaError):
                    ctx.download_frame()  # no frame
            else:
                assert_frame(ctx.download_frame(), want, case.name)
    fresh.azimuthal_resolution = 0.0  # estimated from the plain frame, not left over from an edge case
    for f, ctx in enumerate((fresh, preset)):
        pts, per = plain_frame(L, f)
        layout = W.RS_LAYOUTS[1]
        rec = W.rs_pack(layout, pts["x"], pts["y"], pts["z"], pts["intensity"])
        want = W.robosense_node(rec, per, 16, layout)
        assert ctx.upload_robosense_frame(rec, per, 16, layout) == want.size > 0.9 * pts.size
        assert_frame(ctx.download_frame(), want, "plain frame")
        check_keypoints(L, ctx, want, "plain frame")


def test_robosense_cloud_of_1026_chunks(L):
    """128 x 8201 records: k_rs_carry takes its second stride of 1024 chunks, with a run of non-finite records across chunks
    1023 .. 1025 and a first / second return pair astride it"""
    case = W.robosense_large_case()
    want = W.robosense_node(case.records, case.width, case.height, case.layout, case.mapping, case.device_id, case.rpm)
    assert int(((want["x"] == 7.5) & (want["y"] == 7.5) & (want["z"] == 7.5)).sum()) == 1
    ctx = L.Context(0)
    try:
        ctx.azimuthal_resolution = AZ_RES
        assert ctx.upload_robosense_frame(case.records, case.width, case.height, case.layout, case.mapping, case.device_id, case.rpm) == want.size
        assert_frame(ctx.download_frame(), want, case.name)
    finally:
        ctx.close()
