"""The plain statements of the three driver nodes (tests/wire_cases.py) against the oracle's own restatements, on every case
inside the oracle's domain, bit for bit; and the conditions that keep the cases from being vacuous or from hanging on a
rounding: every decision of the advancement estimator has a margin, every NaN case tells the estimator's loop from "the
first descent and everything after it".  No GPU."""
import math

import numpy as np
import pytest

import wire_cases as W


def assert_same_bytes(got, want, what, any_nan_time=False):
    """bit for bit, field by field; any_nan_time: a NaN time (an advancement frame's, computed from a NaN coordinate) stands
    exactly where the other side has one, whatever its sign and payload"""
    assert got.size == want.size, (what, got.size, want.size)
    if got.tobytes() != want.tobytes():
        for f in got.dtype.names:
            bits = "u%d" % got.dtype[f].itemsize
            differ = got[f].view(bits) != want[f].view(bits)
            if f == "time" and any_nan_time:
                differ &= ~(np.isnan(got[f]) & np.isnan(want[f]))
            bad = np.nonzero(differ)[0]
            assert bad.size == 0, (what, f, bad.size, bad[:5], got[f][bad[:5]], want[f][bad[:5]])


@pytest.fixture(scope="module")
def velodyne():
    return W.velodyne_cases()


def in_oracle_domain(case):
    """the oracle indexes the mapping as the node does: it must cover every ring"""
    if case.mapping is None:
        return True
    return int(W.unpack_records(case.records, case.layout)[5].max()) < len(case.mapping)


def test_velodyne_statement_is_the_oracles_node_bit_for_bit(O, velodyne):
    """Every Velodyne case inside the oracle's domain.  In advancement frames both sides then use libm's atan2f (the node's
    std::atan2(float, float)): bit for bit as well.  The statement's default, math.atan2 in double, stays within the 7.6e-8
    turns of two float arc tangents one ulp (at pi) off."""
    atan2f = W.libm_atan2f()
    compared = 0
    for case in velodyne:
        if not in_oracle_domain(case):
            continue
        for rpm, first in W.ADVANCEMENT_SETTINGS if not case.time_valid else W.ADVANCEMENT_SETTINGS[:1]:
            want, want_valid = O.velodyne_to_lidar(case.records, case.layout, case.mapping, case.device_id, rpm, first)
            got, valid, _ = W.velodyne_node(case.records, case.layout, case.mapping, case.device_id, rpm, first, atan2=atan2f)
            assert valid == want_valid == case.time_valid, case.name
            assert_same_bytes(got, want, (case.name, rpm, first), any_nan_time=not valid)
            compared += got.size
            if not valid:
                plain = W.velodyne_node(case.records, case.layout, case.mapping, case.device_id, rpm, first)[0]
                t, tw = plain["time"], want["time"]
                assert np.array_equal(np.isnan(t), np.isnan(tw)), case.name
                ok = ~np.isnan(t)
                assert ok.sum() == 0 or np.abs(t[ok] - tw[ok]).max() <= 7.6e-8 * 60.0 / rpm * 1.01, (case.name, np.abs(t[ok] - tw[ok]).max())
                plain["time"] = want["time"]
                assert_same_bytes(plain, want, (case.name, "all but the time"))
    assert compared > 100000
    # what the oracle cannot be asked: rings behind the mapping's end.  The rule is the product's: 0xffff, all else as ever.
    outside = [c for c in velodyne if not in_oracle_domain(c)]
    assert outside
    for case in outside:
        got = W.velodyne_node(case.records, case.layout, case.mapping, case.device_id)[0]
        ring = W.unpack_records(case.records, case.layout)[5]
        behind = ring >= len(case.mapping)
        assert behind.any() and (got["laser_id"][behind] == 0xFFFF).all()
        assert np.array_equal(got["laser_id"][~behind], np.asarray(case.mapping)[ring[~behind]])


def test_velodyne_cases_are_what_they_say(velodyne):
    """sizes, layouts, mappings, device ids, the threshold's four frames, non-finite values present"""
    timed = [c for c in velodyne if c.time_valid]
    assert {c.n for c in timed} >= {2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049}
    assert any(c.n == 1 for c in velodyne)  # a single record's time field is never usable: last - first = 0
    assert {c.layout for c in timed} == {W.VELODYNE_LAYOUT, W.PACKED_LAYOUT} and {c.device_id for c in timed} == {0, 255}
    assert {"none" if c.mapping is None else "short" if c.host_path else "full" for c in timed} == {"none", "short", "full"}
    seen = set()
    for c in timed:
        x, y, z, intensity, _, _ = W.unpack_records(c.records, c.layout)
        for a in (x, y, z, intensity):
            seen |= {"nan"} if np.isnan(a).any() else set()
            seen |= {"inf"} if np.isinf(a).any() else set()
            seen |= {"-0"} if ((a == 0) & np.signbit(a)).any() else set()
            seen |= {"payload"} if (a.view(np.uint32) == 0x7FC12345).any() else set()
    assert seen == {"nan", "inf", "-0", "payload"}
    threshold = {c.name: c for c in W.velodyne_threshold_cases()}
    assert len(threshold) == 4 and sum(c.time_valid for c in threshold.values()) == 1
    for c in threshold.values():
        assert W.velodyne_node(c.records, c.layout)[1] == c.time_valid, c.name
    assert float(np.float32(1e-8)) < 1e-8 < float(np.nextafter(np.float32(1e-8), np.float32(1)))
    host = [c for c in velodyne if c.host_path and not c.time_valid]
    assert len(host) >= 2 and all((W.velodyne_node(c.records, c.layout, c.mapping)[0]["laser_id"] >= W.MAX_RINGS).any() for c in host)
    long_ring = [c for c in velodyne if "8193" in c.name][0]
    assert np.bincount(W.unpack_records(long_ring.records, long_ring.layout)[5]).max() == 8193


def test_every_decision_of_the_estimator_has_a_margin(velodyne):
    """On the reference alone, no point left out: the estimator's comparison and the wrap are at least 1e-6 turns from
    tipping, unless the two points compared have bit-equal x and y (both sides then compute the very same value).  Two float
    arc tangents are each off by at most one float ulp at pi, 2.4e-7 rad: 7.6e-8 turns between the node's libm value and the
    device's rounded double; 1e-6 is 13 times that."""
    checked = 0
    for case in velodyne:
        if case.time_valid:
            continue
        for atan2 in (None, W.libm_atan2f()):
            pts, valid, m = W.velodyne_node(case.records, case.layout, case.mapping, case.device_id, **({"atan2": atan2} if atan2 else {}))
            assert not valid and pts.size == case.n == m["compare"].size == m["wrap"].size
            bad = np.nonzero(~((m["compare"] >= W.MARGIN) | m["same_as_previous"]))[0]
            assert bad.size == 0, (case.name, "comparison", bad[:5], m["compare"][bad[:5]])
            bad = np.nonzero(~((m["wrap"] >= W.MARGIN) | m["same_as_first"]))[0]
            assert bad.size == 0, (case.name, "wrap", bad[:5], m["wrap"][bad[:5]])
            checked += case.n
    assert checked > 50000


def test_nan_cases_tell_the_loop_from_the_first_descent_rule(velodyne):
    """Every NaN case has at least 20 points on which "the first descent and everything after it" is a whole turn off the
    node's loop; without NaN the two agree bit for bit on every case.  (Where the frame's first record is NaN every time is
    NaN under either rule: that case can tell nothing apart and is not counted among them.)"""
    nan_cases = 0
    for case in velodyne:
        if case.time_valid:
            continue
        for rpm, first in W.ADVANCEMENT_SETTINGS:
            node = W.velodyne_node(case.records, case.layout, case.mapping, case.device_id, rpm, first)[0]["time"]
            rule = W.first_descent_rule(case.records, case.layout, case.mapping, case.device_id, rpm, first)
            assert np.array_equal(np.isnan(node), np.isnan(rule))
            ok = ~np.isnan(node)
            off = np.abs(rule[ok] - node[ok])
            turn = 60.0 / rpm
            a_turn_off = int((np.abs(off - turn) < 1e-9).sum())
            assert ((off == 0) | (np.abs(off - turn) < 1e-9)).all(), case.name
            if case.nan_case:
                assert a_turn_off >= 20, (case.name, a_turn_off)
                nan_cases += 1
            elif not np.isnan(node).any():
                assert a_turn_off == 0 and np.array_equal(rule, node), case.name
    assert nan_cases == 4 * len(W.ADVANCEMENT_SETTINGS)
    first_nan = [c for c in velodyne if c.name.startswith("NaN first record")][0]
    assert np.isnan(W.velodyne_node(first_nan.records, first_nan.layout)[0]["time"]).all()


def test_the_estimators_rule_in_closed_form(velodyne):
    """"+ 1 exactly when the ring's last descent lies behind the ring's last NaN advancement" is the loop, on every case:
    the rule the device scans for, stated with two running maxima."""
    for case in velodyne:
        if case.time_valid:
            continue
        x, y, _, _, _, ring = W.unpack_records(case.records, case.layout)
        lid = W.laser_ids(ring, case.mapping)
        _, adv = W.frame_advancements(x, y, math.atan2)
        want = W.velodyne_node(case.records, case.layout, case.mapping, case.device_id, 600.0, True)[0]["time"]
        got = adv.copy()
        for r in np.unique(lid):
            idx = np.nonzero(lid == r)[0]
            a = adv[idx]
            k = np.arange(a.size)
            with np.errstate(invalid="ignore"):
                descent = np.concatenate([[False], a[1:] < a[:-1]])
            last_descent = np.maximum.accumulate(np.where(descent, k, -1))
            last_reset = np.maximum.accumulate(np.where(np.isnan(a), k, -1))
            got[idx] = a + (last_descent > last_reset)
        got = got / 600.0 * 60.0
        assert np.array_equal(got.view(np.uint64)[~np.isnan(want)], want.view(np.uint64)[~np.isnan(want)]), case.name
        assert np.array_equal(np.isnan(got), np.isnan(want)), case.name


def test_robosense_statement_is_the_oracles_node_bit_for_bit(O):
    """every RoboSense case, the cloud of 1026 chunks included, and that the edge records do what the cases say"""
    for case in W.robosense_cases() + [W.robosense_large_case()]:
        want = O.robosense_to_lidar(case.records, case.width, case.height, case.layout, case.mapping, case.device_id, case.rpm)
        got = W.robosense_node(case.records, case.width, case.height, case.layout, case.mapping, case.device_id, case.rpm)
        assert_same_bytes(got, want, case.name)
        n = case.width * case.height
        if n >= 60 and got.size and n < 10000:  # the clouds with the edge records (_rs_edges)
            xyz = np.stack([got["x"], got["y"], got["z"]], axis=1)

            def count(v):
                return int((xyz == np.asarray(v, np.float32)).all(axis=1).sum())

            assert count((3, 4, 5)) == 1 and count((6, 7, 8)) == 1 and count((0, 9, 9)) == 1, case.name  # triple, across NaN, signed zero
            kept_zero = got["x"][(got["y"] == 9) & (got["z"] == 9)]
            assert kept_zero.size == 1 and not np.signbit(kept_zero[0])               # the +0.0 came first and stays
            assert np.signbit(got["x"][(got["y"] == -9)]).all() and count((0, -9, 9)) == 1 and count((0, -9, 8)) == 1
            assert np.isfinite(xyz).all()
            if case.width >= 3 and n > 100:
                assert count((11, 12, 13)) == 1, case.name                              # the pair across a ring border
    large = W.robosense_large_case()
    got = W.robosense_node(large.records, large.width, large.height, large.layout, large.mapping, large.device_id, large.rpm)
    assert int(((got["x"] == 7.5) & (got["y"] == 7.5) & (got["z"] == 7.5)).sum()) == 1  # the pair astride the run: the second is dropped
    assert {c.height for c in W.robosense_cases()} >= {16, 32, 128} and {c.layout[0] for c in W.robosense_cases()} == {16, 32}
    assert {c.width * c.height for c in W.robosense_cases()} >= {1, 63, 64, 65}


def test_polydata_statement_is_the_oracles_filter(O):
    """every LidarView case: points bit for bit, stamp, all-valid flag; and that the cases hold what they say"""
    cases = W.polydata_cases()
    seen_types = {"time": set(), "laser": set(), "intensity": set(), "xyz": set()}
    for case in cases:
        with np.errstate(over="ignore", invalid="ignore"):
            want, want_stamp, want_valid = O.polydata_to_point_cloud(case.xyz, case.time, case.laser_id, case.intensity, case.mapping, case.factor)
        got, stamp, valid = W.polydata_filter(case.xyz, case.time, case.laser_id, case.intensity, case.mapping, case.factor)
        assert (stamp, valid) == (want_stamp, want_valid), (case.name, stamp, want_stamp)
        assert_same_bytes(got, want, case.name)
        for k, a in (("time", case.time), ("laser", case.laser_id), ("intensity", case.intensity), ("xyz", case.xyz)):
            seen_types[k].add(a.dtype.type)
    assert all(seen_types[k] == set(W.SCALAR_TYPES) for k in ("time", "laser", "intensity")) and seen_types["xyz"] == {np.float32, np.float64}
    assert {c.time.size for c in cases} >= {1, 63, 64, 65, 1023, 1024, 1025}
    by_name = {c.name: c for c in cases}
    c = [c for c in cases if c.name.startswith("n=65 xyz=float32")][0]
    got, _, valid = W.polydata_filter(c.xyz, c.time, c.laser_id, c.intensity, c.mapping, c.factor)
    assert not valid and got.size == 65 - 2                                        # the all -0.0 point and the all +0.0 point are dropped
    assert np.signbit(got["y"][4]) and got["y"][4] == 0 and got["x"][4] != 0       # one -0.0 coordinate survives (point 6, two dropped before it)
    assert np.isnan(got["y"][5]) and got["x"][5] == 0                              # (0, NaN, 0) is kept
    c = by_name["f64 coordinates that round and overflow when narrowed"]
    got = W.polydata_filter(c.xyz, c.time, c.laser_id, c.intensity)[0]
    assert got["z"][10] == 16777216.0 and got["y"][10] == 1.0 and np.isinf([got["x"][11], got["y"][11], got["z"][11]]).all() and got["y"][11] < 0
    assert got["x"][12] == np.finfo(np.float32).max and got["y"][12] == 0 and np.signbit(got["z"][12]) and np.isinf(got["intensity"][13])
    for name in ("first point", "last point", "a dropped point"):
        c = by_name[f"frame end time in {name}"]
        got, stamp, _ = W.polydata_filter(c.xyz, c.time, c.laser_id, c.intensity)
        assert stamp == 1000500000 and got.size == 299 and (got["time"] <= 0).all() and ((got["time"] == 0).sum() == (0 if "dropped" in name else 1))
    got, stamp, _ = W.polydata_filter(*[getattr(by_name["time -0.0 alone"], f) for f in ("xyz", "time", "laser_id", "intensity")])
    assert stamp == 0 and (got["time"] == 0).all() and not np.signbit(got["time"]).any()  # -0.0 - -0.0 = +0.0
    for name in ("factor 1, a stamp that truncates", "factor 1e-6, a stamp that truncates"):
        c = by_name[name]
        end = float(c.time.max()) * (c.factor * 1e6)
        assert end != int(end) and W.polydata_filter(c.xyz, c.time, c.laser_id, c.intensity, None, c.factor)[1] == int(end)
