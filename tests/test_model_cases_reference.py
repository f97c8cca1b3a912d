"""The sheets of tests/model_cases.py have to be what they say before the device fits are held to them
(tests/test_gpu_model_branches.py): every sheet through the oracle's matcher -- both edge filters, every type -- reaches
exactly the statuses it declares; where the plain reference of model_cases applies, its kept set and its status equal the
oracle's; every ladder flips exactly once; the rounding-decided sheets split the way they promise.  No GPU.

The kept set is observed through the record: columns 9 .. 11 are the mean of the kept points, summed in double over at most
16 floats below 512 (rounding about 2e-12), and the case builder has asserted that flipping any single candidate's
membership moves that mean by more than 5e-5."""
import numpy as np
import pytest

import knn_cases as K
import model_cases as M

IDS = dict(ids=lambda s: s.name)
PLAIN = [s for s in M.SHEETS if any(h.plain for h in s.hoods)]
ROBUST = [s for s in M.SHEETS if s.robust.any()]
LADDERS = [s for s in M.SHEETS if s.ladders]


@pytest.mark.parametrize("sheet", M.SHEETS, **IDS)
def test_sheet_reaches_exactly_what_it_declares(sheet, O):
    st, w, rec, hist = M.oracle_match(sheet, O)
    if sheet.family == "rounding_decided":  # rounding decides which of them, sheet by sheet; the family reaches all (below)
        assert set(st.tolist()) <= set(sheet.declares), (sorted(set(st.tolist())), sorted(sheet.declares))
    else:
        assert set(st.tolist()) == set(sheet.declares), (sorted(set(st.tolist())), sorted(sheet.declares))
    assert hist.tolist() == np.bincount(st, minlength=8).tolist()
    for i, h in enumerate(sheet.hoods):
        assert h.expect is None or st[i] == h.expect, (h.label, i, int(st[i]))
    if sheet.ktype == M.EDGE and not sheet.mp.single_edge_per_ring and sheet.family != "ransac_zero_direction":
        assert not np.any(st == M.MSE_LARGE)  # unreachable behind the RANSAC filter while the winner is a line (model_cases' docstring)
    ok = st == M.SUCCESS
    assert np.array_equal(rec[ok, 12:15], M.xyz32(sheet.queries).astype(np.float64)[ok])  # the BASE point
    assert np.all(w[~ok] == 0.0) and np.all(rec[~ok] == 0.0)
    if sheet.ktype == M.BLOB:
        assert np.all(w[ok] == 1.0)
    for status, least in (sheet.shares or {}).items():
        assert (st == status).sum() >= least, (status, int((st == status).sum()))


@pytest.mark.parametrize("sheet", PLAIN, **IDS)
def test_plain_reference_keeps_what_the_oracle_keeps(sheet, O):
    st, _, rec, _ = M.oracle_match(sheet, O)
    x = M.xyz32(sheet.target).astype(np.float64)
    seen = 0
    for i, h in enumerate(sheet.hoods):
        if not h.plain:
            continue
        kept, pre, _ = M.evaluate(sheet, i)
        if pre != M.SUCCESS:
            assert st[i] == pre, (h.label, i, int(st[i]), pre)
            continue
        assert st[i] not in (M.BAD_PARAM, M.NOT_ENOUGH, M.TOO_FAR), (h.label, i, int(st[i]))
        if st[i] == M.SUCCESS:
            assert np.abs(rec[i, 9:12] - x[kept].mean(0)).max() <= 1e-9, (h.label, i, rec[i, 9:12], x[kept].mean(0))
            seen += 1
    assert seen > 0 or M.SUCCESS not in sheet.declares


@pytest.mark.parametrize("sheet", ROBUST, **IDS)
def test_plain_status_behind_the_pca_on_robust_cases(sheet, O):
    st = M.oracle_match(sheet, O)[0]
    for i in np.flatnonzero(sheet.robust):
        assert M.plain_status(sheet.ktype, sheet.mp, M.evaluate(sheet, i)[2]) == st[i], (sheet.hoods[i].label, int(st[i]))


def flips(seq):
    return sum(a != b for a, b in zip(seq[:-1], seq[1:]))


@pytest.mark.parametrize("sheet", LADDERS, **IDS)
def test_ladder_flips_exactly_once(sheet, O):
    st, w, _, _ = M.oracle_match(sheet, O)
    for name, (what, rungs) in sheet.ladders.items():
        if what == "status":
            seq = st[rungs].tolist()
            assert flips(seq) == 1 and seq[0] != seq[-1] and set(seq) == set(sheet.declares), (name, seq)
            robust = sheet.robust[rungs]
            assert robust[0] and robust[-1], name  # both ends are held to the plain status as well
        else:
            rungs = [r for r in rungs if st[r] == M.SUCCESS]
            seq = (w[rungs] == 1.0).tolist()
            assert flips(seq) == 1 and seq[0] and not seq[-1], (name, w[rungs].tolist())  # exactly 1.0 below the switch, never above it
            assert np.all((w[rungs] > 0.0) & (w[rungs] <= 1.0))


def test_families_reach_their_statuses_for_every_type(O):
    got = {}
    for s in M.SHEETS:
        got.setdefault(s.family, {}).setdefault(s.ktype, set()).update(M.oracle_match(s, O)[0].tolist())
    assert got == M.FAMILY_STATUSES
    per_type = {t: set().union(*[f.get(t, set()) for f in got.values()]) for t in (M.EDGE, M.PLANE, M.BLOB)}
    assert per_type == M.REACHABLE  # every status but INVALID_NUMERICAL and UNKOWN, for every type that can reach it
    single = {bool(s.mp.single_edge_per_ring) for s in M.SHEETS if s.ktype == M.EDGE}
    assert single == {False, True}


def test_rounding_decides_the_rounding_sheets(O):
    """the same flat clusters give both verdicts, and an axis-aligned copy at the origin is always rejected"""
    st = M.oracle_match(M.BY_NAME["rounding_blob_coplanar_k10"], O)[0]
    assert (st == M.SUCCESS).sum() >= 8 and (st == M.BAD_PCA).sum() >= 8 and (st == M.SUCCESS).sum() + (st == M.BAD_PCA).sum() == 64
    st = M.oracle_match(M.BY_NAME["rounding_blob_collinear_k10"], O)[0]
    assert (st == M.SUCCESS).sum() >= 4 and (st == M.BAD_PCA).sum() >= 4
    for k in (4, 10, 16):
        for shape in ("coplanar", "collinear", "coincident"):
            assert M.oracle_match(M.BY_NAME[f"blob_{shape}_k{k}@origin"], O)[0].tolist() == [M.BAD_PCA]


def test_sheets_keep_their_limits_and_select_every_compiled_length():
    for s in M.SHEETS:
        assert s.target.size <= 2048 and 1 <= s.nq <= 128 and s.nq == len(s.hoods) == s.first.size
        c = M.xyz32(s.target).astype(np.float64)
        centre = np.rint(c / M.STEP) * M.STEP
        assert np.all(np.abs(centre) <= 256.0) and np.all(np.abs(c - centre) <= 8.5)
        assert np.all(np.isfinite(c))
    valid = [s for s in M.SHEETS if s.family != "bad_parameters"]
    assert {K.compiled_lengths(s.ktype, s.k) for s in valid} == {(8, 5, 0), (10, 5, 0), (16, 5, 16), (16, 8, 16), (16, 16, 16)}
    for family, ks in (("ring_table", {2, 8, 10, 16}), ("ransac_table", {2, 5, 10, 16}), ("ladder_planarity", {3, 5, 8, 16}), ("blob_structure", {4, 10, 16})):
        assert {s.k for s in M.SHEETS if s.family == family} == ks


def test_lattice_cases_sit_at_the_origin_and_far_from_it():
    where = {}
    for s in M.SHEETS:
        for i, h in enumerate(s.hoods):
            if h.lattice and s.family in ("ring_table", "border", "ransac_table") and s.count[i] > 1:
                centre = np.rint(s.world[i].astype(np.float64) / M.STEP) * M.STEP
                where.setdefault((s.name.split("@")[0], h.label), []).append(np.abs(centre).max())
    assert where
    for key, c in where.items():
        assert min(c) == 0.0 and sum(v >= 192.0 for v in c) >= 2, key


def test_sheet_construction_is_deterministic():
    again = M.build_sheets()
    assert [s.name for s in again] == [s.name for s in M.SHEETS]
    for a, b in zip(again, M.SHEETS):
        assert a.target.tobytes() == b.target.tobytes() and a.queries.tobytes() == b.queries.tobytes() and bytes(a.mp) == bytes(b.mp)
        assert np.array_equal(a.robust, b.robust)


def test_filters_of_the_plain_reference_on_hand_worked_lists():
    """the per-ring table by hand: closest ring 20; 16 and 24 in, 15 and 25 out, a ring seen earlier out, a ring whose first
    copy was dropped stays out"""
    assert M.per_ring_filter(M.RING_ROWS[16][0][1]) == [2, 3, 8, 11, 13, 15]
    assert M.per_ring_filter(M.RING_ROWS[16][1][1]) == [1, 4, 8, 11, 12, 14]
    assert M.per_ring_filter(M.RING_ROWS[10][0][1]) == [2, 3, 8] and M.per_ring_filter(M.RING_ROWS[8][1][1]) == [2, 4]
    assert M.per_ring_filter([20, 20, 20]) == [] and M.per_ring_filter([]) == [] and M.per_ring_filter([20, 24]) == [1] and M.per_ring_filter([20, 25]) == []
    # RANSAC: strict bound; the first of equal hypotheses; a zero direction is supported by everything
    line = np.array([[0, 0, 0], [1, 0, 0], [2, 0.25, 0], [3, 0, 0]], np.float32)
    assert M.ransac_filter(line, 0.25) == [0, 1, 3]
    line[2, 1] = np.nextafter(np.float32(0.25), np.float32(0))
    assert M.ransac_filter(line, 0.25) == [0, 1, 2, 3]
    cross = np.array([[0, 0, 0], [1, 0, 0], [0, 1.5, 0], [2, 0, 0], [0, 2.5, 0]], np.float32)
    assert M.ransac_filter(cross, 0.25) == [0, 1, 3] and M.ransac_filter(cross[:, [1, 0, 2]], 0.25) == [0, 1, 3]
    assert M.ransac_filter(cross[[0, 2, 1, 4, 3]], 0.25) == [0, 1, 3]
    dup = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [1, 2, 0]], np.float32)
    assert M.ransac_filter(dup, 0.25) == [0, 1, 2, 3]
    assert M.ransac_filter(dup[:1], 0.25) == []
