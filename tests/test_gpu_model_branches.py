"""The match model fit on every branch and in every form (tests/model_cases.py, held to what they declare by
tests/test_model_cases_reference.py): the staged form (fit_model behind k_model<8|16, TYPE>), the two-launch form (fit_model
behind k_model_all) and the one-launch form (group_stage + finish_model of lsa_match_fused.hip) give the oracle's status,
histogram, weights and records as bit patterns on every sheet.

The staged and the two-launch form leave their neighbour lists in memory (lsa_download_knn): they must be the cluster's
candidates in designed order, so a failing sheet tells a search fault (lists differ) from a fit fault (lists equal, records
differ).  A count of -1 (planes and blobs) says that the search proved the k-th neighbour beyond the rejection distance; it
is accepted only where the oracle says NEIGHBORS_TOO_FAR.

Positions: in the one-launch form a keypoint's group of 8 lanes sits at one of 8 positions in its wavefront and shifts its
ballots by that position, so every sheet runs with its query order rotated by 0 .. 7 (the other forms: 0 and 3) and is
compared per query.  Ragged launches -- 1, 31, 32 and 33 queries, where the last workgroup's inactive groups run the
filters on whatever LDS holds -- repeat the queries of three table sheets to those counts."""
import numpy as np
import pytest

import knn_cases as K
import model_cases as M
from conftest import bits

pytestmark = pytest.mark.gpu

STAGED, ONE_LAUNCH, TWO_LAUNCH = 0, 1, 2
FORM_NAME = {STAGED: "staged", ONE_LAUNCH: "one-launch", TWO_LAUNCH: "two-launch"}
ROTATIONS = {STAGED: (0, 3), TWO_LAUNCH: (0, 3), ONE_LAUNCH: tuple(range(8))}


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    yield c
    c.close()


def match(ctx, L, sheet, form, perm):
    """the sheet's queries perm[0], perm[1], ... matched in one form against the target that is set"""
    t = sheet.ktype
    ctx.set_fused_match(form)
    ctx.set_keypoints(L.SET_WORKING, t, sheet.queries[perm])
    hist = ctx.match(t, L.SET_WORKING, sheet.mp, sheet.pose)
    st, w, rec = ctx.match_results(t, L.SET_WORKING)
    idx, _, cnt = ctx.knn_lists(t, capacity=perm.size)
    return dict(hist=hist, st=st, w=w, rec=rec, idx=idx, cnt=cnt)


def assert_equals_oracle(sheet, r, ref, perm, what):
    st, w, rec = ref[0][perm], ref[1][perm], ref[2][perm]
    bad = np.flatnonzero(r["st"] != st)
    assert bad.size == 0, f"{sheet.name}, {what}: status differs for {[(sheet.hoods[perm[i]].label, int(r['st'][i]), int(st[i])) for i in bad[:6]]}"
    assert r["hist"].tolist() == np.bincount(st, minlength=8).tolist(), (sheet.name, what)
    bad = np.flatnonzero((bits(r["w"]) != bits(w)) | np.any(bits(r["rec"]) != bits(rec), axis=1))
    assert bad.size == 0, f"{sheet.name}, {what}: weights or records differ for {[(sheet.hoods[perm[i]].label, int(perm[i])) for i in bad[:6]]}"


def assert_lists(sheet, r, ref, perm, what):
    """the lists are the designed candidates, in designed order"""
    if sheet.family == "bad_parameters":
        return  # not searched
    assert r["idx"].shape[0] == perm.size, (sheet.name, what)
    far = r["cnt"] == -1
    assert np.all(ref[0][perm][far] == M.TOO_FAR) and (sheet.ktype != M.EDGE or not far.any()), (sheet.name, what)
    for p in np.flatnonzero(~far):
        want = sheet.candidates(perm[p])[:sheet.k]
        assert r["cnt"][p] in (want.size, -2), (sheet.name, what, sheet.hoods[perm[p]].label, int(r["cnt"][p]))
        assert r["idx"][p, :want.size].tolist() == want.tolist(), f"{sheet.name}, {what}: the SEARCH differs at {sheet.hoods[perm[p]].label}"


def check_forms(ctx, L, O, sheet, perms):
    ref = M.oracle_match(sheet, O)
    ctx.set_target(sheet.ktype, sheet.target, cell=1.0)
    out = {}
    for form in (STAGED, TWO_LAUNCH, ONE_LAUNCH):
        for tag, perm in perms(form):
            what = f"{FORM_NAME[form]} form, {tag}"
            r = match(ctx, L, sheet, form, perm)
            if form == ONE_LAUNCH:
                assert r["idx"].shape[0] == 0  # by design: the lists never leave the chip
            else:
                assert_lists(sheet, r, ref, perm, what)
            assert_equals_oracle(sheet, r, ref, perm, what)
            out[form] = r
    return out


def rotations(sheet):
    def perms(form):
        seen = set()
        for r in ROTATIONS[form]:
            if r % sheet.nq not in seen:  # query j at position (j + r) mod nq
                seen.add(r % sheet.nq)
                yield f"rotated by {r}", np.roll(np.arange(sheet.nq), r)
    return perms


@pytest.mark.parametrize("sheet", M.SHEETS, ids=lambda s: s.name)
def test_fit_equals_oracle_in_every_form_at_every_position(ctx, L, O, sheet):
    out = check_forms(ctx, L, O, sheet, rotations(sheet))
    # the rejected counts sit in the statuses the sheet declares, and reach every one the oracle reaches
    reached = set(M.oracle_match(sheet, O)[0].tolist())
    for r in out.values():
        assert reached == set(np.flatnonzero(r["hist"]).tolist()) <= set(sheet.declares)


@pytest.mark.parametrize("name", ["ring_table_k8_min2", "ring_table_k16_min6", "ransac_table_k10"])
def test_ragged_last_workgroup(ctx, L, O, name):
    """1, 31, 32, 33 queries: groups without a keypoint run beside groups with one"""
    sheet = M.BY_NAME[name]
    check_forms(ctx, L, O, sheet, lambda form: ((f"{n} queries", np.arange(n) % sheet.nq) for n in (1, 31, 32, 33)))


def test_every_compiled_list_length_is_reached():
    """single-type lsa_match selects <KE, KP, KB> from the type and its k: the sheets' k cover all five instantiations"""
    valid = [s for s in M.SHEETS if s.family != "bad_parameters"]
    assert {K.compiled_lengths(s.ktype, s.k) for s in valid} == {(8, 5, 0), (10, 5, 0), (16, 5, 16), (16, 8, 16), (16, 16, 16)}
    for lengths in [(8, 5, 0), (10, 5, 0), (16, 5, 16)]:
        assert {bool(s.mp.single_edge_per_ring) for s in valid if s.ktype == M.EDGE and K.compiled_lengths(s.ktype, s.k) == lengths} == {False, True}, lengths
    for lengths in [(8, 5, 0), (16, 8, 16), (16, 16, 16)]:
        assert {s.family for s in valid if s.ktype == M.PLANE and K.compiled_lengths(s.ktype, s.k) == lengths} >= {"ladder_model_error", "ladder_planarity"}, lengths


@pytest.mark.parametrize("plane", ["ladder_plane_saddle_k5", "ladder_plane_saddle_k8", "ladder_plane_saddle_k16"])
def test_mixed_launch_equals_single_type_runs(ctx, L, O, plane):
    """edges (k = 8), planes and blobs (k = 10) in one lsa_match_types launch: the edges' lists live in KMAX = 16, two
    candidates per lane with the second pass empty; planes of 5, 8 and 16 select <16,5,16>, <16,8,16> and <16,16,16>"""
    sheets = {M.EDGE: M.BY_NAME["ring_table_k8_min2"], M.PLANE: M.BY_NAME[plane], M.BLOB: M.BY_NAME["rounding_blob_coplanar_k10"]}
    mp = M.mixed_params(sheets[M.EDGE], sheets[M.PLANE], sheets[M.BLOB])
    for form in (ONE_LAUNCH, TWO_LAUNCH):
        single = {}
        for t, s in sheets.items():
            ctx.set_target(t, s.target, cell=1.0)
            single[t] = match(ctx, L, s, form, np.arange(s.nq))
        ctx.set_fused_match(form)
        for t, s in sheets.items():
            ctx.set_keypoints(L.SET_WORKING, t, s.queries)
        hist = ctx.match_types(7, L.SET_WORKING, mp, np.eye(4))
        for t, s in sheets.items():
            st, w, rec = ctx.match_results(t, L.SET_WORKING)
            r = dict(hist=hist[t], st=st, w=w, rec=rec)
            what = f"{FORM_NAME[form]} form, mixed launch"
            assert_equals_oracle(s, r, M.oracle_match(s, O), np.arange(s.nq), what)
            a = single[t]
            assert a["hist"].tolist() == r["hist"].tolist() and np.array_equal(a["st"], st), (s.name, what)
            assert np.array_equal(bits(a["w"]), bits(w)) and np.array_equal(bits(a["rec"]), bits(rec)), (s.name, what)
    for t in sheets:
        ctx.set_keypoints(L.SET_WORKING, t, sheets[t].queries[:0])
