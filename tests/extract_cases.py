"""Cases for the keypoint extraction (lsa_extract.hip) at the shapes its kernels branch on, and the plain reference the
labelling is held to.  Needs neither a GPU nor the oracle.

Layer 1, the labelling alone (k_label through lsa_selftest_labels; the oracle's SetKeyPointsLabels through
Extractor.label): `greedy_labels` restates SetKeyPointsLabels (SpinningSensorKeypointExtractor.cxx:474-590) for one ring
with a sort and a walk, which is what the reference does and what the kernel avoids.  The cases put rings at the lengths
where k_label changes its chunk size PER (points per thread: 1 up to 1024 points, 2 up to 2048, 4 up to 4096, 8 up to
8192), at lengths that are no multiple of PER, and fill them with scores that tie, chain and sit on the thresholds.

Domain limit: the scores are what k_curvature can produce -- every one is a norm, a square or a fabsf: non-negative,
finite or +inf, never NaN, never -0.0.  The kernel orders -0.0 below +0.0 (it compares bit patterns) while the reference
compares them equal, so -0.0 is outside the domain and is not a case.

Layer 2, whole frames: `scene_frame` makes a scan of chosen ring lengths (a room with corners, a free-standing plate and
striped intensities), `frame_cases` the frames whose sizes the ring bucketing (chunks of 1024 points, a quarter of a chunk
per wavefront, batches of 64) and the compaction branch on."""
from dataclasses import dataclass, field

import numpy as np

from lidarslam_amd._native import POINT_DTYPE, ExtractParams

LABEL_THREADS = 1024    # kLabelThreads: one block per ring
MAX_RING_POINTS = 8192  # kMaxRingPoints
MAX_RINGS = 512         # kMaxRings
PLANE_HW = 4            # the planes' window (SSKE.cxx:559-560)


def chunk_size(n):
    """PER of nms_fixed_point_any: points per thread of k_label for a ring of n points"""
    return 1 if n <= LABEL_THREADS else 2 if n <= 2 * LABEL_THREADS else 4 if n <= 4 * LABEL_THREADS else 8


def thresholds(params):
    """The five thresholds SetKeyPointsLabels compares with, as floats (SSKE.cxx:476-477: the squares are float products)"""
    f = np.float32
    return {
        "gap": f(params.edge_depth_gap_threshold) * f(params.edge_depth_gap_threshold),
        "angle": f(params.edge_sin_angle_threshold),
        "sal": f(params.edge_saliency_threshold) * f(params.edge_saliency_threshold),
        "int": f(params.edge_intensity_gap_threshold),
        "plane": f(params.plane_sin_angle_threshold),
    }


def edge_windows(W):
    """(criterion, half window) in the reference's order: depth gap, angle, saliency, intensity gap (SSKE.cxx:526-533)"""
    return [("gap", W - 1), ("angle", W), ("sal", W - 1), ("int", 1)]


def greedy_labels(scores, valid, W, thr, trace=None):
    """SetKeyPointsLabels for one ring, literally: scores = (sin_angle, depth_gap, saliency, intensity_gap), float32;
    valid = one byte per point, bit k = valid for type k (EDGE, PLANE, BLOB), taken apart into three bit arrays;
    thr = thresholds(params).  Returns (label, validity afterwards), one byte per point each.

    Per criterion one index list sorted by score descending is walked until the score drops below the threshold; a valid
    point is labelled and clears the validity within its window.  Planes walk the angle list backwards, skip
    (double)v < 1e-6, stop above the plane threshold and clear +-4.  Blobs: every third index.  Last, a labelled point's
    validity bit is set back (SSKE.cxx:584).  A ring shorter than 2W+1 gets no labels.

    The reference sorts with std::sort, which leaves the order of equal scores open.  The project's rule, stated above
    nms_word in lsa_extract.hip, is the stable one: among equal scores the smaller index comes first in the descending
    list -- so it wins among edges, and the larger index wins among planes, which walk the same list backwards.  Here:
    argsort(kind="stable") of the negated scores.

    trace, if a list, receives per pass (half window, candidates at the start of the pass, selected, priority key) for
    selection_stats."""
    arrays = dict(zip(("angle", "gap", "sal", "int"), (np.ascontiguousarray(a, np.float32) for a in scores)))
    valid = np.ascontiguousarray(valid, np.uint8)
    n = valid.size
    label = np.zeros(n, np.uint8)
    if n < 2 * W + 1:
        return label, valid.copy()
    ok = [((valid >> k) & 1).astype(bool) for k in range(3)]
    order = {name: np.argsort(-arrays[name], kind="stable") for name in arrays}

    for name, hw in edge_windows(W):
        v, t, e = arrays[name], float(thr[name]), ok[0]
        start, picked = e & (v >= thr[name]), []
        for i, s in zip(order[name].tolist(), v[order[name]].tolist()):
            if s < t:
                break
            if not e[i]:
                continue
            label[i] |= 1
            picked.append(i)
            e[max(0, i - hw):i + hw + 1] = False
        if trace is not None:
            sel = np.zeros(n, bool)
            sel[picked] = True
            trace.append((hw, start, sel, v.astype(np.float64)))

    v, t, p = arrays["angle"], float(thr["plane"]), ok[1]
    if trace is not None:
        start = p & ~(v.astype(np.float64) < 1e-6) & (v <= thr["plane"])
    back = order["angle"][::-1]
    for i, s in zip(back.tolist(), v[back].tolist()):
        if s > t:
            break
        if not p[i] or s < 1e-6:
            continue
        label[i] |= 2
        p[max(0, i - PLANE_HW):i + PLANE_HW + 1] = False
    if trace is not None:
        trace.append((PLANE_HW, start, (label & 2).astype(bool), -v.astype(np.float64)))

    label[0::3] |= ok[2][0::3].astype(np.uint8) << 2
    after = (ok[0].astype(np.uint8) | (ok[1].astype(np.uint8) << 1) | (ok[2].astype(np.uint8) << 2)) | label
    return label, after


def selection_stats(trace):
    """From greedy_labels' trace: (candidates rejected because of a selected neighbour, those of them whose score is
    bit-equal to that of the selected neighbour that suppressed them).  A candidate of a pass (above the threshold and
    valid when the pass starts) that is not selected was suppressed by a selected neighbour of its window, and the first to
    do so is the one of highest priority: the largest key among the selected points of the window."""
    rejected = ties = 0
    for hw, cand, sel, key in trace:
        rej = cand & ~sel
        if hw == 0 or not rej.any():
            continue
        k = np.where(sel, key, -np.inf)
        padded = np.concatenate([np.full(hw, -np.inf), k, np.full(hw, -np.inf)])
        best = np.lib.stride_tricks.sliding_window_view(padded, 2 * hw + 1).max(axis=1)
        assert np.all(best[rej] >= key[rej])  # a rejected candidate has a selected neighbour of at least its priority
        rejected += int(rej.sum())
        ties += int((rej & (best == key)).sum())
    return rejected, ties


# ---------------------------------------------------------------------------------------------------------------------
# layer 1: the cases
RING_LENGTHS = [63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192]  # and 2W, 2W+1, 2W+2
OTHER_WIDTH_LENGTHS = [1025, 2049, 4097, 8192]
WIDTHS = [4, 1, 5, 8]

# patterns with equal scores inside one window by construction: the tie condition of the CPU test applies to them (the
# sawteeth of period hw + 1 and 2 hw + 1 put their equal scores just out of each other's reach)
TIE_PATTERNS = {"equal", "saw_hw", "alt2", "plateaus", "alpha3", "at_thr", "inf", "denormal",
                "plane_zero", "plane_1e-6", "plane_thr", "plane_thr_ulp", "valid_all", "valid_30", "valid_runs", "valid_one_type"}
PATTERNS = ["equal", "ramp_up", "ramp_down", "saw_hw", "saw_hw1", "saw_2hw1", "alt2", "plateaus", "alpha3", "random", "below",
            "at_thr", "inf", "denormal", "plane_zero", "plane_1e-6", "plane_thr", "plane_thr_ulp", "valid_all", "valid_30",
            "valid_runs", "valid_one_type"]

F_BELOW_1E6 = np.float32(1e-6)                                   # 9.99999997e-07: below 1e-6 as a double, skipped
F_ABOVE_1E6 = np.nextafter(np.float32(1e-6), np.float32(1.0))    # the next float: not below, a plane candidate
assert float(F_BELOW_1E6) < 1e-6 <= float(F_ABOVE_1E6)


@dataclass
class LabelCase:
    name: str
    pattern: str
    W: int
    lens: np.ndarray    # ring lengths (one ring but for the multi-ring launch)
    scores: tuple       # sin_angle, depth_gap, saliency, intensity_gap: float32, the rings one after the other
    valid: np.ndarray   # uint8
    params: ExtractParams = field(default_factory=ExtractParams)

    @property
    def n(self):
        return int(self.lens.sum())

    def rings(self):
        """(ring, first point, length) of every ring"""
        start = np.concatenate([[0], np.cumsum(self.lens)])
        return [(r, int(start[r]), int(self.lens[r])) for r in range(self.lens.size)]


def _edge_scores(u, thr):
    """levels u in [0, 1] -> scores in [thr / 2, 3 thr]: equal levels give bit-equal scores; candidates from u = 0.2 on (a
    criterion that takes every point leaves nothing to the ones behind it)"""
    return np.float32(thr) * (0.5 + 2.5 * np.asarray(u, np.float64)).astype(np.float32)


def _angle_scores(u):
    """levels u in [0, 1] -> sin angles in [0.05, 1]: plane candidates below u = 0.47, edge candidates above 0.853"""
    return (0.05 + 0.95 * np.asarray(u, np.float64)).astype(np.float32)


def _saw(n, p):
    i = np.arange(n)
    return np.full(n, 0.4) if p <= 1 else (i % p) / (p - 1)


def _plateau_levels(n, per, rng, low, high, base):
    """random levels in `base` with plateaus of the levels `low` / `high` in turn; plateau t starts at an anchor -- a multiple
    of 64 * PER and of PER in turn -- shifted by -1, 0, +1 and ends at a multiple of PER shifted by -1, 0, +1 (all nine
    combinations in turn), at least 24 points long (longer than every window, 2 * 8 + 1)"""
    u = rng.uniform(base[0], base[1], n)
    anchors = [a for m in range(0, n, 64 * per) for a in (m, m + 35 * per) if a < n]  # 35 * PER: a multiple of PER, not of 64 * PER
    for t, a in enumerate(anchors):
        d0, d1 = t % 3 - 1, (t // 3) % 3 - 1
        b = max(0, a + d0)
        e = min(n, a + -(-24 // per) * per + (t % 2) * per + d1)
        u[b:e] = (low, high)[t % 2]
    return u


def _validity(pattern, n, W, rng):
    if pattern == "valid_30":
        return sum(((rng.random(n) >= 0.3).astype(np.uint8) << k) for k in range(3)).astype(np.uint8)
    if pattern == "valid_runs":
        v = np.full(n, 7, np.uint8)
        for k in range(3):  # per type: invalid runs of 2W+2 .. 2W+9 points (longer than every window) every 30-odd points
            i = int(rng.integers(0, 5))
            while i < n:
                run = min(2 * max(W, PLANE_HW) + 2 + int(rng.integers(0, 8)), max(2, n // 3))  # (shorter on the shortest rings)
                v[i:i + run] &= ~np.uint8(1 << k)
                i += run + 9 + int(rng.integers(0, 12))
        return v
    if pattern == "valid_one_type":
        return (np.uint8(1) << ((np.arange(n) // min(41, max(3, n // 3))) % 3)).astype(np.uint8)  # blocks of 41 points valid as E, P, B in turn
    return np.full(n, 7, np.uint8)


def label_case(n, W, pattern, seed=0):
    """one ring of n points at NeighborWidth W"""
    rng = np.random.default_rng([n, W, PATTERNS.index(pattern), seed])
    params = ExtractParams(neighbor_width=W)
    if pattern == "denormal":  # denormal scores are candidates only at thresholds of 0
        params = ExtractParams(neighbor_width=W, edge_depth_gap_threshold=0.0, edge_saliency_threshold=0.0, edge_intensity_gap_threshold=0.0,
                               edge_sin_angle_threshold=0.0)
    thr = thresholds(params)
    names = ("gap", "sal", "int")
    hw = dict(edge_windows(W))
    i = np.arange(n)
    alpha3 = lambda: rng.choice([0.1, 0.4, 0.95], n)  # noqa: E731
    edge = {}
    if pattern == "equal":
        angle = np.full(n, 0.3, np.float32)
        edge = {c: _edge_scores(np.full(n, 0.5), thr[c]) for c in names}
    elif pattern in ("ramp_up", "ramp_down"):
        u = i / n if pattern == "ramp_up" else (n - 1 - i) / n
        angle, edge = _angle_scores(u), {c: _edge_scores(u, thr[c]) for c in names}
        for a in (angle, *edge.values()):
            assert np.all(np.diff(a) > 0) if pattern == "ramp_up" else np.all(np.diff(a) < 0)
    elif pattern in ("saw_hw", "saw_hw1", "saw_2hw1"):
        period = {"saw_hw": lambda h: h, "saw_hw1": lambda h: h + 1, "saw_2hw1": lambda h: 2 * h + 1}[pattern]
        angle, edge = _angle_scores(_saw(n, period(hw["angle"]))), {c: _edge_scores(_saw(n, period(hw[c])), thr[c]) for c in names}
    elif pattern == "alt2":
        u = np.where(i % 2 == 0, 0.2, 0.9)
        angle, edge = _angle_scores(u), {c: _edge_scores(np.roll(u, k), thr[c]) for k, c in enumerate(names)}
    elif pattern == "plateaus":
        per = chunk_size(n)
        angle = _angle_scores(_plateau_levels(n, per, rng, 0.02, 0.95, (0.2, 0.45)))
        edge = {c: _edge_scores(_plateau_levels(n, per, rng, 0.9, 0.9, (0.0, 0.5)), thr[c]) for c in names}
    elif pattern == "random":
        angle, edge = _angle_scores(rng.random(n)), {c: _edge_scores(rng.random(n), thr[c]) for c in names}
    elif pattern == "below":
        angle = (0.6 + 0.2 * rng.random(n)).astype(np.float32)  # above the plane threshold, below the edge threshold
        edge = {c: np.float32(thr[c]) * (0.1 + 0.8 * rng.random(n)).astype(np.float32) for c in names}
        assert all(np.all(edge[c] < thr[c]) for c in names) and np.all((angle > thr["plane"]) & (angle < thr["angle"]))
    elif pattern == "at_thr":
        angle = np.where((i // 7) % 2 == 0, thr["plane"], thr["angle"]).astype(np.float32)
        edge = {c: np.full(n, thr[c], np.float32) for c in names}
    elif pattern == "inf":
        pair = lambda k: np.isin(i % 11, (k, k + 1))  # noqa: E731  (+inf in adjacent pairs: ties at the top of every list)
        angle = np.where(pair(6), np.float32(np.inf), _angle_scores(rng.random(n)))
        edge = {c: np.where(pair(k), np.float32(np.inf), _edge_scores(rng.random(n), thr[c])) for c, k in zip(names, (3, 0, 8))}
    elif pattern == "denormal":
        den = lambda: rng.integers(0, 4, n).astype(np.uint32).view(np.float32)  # noqa: E731  (0 and the three smallest denormals)
        angle = np.where(rng.random(n) < 0.3, rng.choice(np.float32([0.2, 0.3]), n), den())
        edge = {c: den() for c in names}
    else:
        plane_alphabet = {
            "plane_zero": [0.0, 0.2, 0.3, 0.9],
            "plane_1e-6": [F_BELOW_1E6, F_ABOVE_1E6, 0.3, 0.9],
            "plane_thr": [thr["plane"], 0.3, 0.9],
            "plane_thr_ulp": [np.nextafter(thr["plane"], np.float32(1.0)), thr["plane"], 0.9],
        }.get(pattern)
        angle = rng.choice(np.float32(plane_alphabet), n) if plane_alphabet else _angle_scores(alpha3())
        edge = {c: _edge_scores(alpha3(), thr[c]) for c in names}
    scores = tuple(np.ascontiguousarray(a, np.float32) for a in (angle, edge["gap"], edge["sal"], edge["int"]))
    for a in scores:  # the domain k_curvature can produce
        assert not np.isnan(a).any() and np.all(a >= 0) and not np.signbit(a).any()
    return LabelCase(f"n{n}-W{W}-{pattern}", pattern, W, np.array([n], np.int32), scores, _validity(pattern, n, W, rng), params)


def multi_ring_case():
    """One launch: rings of the four chunk sizes side by side, a zero-length ring between them, a ring shorter than 2W+1, and
    the last ring at id 511 (the rings between are empty)."""
    lens = np.zeros(MAX_RINGS, np.int32)
    lens[:7] = [1023, 2049, 0, 4097, 5, 1500, 8191]
    lens[MAX_RINGS - 1] = 3000
    parts = [label_case(int(n), 4, "alpha3", seed=100 + r) for r, n in enumerate(lens) if n > 0]
    scores = tuple(np.concatenate([p.scores[k] for p in parts]) for k in range(4))
    return LabelCase("multi_ring", "alpha3", 4, lens, scores, np.concatenate([p.valid for p in parts]), ExtractParams(neighbor_width=4))


def vacuity_problems(case):
    """What makes a case vacuous, by the reference alone: a type without a labelled point, no candidate rejected because of
    a selected neighbour, and for the tie patterns no rejected candidate whose score is bit-equal to that of the selected
    neighbour that suppressed it.  (`below` and rings shorter than 2W+1 are to yield no edge and no plane at all.)"""
    trace = []
    counts = reference_labels(case, trace)[2].sum(axis=0)
    if case.pattern == "below" or case.lens.max() < 2 * case.W + 1:
        return [f"labelled: {counts.tolist()}"] if counts[0] or counts[1] else []
    rejected, ties = selection_stats(trace)
    problems = [f"no {name} labelled" for name, c in zip(("edge", "plane", "blob"), counts) if c == 0]
    if rejected == 0:
        problems.append("no candidate rejected by a selected neighbour")
    if case.pattern in TIE_PATTERNS and ties == 0:
        problems.append("no candidate rejected by a selected neighbour of bit-equal score")
    return problems


_label_cases = None


def label_cases():
    """W = 4: every length with every pattern; W = 1, 5, 8: the lengths one past each chunk size's limit and the longest
    ring with every pattern; the multi-ring launch."""
    global _label_cases
    if _label_cases is None:
        cases = []
        for W in WIDTHS:
            lengths = [2 * W, 2 * W + 1, 2 * W + 2] + RING_LENGTHS if W == 4 else OTHER_WIDTH_LENGTHS
            for n in lengths:
                for p in PATTERNS:
                    c = label_case(n, W, p)
                    # on the two or three usable points of the shortest rings a random draw is often vacuous: the first
                    # seed whose draw is not (tests/test_extract_reference.py asserts the condition for every case)
                    for seed in range(1, 200 if n <= 2 * W + 2 else 1):
                        if not vacuity_problems(c):
                            break
                        c = label_case(n, W, p, seed)
                    cases.append(c)
        cases.append(multi_ring_case())
        assert len({c.name for c in cases}) == len(cases)
        _label_cases = cases
    return _label_cases


def reference_labels(case, trace=None):
    """greedy_labels ring by ring -> (label, validity afterwards, ring_counts (rings, 3)) in the layout of lsa_selftest_labels"""
    thr = thresholds(case.params)
    label, after, counts = np.zeros(case.n, np.uint8), np.zeros(case.n, np.uint8), np.zeros((case.lens.size, 3), np.int32)
    for r, s, n in case.rings():
        if n == 0:
            continue
        l, a = greedy_labels([x[s:s + n] for x in case.scores], case.valid[s:s + n], case.W, thr, trace)
        label[s:s + n], after[s:s + n] = l, a
        counts[r] = [np.count_nonzero(l & (1 << k)) for k in range(3)]
    return label, after, counts


_references = {}


def cached_reference(case):
    """reference_labels, computed once per case and process; read-only"""
    if case.name not in _references:
        ref = reference_labels(case)
        for a in ref:
            a.setflags(write=False)
        _references[case.name] = ref
    return _references[case.name]


def label_batches():
    """The cases grouped by their parameters into launches of at most 512 rings: [(params, [case, ...]), ...]; a case with
    more than one ring is a launch of its own."""
    groups, out = {}, []
    for c in label_cases():
        if c.lens.size > 1:
            out.append((c.params, [c]))
        else:
            groups.setdefault(bytes(c.params), []).append(c)
    for cases in groups.values():
        for i in range(0, len(cases), MAX_RINGS):
            out.append((cases[i].params, cases[i:i + MAX_RINGS]))
    return out


def run_batch(label_fn, params, cases):
    """label_fn(ring_lengths, sin_angle, depth_gap, saliency, intensity_gap, valid, params) on the cases' rings in one call
    -> {case name: (label, validity afterwards, ring_counts)}"""
    lens = np.concatenate([c.lens for c in cases])
    scores = [np.concatenate([c.scores[k] for c in cases]) for k in range(4)]
    label, after, counts = label_fn(lens, *scores, np.concatenate([c.valid for c in cases]), params)
    out, p, r = {}, 0, 0
    for c in cases:
        out[c.name] = (label[p:p + c.n], after[p:p + c.n], counts[r:r + c.lens.size])
        p, r = p + c.n, r + c.lens.size
    return out


def assert_labels_equal(got, want, what):
    for name, a, b in zip(("label", "validity", "ring_counts"), got, want):
        bad = np.argwhere(np.asarray(a) != np.asarray(b))
        assert bad.size == 0, f"{what}: {name} differs at {len(bad)} places, first {bad[:5].tolist()}: {np.asarray(a)[tuple(bad[:5].T)]} against {np.asarray(b)[tuple(bad[:5].T)]}"


# ---------------------------------------------------------------------------------------------------------------------
# layer 2: whole frames
AZIMUTH_STEP = 2 * np.pi / MAX_RING_POINTS  # every ring is sampled at this step: 8192 points go once round
AZIMUTHAL_RESOLUTION = float(np.float32(AZIMUTH_STEP))  # set in the context and in the oracle's extractor alike
ROOM = np.array([(6.0, -4.0), (6.0, 5.0), (-3.0, 5.0), (-3.0, 1.0), (-7.0, 1.0), (-7.0, -4.0)])  # an L: five corners and a reflex one
PLATE_AZIMUTH, PLATE_RANGE, PLATE_HALF_WIDTH = 0.3, 2.5, 0.0135  # the free-standing post: a plate 14 points wide, facing the sensor


def _ranges(az):
    """distance from the sensor (the origin) to the nearest surface along each azimuth"""
    d = np.stack([np.cos(az), np.sin(az)], 1)
    c, s = np.cos(PLATE_AZIMUTH), np.sin(PLATE_AZIMUTH)
    mid = PLATE_RANGE * np.array([c, s])
    segments = [(ROOM[k], ROOM[(k + 1) % len(ROOM)]) for k in range(len(ROOM))]
    segments.append((mid - PLATE_HALF_WIDTH * np.array([-s, c]), mid + PLATE_HALF_WIDTH * np.array([-s, c])))
    best = np.full(az.size, np.inf)
    for P, Q in segments:
        e = Q - P
        den = d[:, 0] * e[1] - d[:, 1] * e[0]
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (P[0] * e[1] - P[1] * e[0]) / den
            u = (P[0] * d[:, 1] - P[1] * d[:, 0]) / den
        hit = (den != 0) & (t > 0) & (u >= 0) & (u <= 1)
        best = np.where(hit & (t < best), t, best)
    assert np.all(np.isfinite(best))
    return best


def scene_frame(rings, by_ring=False):
    """A frame of lsa_point_t.  rings = [(laser id, points), ...].  Every ring samples the room at AZIMUTH_STEP over a sector
    centred on the plate (8192 points: the whole turn), at an elevation of its own.  Intensities take three values in stripes
    of nine steps, so that intensity gaps tie.  Firing order: column by column, the rings of a column by id; times increase
    in that order.  by_ring: the same points delivered ring after ring."""
    parts = []
    for ring, n in rings:
        j = np.arange(n)
        col = j - (n - 1) // 2  # column 0 looks at the middle of the plate
        az = PLATE_AZIMUTH + col * AZIMUTH_STEP
        rho = _ranges(az)
        p = np.zeros(n, POINT_DTYPE)
        p["x"], p["y"] = rho * np.cos(az), rho * np.sin(az)
        p["z"] = rho * np.tan(np.deg2rad(((ring % 16) - 7.5) * 0.8))
        p["w"] = 1.0
        p["intensity"] = np.float32([10.0, 80.0, 200.0])[(np.floor_divide(col, 9)) % 3]
        p["laser_id"] = ring
        parts.append((col, p))
    cols = np.concatenate([c for c, _ in parts]) if parts else np.zeros(0, int)
    pts = np.concatenate([p for _, p in parts]) if parts else np.zeros(0, POINT_DTYPE)
    order = np.lexsort((pts["laser_id"], cols))
    pts = pts[order]
    pts["time"] = -0.1 + 0.1 * np.arange(pts.size) / max(pts.size, 1)
    if by_ring:
        pts = pts[np.argsort(pts["laser_id"], kind="stable")]
    return np.ascontiguousarray(pts)


def sixteen_rings(total):
    """`total` points on 16 rings: rings too short to be labelled (two points each) in front, the rest on the last rings
    -- four of them, or one when there are fewer than 255 points"""
    short = 12 if total >= 255 else 15
    rest, k = total - 2 * short, 16 - short
    lens = [2] * short + [rest // k + (1 if i < rest % k else 0) for i in range(k)]
    assert sum(lens) == total and len(lens) == 16
    return list(enumerate(lens))


@dataclass
class FrameCase:
    name: str
    rings: list
    by_ring: bool = False
    W: int = 4

    def frame(self):
        return scene_frame(self.rings, self.by_ring)

    def params(self):
        return ExtractParams(neighbor_width=self.W)


SINGLE_RING_LENGTHS = [1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192]
SIXTEEN_RING_TOTALS = [1023, 1024, 1025, 255, 256, 257, 64, 65]


def frame_cases():
    cases = [FrameCase(f"one_ring_{n}", [(0, n)]) for n in SINGLE_RING_LENGTHS]
    cases += [FrameCase(f"sixteen_rings_{t}", sixteen_rings(t)) for t in SIXTEEN_RING_TOTALS]
    cases += [FrameCase(f"sixteen_rings_{t}_by_ring", sixteen_rings(t), by_ring=True) for t in SIXTEEN_RING_TOTALS]
    cases += [FrameCase("sixteen_rings_of_8192", [(r, 8192) for r in range(16)]), FrameCase("sixteen_rings_of_8192_by_ring", [(r, 8192) for r in range(16)], by_ring=True)]
    cases += [FrameCase("rings_0_and_511", [(0, 1500), (MAX_RINGS - 1, 700)])]
    cases += [FrameCase("one_ring_4097_W1", [(0, 4097)], W=1), FrameCase("one_ring_4097_W8", [(0, 4097)], W=8)]
    return cases


def assert_extraction_equal(ctx, ex, O, L, pts, params=None, mask=7):
    """Extraction of pts on the device against the oracle: counts, the ten debug arrays bit for bit, the three clouds byte
    for byte.  mask: the keypoint types the context keeps (lsa_set_keypoint_types); the others come out empty."""
    from conftest import bits

    ctx.upload_frame(pts)
    counts = ctx.extract_keypoints(params)
    ref = ex.compute(pts, params)
    assert counts.tolist() == [int(ref[k]) if (mask >> k) & 1 else 0 for k in range(3)]
    for i, name in enumerate(O.DEBUG_NAMES):
        a, b = ctx.debug_array(i), ex.debug(i)
        bad = np.flatnonzero(bits(a) != bits(b))
        assert bad.size == 0, f"{name}: {bad.size} mismatches, first at {bad[:5]}: gpu {a[bad[:5]]} oracle {b[bad[:5]]}"
    for k in range(3):
        want = ex.keypoints(k) if (mask >> k) & 1 else ex.keypoints(k)[:0]
        assert ctx.keypoints(L.SET_RAW_CURRENT, k).tobytes() == want.tobytes(), f"keypoint cloud {k}"
    return counts
