"""Cases for the dense map's re-projection under a corrected trajectory (DenseMapHost.reproject in lidarslam_amd/_dense_map.py;
lsa_dense_map_reproject in lidarslam_amd/csrc/lsa_dense_reproject.hip).  Needs neither a GPU nor the native library.

As in tests/dense_map_cases.py every coordinate is a multiple of 0.125 and the leaf is 0.5; the translations are multiples of
0.125 too, so that wherever a case must be exact it is exact: a moved coordinate is the sum of two such numbers, and every
quotient by the leaf is exact.

A case is (calls, corrections, first_frame): the calls build the map, corrections is (n, 16) float64 with entry j for ordinal
first_frame + j.  A correction need not be rigid for the definition to hold -- it is arithmetic on twelve numbers -- and
`collapse` uses one that is not, to bring thousands of voxels to one key."""
import numpy as np

import dense_map_cases as K

LEAF, STEP = K.LEAF, K.STEP
cloud = K.cloud


def identity(n=1):
    return np.tile(np.eye(4).reshape(1, 16), (n, 1))


def translation(tx=0.0, ty=0.0, tz=0.0):
    T = np.eye(4)
    T[:3, 3] = (tx, ty, tz)
    return T.reshape(1, 16)


def translations(rows):
    return np.concatenate([translation(*r) for r in rows])


def quarter_turn_z(tx=0.0, ty=0.0, tz=0.0):
    T = np.eye(4)
    T[:2, :2] = [[0.0, -1.0], [1.0, 0.0]]
    T[:3, 3] = (tx, ty, tz)
    return T.reshape(1, 16)


def small_rotation(f):
    """a rotation of about a degree about a tilted axis and a few centimetres: nothing about it is exact"""
    a = 0.017 + 0.003 * f
    axis = np.array([0.3, -0.2, 0.93])
    axis /= np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * (Kx @ Kx)
    T[:3, 3] = (0.031 + 0.01 * f, -0.017, 0.004 * f)
    return T.reshape(1, 16)


def move(points, correction):
    """the points under one correction, by the definition's arithmetic: double, products summed left to right, narrowed"""
    T = np.asarray(correction, np.float64).reshape(16)
    out = points.copy()
    x, y, z = (points[a].astype(np.float64) for a in ("x", "y", "z"))
    with np.errstate(over="ignore", invalid="ignore"):
        for row, a in enumerate(("x", "y", "z")):
            out[a] = (((T[4 * row] * x + T[4 * row + 1] * y) + T[4 * row + 2] * z) + T[4 * row + 3]).astype(np.float32)
    return out


# ---- the merge rule on hand-written voxels ---------------------------------------------------------------------------------------
# Voxel A is (0, 0, 0) and keeps its point of ordinal 0 or 2 (identity); voxel B is (1, 0, 0), holds a point of ordinal 1, and
# correction 1 moves it one leaf down x, onto A.
def _onto_a(n=3):
    D = identity(n)
    D[1] = translation(-LEAF)
    return D


def merge_counts():
    """count adds up, first_frame is the min, last_frame the max; frames: 1 + 1 under a span of 6, the cap does not bind"""
    a = cloud([[0.125, 0.0, 0.0]] * 3, intensity=[5, 9, 1])  # ordinal 0: count 3
    b = cloud([[0.625, 0.125, 0.0]] * 2, intensity=[4, 3], first_index=10)  # ordinal 1: count 2
    c = cloud([[0.75, 0.25, 0.0]], intensity=[2], first_index=20)  # ordinal 5, voxel B again: count 3, frames 2, last 5
    D = identity(6)
    D[1] = translation(-LEAF)
    return [(a, 0), (b, 1), (c, 5)], D, 0


def merge_frames_cap_binds():
    """both voxels were seen in ordinals 0, 1 and 2: 3 + 3 frames under a span of 3 are 3"""
    calls = []
    for f in range(3):
        a = cloud([[0.125, 0.0, 0.0]], intensity=[9 - f], first_index=10 * f)  # A keeps ordinal 0's
        b = cloud([[0.625, 0.0, 0.125]], intensity=[1 if f != 1 else 7], first_index=10 * f + 5)  # B takes ordinal 1's
        calls.append((np.concatenate([a, b]), f))
    return calls, _onto_a(), 0


def merge_intensity():
    """the larger intensity gives the point and the source, the later frame's here"""
    a = cloud([[0.125, 0.0, 0.0]], intensity=[4])
    b = cloud([[0.625, 0.25, 0.375]], intensity=[6], first_index=10)
    return [(a, 0), (b, 1)], _onto_a(), 0


def merge_source_tie():
    """equal intensities: the smaller source keeps the voxel -- A's point is of ordinal 2 here, B's of ordinal 1"""
    a0 = cloud([[0.125, 0.0, 0.0]], intensity=[3])
    b = cloud([[0.625, 0.25, 0.375]], intensity=[6], first_index=10)
    a2 = cloud([[0.25, 0.125, 0.0]], intensity=[6], first_index=20)  # replaces A's point: source 2
    return [(a0, 0), (b, 1), (a2, 2)], _onto_a(), 0


def merge_signed_source_tie():
    """sources are compared as signed numbers: ordinal -1 is the smaller one, not the larger"""
    b = cloud([[0.625, 0.25, 0.375]], intensity=[6], first_index=10)  # ordinal -1, moved by entry 0
    a = cloud([[0.125, 0.0, 0.0]], intensity=[6])  # ordinal 1, entry 2
    D = identity(3)
    D[0] = translation(-LEAF)
    return [(b, -1), (a, 1)], D, -1


def merge_key_tie():
    """equal intensity and one source: an eighth of a metre up every axis brings the last lattice place below a face and the
    face itself into one voxel, from two old voxels; the smaller old key keeps it -- along x, along y, along z"""
    xyz = [[0.375, 0.0, 0.0], [0.5, 0.0, 0.0],          # voxels (0,0,0) and (1,0,0) -> (1,0,0)
           [4.0, 0.875, 0.0], [4.0, 1.0, 0.0],          # (8,1,0) and (8,2,0) -> (8,2,0)
           [-3.0, -3.0, -0.125], [-3.0, -3.0, 0.0]]     # (-6,-6,-1) and (-6,-6,0) -> (-6,-6,0)
    pts = cloud(xyz, intensity=[7] * 6)
    return [(pts[::-1].copy(), 0)], translation(STEP, STEP, STEP), 0


def clamp_below_and_above():
    """ordinals 0..4 under two corrections that begin at ordinal 2: 0, 1 and 2 take entry 0; 3 and 4 take entry 1"""
    calls = [(cloud([[2.0 * f, 0.125 * f, 0.0], [2.0 * f, 1.0, -1.0]], intensity=[f, f + 1], first_index=10 * f), f) for f in range(5)]
    return calls, translations([(0.0, LEAF, 0.0), (0.0, 0.0, -3 * LEAF)]), 2


def drops():
    """ordinal 0 is moved by 3e38 m and loses both its voxels; ordinal 1 goes one leaf up x, which takes the voxel at the index
    edge out of the range and keeps the other"""
    edge = float(1 << 20) * LEAF
    a = cloud([[0.125, 0.0, 0.0], [-7.0, 2.0, 0.5]], intensity=[1, 2])
    b = cloud([[edge - STEP, 1.0, 0.0], [3.125, 1.0, 0.0]], intensity=[3, 4], first_index=10)
    return [(a, 0), (b, 1)], translations([(3e38, 0.0, 0.0), (LEAF, 0.0, 0.0)]), 0


DROPPED = {"drops": 3}


def frames_of(points, nframes):
    """the points dealt to nframes calls, ordinals 0 .. nframes - 1"""
    return [(points[f::nframes].copy(), f) for f in range(nframes)]


def per_frame_translations(nframes):
    """frame f goes f leaves up x and an eighth of a metre times f down z: keys shift, voxels of different frames merge"""
    return translations([(f * LEAF, 0.0, -f * STEP) for f in range(nframes)])


def sized(n):
    """n distinct voxels over three frames under a translation per frame"""
    return frames_of(K.distinct_voxels(n, seed=31), 3), per_frame_translations(3), 0


def collapse(n=4097):
    """n voxels of two frames brought to ONE key by a correction with a zero matrix (contention on one slot); intensities from
    a small set, so the point is settled by source and then by old key among hundreds of ties"""
    pts = K.distinct_voxels(n, seed=41)
    pts["intensity"] = (np.arange(n) % 5).astype(np.float32)
    D = np.zeros((2, 16))
    D[:, 15] = 1.0
    D[:, [3, 7, 11]] = (0.125, -0.25, 1.0)
    return frames_of(pts, 2), D, 0


def single_point_voxels(n=4097, nframes=5):
    """-> (frames, corrections): n voxels that each hold one point of one of nframes frames, every intensity distinct; frame f
    goes f whole leaves up x, so that voxels of one frame never meet and voxels of different frames do"""
    pts = K.distinct_voxels(n, seed=53)
    pts["intensity"] = np.random.default_rng(7).permutation(n).astype(np.float32)
    return frames_of(pts, nframes), translations([(f * LEAF, 0.0, 0.0) for f in range(nframes)])


def _with(case, corrections, first_frame=0):
    return lambda: (K.PROPERTY_CASES[case](), corrections, first_frame)


# every case by name: (calls, corrections, first_frame)
CASES = {
    "merge_counts": merge_counts, "merge_cap_binds": merge_frames_cap_binds, "merge_intensity": merge_intensity, "merge_source": merge_source_tie,
    "merge_signed_source": merge_signed_source_tie, "merge_key": merge_key_tie, "clamp": clamp_below_and_above, "drops": drops,
    "identity_ties": _with("ties", identity(2)), "identity_nan": _with("nan", identity(4)), "identity_signed_zero": _with("signed_zero", identity(2)),
    "identity_ordinal": _with("ordinal", identity(3), 4), "identity_faces": _with("faces", identity()), "identity_wall": _with("wall", identity(8)),
    "identity_negative": _with("negative", identity()), "one_leaf_wall": _with("wall", translation(LEAF, -LEAF, 2 * LEAF)),
    "one_leaf_ties": _with("ties", translation(LEAF, -LEAF, 2 * LEAF)), "skipping": _with("skipping", translation(-LEAF)),
    "quarter_turn": lambda: (frames_of(K.distinct_voxels(4097, seed=61), 3), np.concatenate([quarter_turn_z(), quarter_turn_z(LEAF, 0.0, STEP), identity()]), 0),
    "quarter_turn_wall": _with("wall", quarter_turn_z(STEP, -STEP, 0.0)),
    "collapse": collapse,
    "rebuild": lambda: (single_point_voxels()[0], single_point_voxels()[1], 0),
}
# cases in which no coordinate is -0.0, so that the identity keeps every byte
IDENTITY_KEEPS = ("identity_ties", "identity_nan", "identity_signed_zero", "identity_ordinal", "identity_faces", "identity_wall")


def reprojected_host(DenseMapHost, case, leaf=LEAF):
    """-> (host map after the case's re-projection, what reproject returned)"""
    calls, D, first = case
    h = K.host_map(DenseMapHost, calls, leaf)
    return h, h.reproject(D, first)


def state(h, min_frames=1):
    """the bytes a map is compared by: points, records, sources"""
    pts, vox = h.get(min_frames)
    return pts.tobytes(), vox.tobytes(), np.ascontiguousarray(h.sources(min_frames), np.int32).tobytes()
