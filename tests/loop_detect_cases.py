"""What the host and the device tests of loop detection over a log share (test_loop_detect_host.py, test_gpu_loop_detect.py):
descriptor tables, trajectories, the parameter grid, and the definition written out as a Python loop over L.place_distance and
L.place_select."""
import itertools

import numpy as np

SHAPES = [(1, 1), (3, 7), (20, 60)]
TABLES = ["random", "identical", "turned", "empty"]
TRAJECTORIES = ["forward_back", "stationary", "square"]


def descriptors(kind, n, rings, sectors, seed=5):
    """(n, rings * sectors + sectors) float32: cells in [0, 4), then the column norms"""
    rng = np.random.default_rng(seed + 31 * rings + sectors)

    def with_norms(cells):
        cells = cells.astype(np.float32)
        return np.concatenate([cells.reshape(-1), np.sqrt((cells * cells).sum(axis=0, dtype=np.float32)).astype(np.float32)])

    base = rng.uniform(0.0, 4.0, (rings, sectors)) * (rng.uniform(0, 1, (rings, sectors)) < 0.8)
    out = []
    for i in range(n):
        if kind == "random":
            cells = rng.uniform(0.0, 4.0, (rings, sectors)) * (rng.uniform(0, 1, (rings, sectors)) < 0.8)
        elif kind == "identical":  # every distance ties: the lower index wins
            cells = base
        elif kind == "turned":  # frame i is the base turned by i columns; a little noise so that the distances differ
            cells = np.roll(base, i, axis=1) + (rng.uniform(0, 0.05, (rings, sectors)) if i % 3 else 0.0)
        else:  # two frames in three are empty
            cells = base + rng.uniform(0, 0.5, (rings, sectors)) if i % 3 == 0 else np.zeros((rings, sectors))
        out.append(with_norms(cells))
    return np.stack(out)


def trajectory(kind, n):
    """poses (n, 4, 4) and times (n,)"""
    xyz = np.zeros((n, 3))
    half = max(n // 2, 1)
    for i in range(n):
        if kind == "forward_back":  # out along x, back over the same track, a little beside it
            xyz[i] = [i, 0.0, 0.0] if i < half else [2 * half - 1 - i, 0.25, 0.0]
        elif kind == "stationary":  # moves, stands still for a third of the log (equal travelled), moves back
            a, b = n // 3, 2 * n // 3
            xyz[i] = [i, 0, 0] if i < a else ([a - 1, 0, 0] if i < b else [a - 1 - (i - b + 1) * 0.5, 0.1, 0])
        else:  # a closed square of four equal sides
            side = max(n // 4, 1)
            leg, at = min(i // side, 3), i - min(i // side, 3) * side
            corner = [(0, 0), (side, 0), (side, side), (0, side)][leg]
            step = [(1, 0), (0, 1), (-1, 0), (0, -1)][leg]
            xyz[i] = [corner[0] + step[0] * at, corner[1] + step[1] * at, 0.01 * i]
    P = np.tile(np.eye(4), (n, 1, 1))
    P[:, :3, 3] = xyz
    return P, 0.1 * np.arange(n)


def grid(n, points=24):
    """`points` parameter sets that between them use every value of every parameter"""
    strides = [1, 3, n + 2]
    ranges = [(0, -1), (0, n - 1), (n // 3, max(n - 2, n // 3))]
    min_travelled = [0.0, 3.0]
    max_distance = [0.0, 2.5]
    max_descriptor_distance = [0.0, 0.3]
    windows = [0, 2, n + 5]
    per_query = [1, 3, 16]
    every = list(itertools.product(strides, ranges, min_travelled, max_distance, max_descriptor_distance, windows, per_query))
    step = 131  # coprime to len(every) = 648: a walk through all of it
    for k in range(points):
        s, (first, last), mt, md, mdd, w, pq = every[(k * step + 7 * (k // 5)) % len(every)]
        yield dict(first_query=first, last_query=last, query_stride=s, per_query=pq, min_travelled=mt, max_distance=md, max_descriptor_distance=mdd,
                   exclusion_half_window=w)


def distance_table(L, D, rings, sectors):
    """table[q] = (distance (q,), shift (q,)) of frame q against the frames before it, by L.place_distance"""
    table = []
    for q in range(D.shape[0]):
        pairs = [L.place_distance(D[q], D[i], rings=rings, sectors=sectors) for i in range(q)]
        table.append((np.array([d for d, _ in pairs], np.float32), np.array([s for _, s in pairs], np.int32)))
    return table


def by_definition(L, table, P, t, sectors, first_query, last_query, query_stride, per_query, **search):
    """[(query, frame, distance, shift, yaw)] and the number of candidates of every query"""
    n = P.shape[0]
    last = n - 1 if last_query < 0 else last_query
    out, counts = [], []
    for q in range(first_query, last + 1, query_stride):
        got = L.place_select(table[q][0], table[q][1], P, t, q, sectors=sectors, capacity=per_query, **search)
        out += [(q,) + c for c in got]
        counts.append(len(got))
    return out, counts
