"""lsa_loop_closure_candidate (host only, no device): the logged frame nearest in position to the query among those at least
min_travelled metres back along the trajectory and within max_distance -- against a brute-force statement in numpy, on random
and on looped trajectories.  The statement uses the helper's own association of the sums (sqrt(dx dx + dy dy + dz dz), steps
added front to back), so the comparison is exact, ties included."""
import numpy as np
import pytest


def poses_of(xyz):
    P = np.tile(np.eye(4), (len(xyz), 1, 1))
    P[:, :3, 3] = np.asarray(xyz, np.float64)
    return P


def dist(a, b):
    d = a - b
    return np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])


def brute(xyz, query, min_travelled, max_distance):
    xyz = np.asarray(xyz, np.float64)
    travelled = [0.0]
    for i in range(1, query + 1):
        travelled.append(travelled[-1] + dist(xyz[i], xyz[i - 1]))
    best, best_d = -1, None
    for i in range(query):
        if not travelled[query] - travelled[i] >= min_travelled:
            continue
        d = dist(xyz[i], xyz[query])
        if not d <= max_distance:
            continue
        if best < 0 or d < best_d:
            best, best_d = i, d
    return best


def candidate(L, xyz, query, min_travelled, max_distance):
    xyz = np.asarray(xyz, np.float64)
    return L.loop_closure_candidate(poses_of(xyz), 100.0 + 0.1 * np.arange(len(xyz)), query, min_travelled, max_distance)


def test_a_straight_line_has_no_candidate(L):
    xyz = [[0.5 * i, 0.0, 0.0] for i in range(40)]
    for q in (0, 1, 20, 39):
        assert candidate(L, xyz, q, 5.0, 2.0) == -1 == brute(xyz, q, 5.0, 2.0)
    # ... unless the neighbours of the query are let in
    assert candidate(L, xyz, 39, 0.0, 2.0) == 38 == brute(xyz, 39, 0.0, 2.0)


def figure_of_eight(n=81, lift=0.1):
    s = np.linspace(0.0, 2 * np.pi, n)
    return np.stack([20.0 * np.sin(s), 10.0 * np.sin(2 * s), lift * s], 1)  # passes (0, 0) at s = 0, pi and 2 pi


def test_a_figure_of_eight_gives_the_crossing(L):
    xyz = figure_of_eight()
    mid = 40  # s = pi: back at the crossing the trajectory started from
    assert np.hypot(xyz[mid][0], xyz[mid][1]) < 1e-9
    assert candidate(L, xyz, mid, 10.0, 3.0) == 0 == brute(xyz, mid, 10.0, 3.0)
    # from the end of the second lobe both earlier passes qualify: the nearer one (in height) is the second
    assert candidate(L, xyz, 80, 10.0, 3.0) == mid == brute(xyz, 80, 10.0, 3.0)
    # half-way round a lobe nothing is near
    assert candidate(L, xyz, 20, 10.0, 3.0) == -1 == brute(xyz, 20, 10.0, 3.0)
    # every query of the curve
    for q in range(len(xyz)):
        assert candidate(L, xyz, q, 10.0, 3.0) == brute(xyz, q, 10.0, 3.0), q


def test_ties_go_to_the_lower_index(L):
    # frames 1 and 3 mirror each other about the query's position; frame 2 is further away
    xyz = [[-50.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 30.0, 0.0], [0.0, -1.0, 0.0], [40.0, -1.0, 0.0], [40.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
    assert dist(np.array(xyz[1]), np.array(xyz[6])) == dist(np.array(xyz[3]), np.array(xyz[6]))
    assert candidate(L, xyz, 6, 10.0, 5.0) == 1 == brute(xyz, 6, 10.0, 5.0)
    # the same place logged twice
    xyz2 = [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [30.0, 0.0, 0.0], [0.0, 0.5, 0.0]]
    assert candidate(L, xyz2, 3, 10.0, 5.0) == 0 == brute(xyz2, 3, 10.0, 5.0)


def test_min_travelled_excludes_the_neighbours_of_the_query(L):
    xyz = figure_of_eight(lift=1.0)  # the second pass of the crossing is 3.14 m above the first, a step is 2.2 m long
    q = 40
    step = dist(xyz[q], xyz[q - 1])
    assert step < dist(xyz[0], xyz[q]) < 4.0 < dist(xyz[q - 2], xyz[q])
    assert candidate(L, xyz, q, 0.0, 4.0) == q - 1 == brute(xyz, q, 0.0, 4.0)  # the frame just before is the nearest of all
    assert candidate(L, xyz, q, 1.5 * step, 4.0) == 0 == brute(xyz, q, 1.5 * step, 4.0)
    # exactly the way travelled is enough (>=), more than the whole way is not
    travelled = 0.0
    for i in range(1, q + 1):
        travelled = travelled + dist(xyz[i], xyz[i - 1])
    assert candidate(L, xyz, q, travelled, 4.0) == 0 == brute(xyz, q, travelled, 4.0)
    assert candidate(L, xyz, q, travelled * 2, 4.0) == -1
    # max_distance is inclusive too
    d = dist(xyz[0], xyz[q])
    assert candidate(L, xyz, q, 10.0, d) == 0 and candidate(L, xyz, q, 10.0, np.nextafter(d, 0.0)) == -1


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_walks_against_brute_force(L, seed):
    rng = np.random.default_rng(seed)
    xyz = np.cumsum(rng.normal(0.0, 1.0, (300, 3)) * [1.0, 1.0, 0.05], 0)
    found = 0
    for q in range(0, 300, 7):
        for min_travelled, max_distance in [(0.0, 1.0), (20.0, 4.0), (50.0, 10.0), (1e9, 1e9)]:
            got = candidate(L, xyz, q, min_travelled, max_distance)
            assert got == brute(xyz, q, min_travelled, max_distance), (q, min_travelled, max_distance)
            found += got >= 0
    assert found > 20  # (the walks do come back to where they were)


def test_bad_arguments_are_refused(L):
    xyz = figure_of_eight()
    for q in (-1, len(xyz)):
        with pytest.raises(L.LsaError) as e:
            candidate(L, xyz, q, 1.0, 1.0)
        assert e.value.code == L.E_ARG
    for mt, md in [(-1.0, 1.0), (1.0, -1.0), (np.nan, 1.0)]:
        with pytest.raises(L.LsaError) as e:
            candidate(L, xyz, 10, mt, md)
        assert e.value.code == L.E_ARG
    assert L.lib().lsa_loop_closure_candidate(None, 5, 2, 1.0, 1.0) == L.E_ARG
