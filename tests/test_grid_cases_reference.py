"""The cases of tests/grid_cases.py have to be trusted before the device maps are held to them (tests/test_gpu_grid_cases.py):
every case contains what it is there to contain, the oracle's RollingGrid equals the plain statement of the per-voxel rule
byte for byte on every call of every case (samplings FIRST, LAST, MAX_INTENSITY, CENTER_POINT -- this checks the oracle
itself), and the host RollingGrid behind the C ABI equals the oracle on one and on four threads.  No GPU, no tolerance."""
import numpy as np
import pytest

import grid_cases as G
import lidarslam_amd as L
from oracle import oracle as O
from test_rolling_grid import same_state, same_submap

ALL = G.CASES + G.MULTI.maps


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c.name)
def test_every_case_contains_what_it_is_there_for(case):
    assert G.vacuity_problems(case) == []
    assert all(op.points.size <= G.BATCH for op in case.ops if isinstance(op, G.Add))


def test_the_launches_of_several_maps_are_the_stated_ones():
    assert G.multi_problems(G.MULTI) == []


def test_the_key_on_faces_rounds_half_away_from_zero():
    """the statement's own rounding at the places the cases are about, in plain numbers: GridSize 6, origin -12"""
    xyz = np.array([[-14.0, 0, 0], [-13.875, 0, 0], [10.0, 0, 0], [9.875, 0, 0], [-10.0, 0, 0], [-12.25, -12.25, -12.25], [-11.75, 0, 0]], np.float32)
    out, inn, inside, _ = G.voxel_coords(xyz, 6, 4.0, 0.5, (0, 0, 0))
    assert inside.tolist() == [False, True, False, True, True, True, True]
    assert out[:, 0].tolist() == [-1, 0, 6, 5, 1, 0, 0]       # -0.5 -> -1, 5.5 -> 6, 0.5 -> 1
    assert inn[4:, 0].tolist() == [-4, -1, 1]                  # -2.0 / 0.5; -0.5 -> -1; 0.5 -> 1
    keys = G.voxel_keys(xyz, 6, 4.0, 0.5, (0, 0, 0))
    assert keys[0] == keys[2] == G.NO_KEY
    assert int(keys[5]) == (0 << 32) | ((-1 * 36 - 1 * 6 - 1) & 0xFFFFFFFF)  # To1d of negative leaf coordinates, as unsigned


class StatementMap(G.Statement):
    """the statement behind the calls same_state makes (sub-maps are not stated: the oracle's own are compared with the host's)"""

    def __init__(self, case, sampling):
        super().__init__(case.grid_size, sampling, case.min_frames)


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_the_oracle_equals_the_statement_on_every_call(case):
    for sampling in case.samplings():
        s, o = StatementMap(case, sampling), O.RollingGrid(Sampling=sampling, **case.params())
        calls = 0
        for op in case.ops:
            if isinstance(op, G.SubMap):
                continue
            if isinstance(op, G.Add):
                for m in (s, o):
                    m.add(op.points, fixed=op.fixed, time=op.time, roll=op.roll)
            else:
                for m in (s, o):
                    m.roll(op.mn, op.mx)
            same_state(s, o)
            calls += 1
        assert calls >= 1 and o.size() > 0


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_the_host_grid_equals_the_oracle(case, threads):
    for sampling in case.samplings() + ((4,) if case.centroid else ()):
        g, o = L.RollingGrid(Sampling=sampling, **case.params()), O.RollingGrid(Sampling=sampling, **case.params())
        g.set("AddThreads", threads)
        G.play(case, sampling, g, o, same_state, same_submap)
        assert o.size() > 0
