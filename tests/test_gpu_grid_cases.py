"""The device maps (lsa_device_grid.hip, lsa_grid_add.hip, lsa_grid_submap.hip) on the cases of tests/grid_cases.py -- dense
and lattice clouds: long runs of points per voxel that cross the blocks of the fold and the runs of the sort, ties of
intensity and of distance, fixed voxels, Adds that change nothing, points and boxes exactly on faces, several maps in one
launch -- against the oracle's RollingGrid, call by call, byte for byte: map, clean map, size, sub-map, its point order and
its validity.  tests/test_grid_cases_reference.py holds the cases to what they declare and the oracle to a plain statement
of the rule.  No tolerance anywhere."""
import numpy as np
import pytest

import grid_cases as G
import lidarslam_amd as L
from oracle import oracle as O
from test_gpu_device_grid import same_state, same_submap

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


def pair(ctx, case, sampling, form=0, ordered=1):
    g, o = L.DeviceGrid(ctx), O.RollingGrid(Ordered=ordered, Sampling=sampling, **case.params())
    g.set("Ordered", ordered)  # before the first insertion: exact from then on
    g.set("Sampling", sampling)
    for k, v in case.params().items():
        g.set(k, v)
    g.set("GlobalScans", form)
    return g, o


def run(ctx, case, samplings, form=0, ordered=1):
    for sampling in samplings:
        g, o = pair(ctx, case, sampling, form, ordered)
        try:
            G.play(case, sampling, g, o, same_state, same_submap)
            assert o.size() > 0
        finally:
            g.close()


@pytest.mark.parametrize("ordered", [1, 0])
@pytest.mark.parametrize("form", [0, 1, 2])  # the merge with its scans in LDS, in global memory, there in blocks of 64
@pytest.mark.parametrize("case", [c for c in G.CASES if c.layer in (1, 2)], ids=lambda c: c.name)
def test_runs_ties_and_rules_in_every_form_of_the_merge(ctx, case, form, ordered):
    run(ctx, case, case.samplings(), form, ordered)


@pytest.mark.parametrize("case", [c for c in G.CASES if c.layer == 3], ids=lambda c: c.name)
def test_faces_rolls_and_sub_map_boxes(ctx, case):
    run(ctx, case, case.samplings())


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("case", [c for c in G.CASES if c.centroid], ids=lambda c: c.name)
def test_centroid_on_few_voxels(ctx, case, form):
    """the oracle's loop costs points x voxels: at most 64 voxels"""
    run(ctx, case, (4,), form)


@pytest.mark.parametrize("form", [0, 1])
def test_several_maps_in_one_launch(ctx, form):
    """lsa_device_grid_stage_keypoints_all + lsa_device_grid_add_staged_all (blockIdx.y = map): three maps of different
    parameters and sizes, staged counts (1, 4097, 300), (4097, 1, 0), (0, 0, 257), twice; the pose is the identity, so the
    staged points are the keypoints"""
    m = G.MULTI
    lib = L.lib()
    pairs = [pair(ctx, c, c.sampling, form) for c in m.maps]
    try:
        for (g, o), c, nb in zip(pairs, m.maps, m.before):
            for op in c.ops[:nb]:
                g.add(op.points, fixed=op.fixed, time=op.time, roll=op.roll), o.add(op.points, fixed=op.fixed, time=op.time, roll=op.roll)
            same_state(g, o)
        assert sorted(o.size() > 1024 for _, o in pairs) == [False, False, True] and min(o.size() for _, o in pairs) == 0
        handles = np.array([g.h.value for g, _ in pairs], np.uint64)  # lsa_device_grid* const*
        types = np.array([L.EDGE, L.PLANE, L.BLOB], np.int32)
        pose = L.pose16(np.eye(4))
        for t, batch in m.rounds:
            for k, pts in enumerate(batch):
                ctx.set_keypoints(L.SET_WORKING, k, pts)
            assert lib.lsa_device_grid_stage_keypoints_all(L.ptr(handles), L.ptr(types), 3, L.SET_WORKING, L.ptr(pose)) == 0, lib.lsa_last_error(ctx.h)
            assert lib.lsa_device_grid_add_staged_all(L.ptr(handles), 3, t) == 0, lib.lsa_last_error(ctx.h)
            for (g, o), pts in zip(pairs, batch):
                o.add(pts, fixed=False, time=t, roll=True)
                same_state(g, o)
                same_submap(g, o)
        assert all(o.size() > 0 for _, o in pairs)
    finally:
        for g, _ in pairs:
            g.close()
