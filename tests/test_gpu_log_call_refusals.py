"""What the five calls on the keypoint log refuse before they do anything (lsa_slam_log.cpp: SlamCore::LogReady / LogCovers):
logging off, a log that does not cover the logged poses, a log that stopped.  Every cell of the table holds the returned
code and the distinguishing words of lsa_slam_last_error, and that the refusal left the pose, the log and the maps alone.
Synthetic 16-ring sensor, three frames."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODEL, SEED, NFRAMES = 16, 1000, 3


@pytest.fixture(scope="module")
def frames(L):
    return [L.synth_frame(MODEL, SEED, f) for f in range(NFRAMES)]


def make_off(L, frames):
    s = L.Slam(0, EgoMotion=3, LoggingTimeout=0)
    for f, (pts, stamp) in enumerate(frames):
        s.add_frame(pts, stamp, f)
    return s


def make_not_covering(L, frames):
    """logging switched on after the first frame: three logged poses, two logged frames"""
    s = L.Slam(0, EgoMotion=3, LoggingTimeout=0)
    s.add_frame(frames[0][0], frames[0][1], 0)
    s.set_param("LoggingTimeout", -1)
    for f in (1, 2):
        s.add_frame(frames[f][0], frames[f][1], f)
    assert s.trajectory()[1].size == 3 and s.logged_frames() == 2
    return s


def make_stopped(L, frames):
    s = L.Slam(0, EgoMotion=3, LoggingTimeout=-1)
    s.context().debug_set("kplog_fail_alloc", 1)  # the log's first chunk cannot be had
    s.add_frame(frames[0][0], frames[0][1], 0)
    s.context().debug_set("kplog_fail_alloc", 0)
    for f in (1, 2):
        s.add_frame(frames[f][0], frames[f][1], f)
    assert s.trajectory()[1].size == 3 and s.logged_frames() == 0
    return s


STATES = {"off": make_off, "not_covering": make_not_covering, "stopped": make_stopped}


@pytest.fixture(scope="module")
def slams(L, frames):
    """one object per state, made when first asked for and shared by the calls: a refusal changes nothing (asserted)"""
    made = {}

    def get(state):
        if state not in made:
            made[state] = STATES[state](L, frames)
        return made[state]

    yield get
    for s in made.values():
        s.close()


def call(L, s, name, short=False):
    P, t, _ = s.trajectory()
    if name == "SetTrajectoryAndRebuildMaps":
        s.set_trajectory(P[:-1], t[:-1]) if short else s.set_trajectory(P, t)
    elif name == "RecognizePlace":
        s.recognize_place(P.shape[0] - 1)
    elif name == "OptimizeLoggedTrajectory":
        s.optimize_trajectory([])
    elif name == "RunPoseGraphOptimization":
        s.run_pose_graph_optimization(t, P[:, :3, 3], np.tile(np.eye(3), (t.size, 1, 1)))
    elif name == "RegisterLoggedFrames":
        s.register_logged_frames(P.shape[0] - 1, 0)


# the last clause of "keypoint logging is off (LoggingTimeout = 0): ..." per call
MISSING = {
    "SetTrajectoryAndRebuildMaps": "there is nothing to rebuild the maps from",
    "RecognizePlace": "there are no logged keypoints to describe",
    "OptimizeLoggedTrajectory": "there is no logged trajectory to optimize",
    "RunPoseGraphOptimization": "there is no logged trajectory to optimize",
    "RegisterLoggedFrames": "there are no logged keypoints to register against",
}
WORDS = {
    "off": lambda name: "keypoint logging is off (LoggingTimeout = 0): " + MISSING[name],
    "not_covering": lambda name: "the keypoint log does not cover the logged poses (logging was switched on after the first of them)",
    "stopped": lambda name: "keypoint logging stopped when a chunk could not be allocated; Reset(true) starts it again",
}
CELLS = [(state, name, False) for state in STATES for name in MISSING] + [("not_covering", "SetTrajectoryAndRebuildMaps", True)]


def snapshot(L, s):
    return s.world_transform().tobytes(), s.logged_frames(), tuple(s.map(k).size for k in (L.EDGE, L.PLANE, L.BLOB))


@pytest.mark.parametrize("state,name,short", CELLS, ids=[f"{s}-{n}{'-short' if w else ''}" for s, n, w in CELLS])
def test_a_log_call_refuses_and_changes_nothing(L, slams, state, name, short):
    s = slams(state)
    before = snapshot(L, s)
    with pytest.raises(L.LsaError) as e:
        call(L, s, name, short)
    said = s.L.lsa_slam_last_error(s.h).decode()
    if short:
        # a wrong number of poses is refused before the log is asked whether it covers them
        assert e.value.code == L.E_ARG and said == name + ": 2 poses for 3 logged ones", said
    else:
        assert e.value.code == L.E_STATE and said == name + ": " + WORDS[state](name), said
    assert snapshot(L, s) == before
