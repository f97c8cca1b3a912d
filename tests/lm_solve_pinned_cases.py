"""Cases of the pinned one-launch solve (tests/test_gpu_lm_solve_pinned.py) and how each is rebuilt and run.

Shared by the test and by tests/golden/make_lm_solve_parent.py, which records what the library of the commit BEFORE a change
to k_lm_solve returns; the test then holds the library under test against that record, bit for bit.

A case is (rings, two_d, start point, max_iter, min_matches, give_up_block).  Its inputs are the residual blocks of
tests/test_gpu_match.py::test_one_launch_solve_equals_the_host_driven_loop: edge and plane keypoints of synthetic scan 1
(seed 1000) matched on those of scan 0 under the ego-motion setup at the pose (0.45, 0.02, 0; yaw 0.01), saturation 5 m.
Everything in front of the solve is bit-exact against the oracle (tests/test_gpu_match.py), so the record depends on the
solve kernel alone.
"""
import numpy as np

MODELS = (16, 64, 128)  # VLP-16, HDL-64, VLS-128
PRIORS = ((0.3, 0.0), (0.45, 0.01), (0.0, 0.0))  # (dx, yaw) of test_one_launch_solve_equals_the_host_driven_loop
NO_BLOCK = -1
GIVE_UP_BLOCK = 3

# the kernel's result, 45 doubles: pose[6], initial cost, final cost, the 29 sums at the final point (cost, g[6], the upper
# triangle of H row by row, the count), successful / unsuccessful steps, iterations, evaluations, skipped, termination
# code, matches, failure.  lsa_solve_result_t carries all of them but the count among the sums, which is the number of
# matches again, and the failure, which is 0 whenever a result is returned.
RESULT_DOUBLES = 45


def cases():
    """[(name, rings, two_d, w0[6], max_iter, min_matches, give_up_block)]"""
    out = []
    for model in MODELS:
        for two_d in (False, True):
            tag = f"r{model}_{'2d' if two_d else '3d'}"
            for i, (dx, yaw) in enumerate(PRIORS):
                out.append((f"{tag}_prior{i}", model, two_d, np.array([dx, 0.02, 0.0, 0.0, 0.0, yaw]), 15, 0, NO_BLOCK))
            w0 = np.array([0.45, 0.02, 0.0, 0.0, 0.0, 0.01])
            out.append((f"{tag}_max_iter1", model, two_d, w0, 1, 0, NO_BLOCK))
            out.append((f"{tag}_min_matches", model, two_d, w0, 15, 10 ** 7, NO_BLOCK))
    # a workgroup abandons the exchange: that solve reports LSA_E_STATE; the one after it is recorded
    out.append(("r128_3d_after_give_up", 128, False, np.array([0.45, 0.02, 0.0, 0.0, 0.0, 0.01]), 15, 0, GIVE_UP_BLOCK))
    return out


def match_pose():
    T = np.eye(4)
    c, s = np.cos(0.01), np.sin(0.01)
    T[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    T[:3, 3] = [0.45, 0.02, 0.0]
    return T


def keypoints(O, L, model):
    """edge / plane / blob keypoints of scans 0 and 1, extracted by the oracle"""
    ex = O.Extractor()
    per = []
    for f in range(2):
        pts, _ = L.synth_frame(model, 1000, f)
        ex.compute(pts)
        per.append([ex.keypoints(k) for k in range(3)])
    return per


def setup_residuals(ctx, L, kps):
    prev, cur = kps
    mp = L.MatchParams.ego_motion(saturation_distance=5.0)
    for k in (0, 1):
        ctx.set_keypoints(L.SET_WORKING, k, cur[k])
        ctx.set_target(k, prev[k])
        ctx.match(k, L.SET_WORKING, mp, match_pose())
    ctx.set_keypoints(L.SET_WORKING, 2, cur[2][:0])
    ctx.match(2, L.SET_WORKING, mp, match_pose())


def result_doubles(r):
    H = np.array(r.H, np.float64).reshape(6, 6)
    sums = [r.cost] + list(r.g) + [H[a, b] for a in range(6) for b in range(a, 6)] + [float(r.num_matches)]
    v = list(r.pose) + [r.initial_cost, r.final_cost] + sums + [
        float(r.num_successful_steps), float(r.num_unsuccessful_steps), float(r.num_iterations), float(r.num_evaluations),
        float(r.skipped), float(r.termination), float(r.num_matches), 0.0]
    v = np.array(v, np.float64)
    assert v.size == RESULT_DOUBLES
    return v


def run_case(ctx, L, case):
    """the 45 doubles of one case; the residual blocks of its sensor model are set up already"""
    name, model, two_d, w0, max_iter, min_matches, give_up = case
    if give_up != NO_BLOCK:
        ctx.debug_set("lm_give_up_block", give_up)
        try:
            ctx.solve_device(7, w0, max_iter=max_iter, two_d=two_d, min_matches=min_matches)
        except L.LsaError:
            pass
        else:
            raise AssertionError(f"{name}: the solve whose workgroup {give_up} gave up returned a result")
    return result_doubles(ctx.solve_device(7, w0, max_iter=max_iter, two_d=two_d, min_matches=min_matches))
