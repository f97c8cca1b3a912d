"""Cases of tests/test_gpu_lm_step_lanes.py: solves that walk the trust-region branches the pinned cases do not reach.

Shared by the test and by tests/golden/make_lm_step_lanes_parent.py, which records what the library of the commit BEFORE
the step was spread over the first wavefront's lanes returns; the test holds the library under test to that record, bit
for bit.  The residual blocks are those of tests/lm_solve_pinned_cases.py (scan 1 on scan 0, seed 1000, matched at
(0.45, 0.02, 0; yaw 0.01), saturation 5 m): VLP-16 (about 3 k residual blocks, 6 workgroups) and one HDL-64 start.

Start points.  The synthetic scene is forgiving: from (dx, yaw) up to (6 m, 0.5) -- the FAR starts below are of that kind --
every candidate of the recorded library is accepted.  Steps are rejected only from starts that are turned by a radian or
more, where most residual blocks lie beyond the saturation distance; the WILD starts were found by a random search with
the recorded library (which is how they were chosen: by what the PARENT does with them) and are kept because of where its
rejections fall:
  wild_a   the first candidate is rejected, the second accepted (the kept system, then a new one);
  wild_b   iterations 2 and 3 are rejected one after the other, 4 is accepted;
  wild_c   iterations 4, 5 and 6 are rejected; 8 rejections in 15 iterations;
  wild_d   iterations 5 to 8 are rejected;
  wild_64  HDL-64: iterations 1 and 2 are rejected.
In 2D mode z, rx and ry of a start are not parameters but stay part of the point, so a wild start is a tilted 2D problem.
No start was found that makes the parent's damped Cholesky fail or the model's cost change negative (the invalid step):
these records do not walk it.  tests/lm_step_cases.py does, with scripted sums instead of residual blocks.

A case is (name, rings, two_d, w0 | None, max_iter, min_matches, give_up_block, restart_of, yaw_turns): with `restart_of`
the start point is the pose the named case (run before it) returned, plus `yaw_turns` full turns on the yaw -- whole
turns leave the problem where it is and make the point's norm large, which is what the parameter tolerance compares the
step with.
"""
import numpy as np

import lm_solve_pinned_cases as PC

MODELS = (16, 64)
NO_BLOCK = PC.NO_BLOCK
GIVE_UP_BLOCK = 3
RESULT_DOUBLES = PC.RESULT_DOUBLES

FAR = {"far1": (1.0, 0.02, 0.0, 0.0, 0.0, 0.1), "far2": (2.0, 0.02, 0.0, 0.0, 0.0, 0.2), "far3": (3.0, 0.02, 0.0, 0.0, 0.0, 0.3)}
WILD = {
    "wild_a": (3.94, 4.39, -1.68, -0.97, -1.49, -0.18),
    "wild_b": (0.12, -12.57, 25.46, 0.91, 2.06, -1.6),
    "wild_c": (-23.93, -7.16, -21.98, 0.97, 1.98, -0.74),
    "wild_d": (-20.04, 10.67, -28.74, -1.14, 2.63, 0.23),
}
WILD_64 = (8.37, 28.69, 6.29, -1.32, 1.09, 0.51)
# every residual block far beyond the saturation distance (Tukey's weight is 0 there): the gradient at the start point is
# exactly 0.  (A kilometre is not enough: the scene has lines and planes the shift runs nearly along.)
SATURATED = (1.0e6, 2.3e6, 3.7e6, 0.0, 0.0, 0.0)
TURNS = 10000  # full turns of the yaw: |x| about 6.3e4, inside the range lsa_pmath.h reduces exactly


def cases():
    """[(name, rings, two_d, w0 | None, max_iter, min_matches, give_up_block, restart_of, yaw_turns)]"""
    out = []

    def add(name, rings, two_d, w0, max_iter=15, min_matches=0, give_up=NO_BLOCK, restart_of=None, turns=0):
        out.append((name, rings, two_d, None if w0 is None else np.array(w0, np.float64), max_iter, min_matches, give_up, restart_of, turns))

    for two_d in (False, True):
        tag = "r16_" + ("2d" if two_d else "3d")
        for n, w in FAR.items():
            add(f"{tag}_{n}", 16, two_d, w)
        for n, w in WILD.items():
            add(f"{tag}_{n}", 16, two_d, w)
        for n in ("wild_a", "wild_b"):
            for mi in (1, 2, 3):
                add(f"{tag}_{n}_max_iter{mi}", 16, two_d, WILD[n], max_iter=mi)
        add(f"{tag}_wild_c_max_iter8", 16, two_d, WILD["wild_c"], max_iter=8)
        add(f"{tag}_far2_max_iter0", 16, two_d, FAR["far2"], max_iter=0)
        # restarted from its own result: done at once
        add(f"{tag}_far2_restart", 16, two_d, None, restart_of=f"{tag}_far2")
        add(f"{tag}_wild_a_restart", 16, two_d, None, restart_of=f"{tag}_wild_a")
        add(f"{tag}_far2_restart_turned", 16, two_d, None, restart_of=f"{tag}_far2", turns=TURNS)
        add(f"{tag}_saturated", 16, two_d, SATURATED)
        add(f"{tag}_wild_b_min_matches", 16, two_d, WILD["wild_b"], min_matches=10 ** 7)
        add(f"{tag}_wild_a_after_give_up", 16, two_d, WILD["wild_a"], give_up=GIVE_UP_BLOCK)
    for two_d in (False, True):
        add("r64_" + ("2d" if two_d else "3d") + "_wild_64", 64, two_d, WILD_64)
    return out


def start_point(case, results):
    """the case's start point; `results`: name -> 45 doubles of the cases run before it"""
    name, rings, two_d, w0, max_iter, min_matches, give_up, restart_of, turns = case
    if restart_of is None:
        return w0
    w = np.array(results[restart_of][:6], np.float64)
    w[5] = w[5] + turns * (2.0 * np.pi)
    return w


def run_model(ctx, L, model, kps):
    """name -> 45 doubles for the cases of one sensor model, in order"""
    PC.setup_residuals(ctx, L, kps)
    results = {}
    for case in cases():
        if case[1] != model:
            continue
        pinned_case = (case[0], case[1], case[2], start_point(case, results), case[4], case[5], case[6])
        results[case[0]] = PC.run_case(ctx, L, pinned_case)
    return results


def rejected_iterations(res, stem):
    """iterations 1..3 of the start `stem` that ended in a rejection, from its max_iter = 1, 2, 3 cases: the solve is
    deterministic, so max_iter = k stops the same walk after k iterations"""
    out, before = [], 0.0
    for mi in (1, 2, 3):
        u = res[f"{stem}_max_iter{mi}"][38]
        if u == before + 1:
            out.append(mi)
        before = u
    return out
