"""The trust-region step spread over the first wavefront's lanes returns what the one-lane step returned, bit for bit, on
the branches tests/test_gpu_lm_solve_pinned.py does not reach: rejected candidates (the kept scaled system, then a new one),
rejections in a row, max_iter 0 to 3, a solve restarted from its own result, a start without a gradient, too few matches,
and the solve after one that was given up.

tests/golden/lm_step_lanes_parent.npz was written on an MI355X by tests/golden/make_lm_step_lanes_parent.py from the library
of commit 3f43cd1 ("Split the SLAM host pipeline by job; one refusal path for the log calls"), the parent of the change --
never from the code under test.  The comparison is `==` on the bit patterns of all 45 doubles of every case
(tests/lm_step_lanes_cases.py).

Not walked by these records: the invalid step -- a failed Cholesky factorization or a negative model cost change -- with its
retry, the reset of the count and kCodeInvalidSteps; kCodeMinRadius; the clamps at max_radius and min_diagonal; kCodeGradient
after iteration 0; non-finite sums.  No start on residual blocks was found that reaches them (a random search with the
parent's library over some thousand starts): the residual blocks decide what the step sees.  tests/test_gpu_lm_step.py and
tests/test_lm_step_reference.py walk them by feeding the step its 29 sums directly, against an independent statement of
the loop (tests/lm_step_cases.py) instead of a parent's bits.
"""
import os

import numpy as np
import pytest

import lm_solve_pinned_cases as PC
import lm_step_lanes_cases as SC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lm_step_lanes_parent.npz")
COMMIT = "3f43cd1"


@pytest.fixture(scope="module")
def recorded():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def test_the_record_holds_the_cases_and_the_branches(recorded):
    """the fixture's inputs are the cases this tree builds, and the parent walked the branches they are there for: a
    re-recording cannot silently lose them"""
    assert str(recorded["commit"]).startswith(COMMIT)
    cases = SC.cases()
    assert [str(n) for n in recorded["names"]] == [c[0] for c in cases]
    assert recorded["result"].shape == (len(cases), SC.RESULT_DOUBLES) and recorded["result"].dtype == np.float64
    res = {str(n): r for n, r in zip(recorded["names"], recorded["result"])}
    for i, (name, rings, two_d, w0, max_iter, min_matches, give_up, restart_of, turns) in enumerate(cases):
        assert (recorded["rings"][i], recorded["two_d"][i], recorded["max_iter"][i], recorded["min_matches"][i], recorded["give_up_block"][i],
                str(recorded["restart_of"][i]), recorded["yaw_turns"][i]) == (rings, int(two_d), max_iter, min_matches, give_up, restart_of or "", turns), name
        # (a restarted case starts where the recorded result of the case before it says)
        assert np.array_equal(recorded["w0"][i].view(np.uint64), SC.start_point(cases[i], res).view(np.uint64)), name
    # at least three cases with a rejected step, one with two rejections in a row, five ways of ending
    assert sum(r[38] >= 1 for r in res.values()) >= 3
    assert SC.rejected_iterations(res, "r16_3d_wild_b") == [2, 3]
    assert len({int(r[42]) for r in res.values()}) >= 5
    # a rejection followed by an acceptance inside one solve: the first candidate is rejected, the solve goes on to converge
    assert SC.rejected_iterations(res, "r16_3d_wild_a") == [1] and res["r16_3d_wild_a"][38] == 1 and res["r16_3d_wild_a"][37] >= 3
    # the restarted solves are over at once, the skipped one never starts
    assert all(r[39] <= 1 for n, r in res.items() if "restart" in n)
    assert all(r[41] == 1 and r[42] == 1 for n, r in res.items() if "min_matches" in n)
    assert all(r[39] == int(n[-1]) for n, r in res.items() if "max_iter" in n and "_3d_" in n)


@pytest.fixture(scope="module")
def own_ctx(L):
    """a context of this module's own: the case whose workgroup gives up counts a fall-back, and other tests hold the
    shared context's count at 0"""
    ctx = L.Context(0)
    yield ctx
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("model", SC.MODELS)
def test_solve_device_returns_the_recorded_bits(own_ctx, O, L, recorded, model):
    want = {str(n): r for n, r in zip(recorded["names"], recorded["result"])}
    before = own_ctx.solve_device_fallbacks()
    got = SC.run_model(own_ctx, L, model, PC.keypoints(O, L, model))
    assert got, model
    bad = []
    for name, g in got.items():
        a, b = g.view(np.uint64), want[name].view(np.uint64)
        diff = np.flatnonzero(a != b)
        print(f"{name}: {diff.size} of {a.size} entries differ" + "".join(f"; [{i}] {g[i]!r} recorded {want[name][i]!r}" for i in diff[:6]))
        if diff.size:
            bad.append((name, diff.tolist()))
    assert not bad, bad
    # only the workgroups told to give up made a solve fall back
    gave_up = sum(c[6] != SC.NO_BLOCK for c in SC.cases() if c[1] == model)
    assert own_ctx.solve_device_fallbacks() == before + gave_up
