"""The one-launch solve (k_lm_solve, lsa_solve_device) returns what it returned before, bit for bit.

tests/golden/lm_solve_parent.npz was written on an MI355X by tests/golden/make_lm_solve_parent.py from the library of
commit 692572f34fdd3e45960885fd05a9f493002b7c63 ("One ICP loop driver for ego-motion and localization"), the parent of the
change that folds the workgroups' sums straight from the exchange granules -- never from the code under test.  It holds,
for every case, the inputs that rebuild it and the 45 doubles of the kernel's result (tests/lm_solve_pinned_cases.py):
16 / 64 / 128 rings x 2D / 3D x the three start points of test_one_launch_solve_equals_the_host_driven_loop, and per sensor
model and mode a max_iter = 1 solve and a solve skipped for min_matches, and the solve after one whose workgroup 3 gave up.

The invariant behind it: every double the kernel produces is obtained by the same sequence of IEEE operations on the same
operands, however the work is spread over lanes and barriers.  So the comparison is `==` on the bit patterns, every entry.
"""
import os

import numpy as np
import pytest

import lm_solve_pinned_cases as PC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lm_solve_parent.npz")
COMMIT = "692572f34fdd3e45960885fd05a9f493002b7c63"


@pytest.fixture(scope="module")
def recorded():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def test_the_record_holds_the_cases_of_this_tree(recorded):
    """the fixture's inputs are the cases this tree builds: nothing was dropped or swapped since it was recorded"""
    assert str(recorded["commit"]) == COMMIT
    cases = PC.cases()
    assert [str(n) for n in recorded["names"]] == [c[0] for c in cases]
    assert len(cases) == 3 * 2 * (3 + 2) + 1
    assert recorded["result"].shape == (len(cases), PC.RESULT_DOUBLES) and recorded["result"].dtype == np.float64
    for i, (name, model, two_d, w0, max_iter, min_matches, give_up) in enumerate(cases):
        assert (recorded["rings"][i], recorded["two_d"][i], recorded["max_iter"][i], recorded["min_matches"][i], recorded["give_up_block"][i]) == (
            model, int(two_d), max_iter, min_matches, give_up), name
        assert np.array_equal(recorded["w0"][i].view(np.uint64), w0.view(np.uint64)), name
    # the record is of solves that did something: several evaluations, steps taken, and the three ways a case can end early
    res = {str(n): r for n, r in zip(recorded["names"], recorded["result"])}
    assert all(r[40] >= 3 and r[37] >= 2 and r[41] == 0 for n, r in res.items() if "prior0" in n or "prior1" in n)
    assert all(r[39] == 1 for n, r in res.items() if "max_iter1" in n)
    assert all(r[41] == 1 and r[40] == 1 and r[42] == 1 for n, r in res.items() if "min_matches" in n)


@pytest.fixture(scope="module")
def own_ctx(L):
    """a context of this module's own: the case whose workgroup gives up counts a fall-back, and other tests hold the
    shared context's count at 0"""
    ctx = L.Context(0)
    yield ctx
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("model", PC.MODELS)
def test_solve_device_returns_the_recorded_bits(own_ctx, O, L, recorded, model):
    gpu_ctx = own_ctx
    PC.setup_residuals(gpu_ctx, L, PC.keypoints(O, L, model))
    want = {str(n): r for n, r in zip(recorded["names"], recorded["result"])}
    before = gpu_ctx.solve_device_fallbacks()
    gave_up = 0
    bad = []
    for case in PC.cases():
        if case[1] != model:
            continue
        gave_up += case[6] != PC.NO_BLOCK
        got = PC.run_case(gpu_ctx, L, case)
        a, b = got.view(np.uint64), want[case[0]].view(np.uint64)
        diff = np.flatnonzero(a != b)
        print(f"{case[0]}: {diff.size} of {a.size} entries differ" + "".join(f"; [{i}] {got[i]!r} recorded {want[case[0]][i]!r}" for i in diff[:6]))
        if diff.size:
            bad.append((case[0], diff.tolist()))
    assert not bad, bad
    # only the workgroup told to give up made a solve fall back
    assert gpu_ctx.solve_device_fallbacks() == before + gave_up
