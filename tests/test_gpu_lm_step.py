"""The device's trust-region step -- lm_step of lsa_lm.hip, the code k_lm_solve inlines, driven by lsa_selftest_lm_step on
scripted sums -- equals the independent float64 statement of tests/lm_step_cases.py bit for bit: every record of every
case, 2D and 3D, and the 45 result doubles (the sums of the last accepted point: a wrong buffer flip shows there).  All
scripts run in one launch.  tests/test_lm_step_reference.py asserts on the reference's trace that every case reaches its
branch, and holds the host loop to the same records."""
import numpy as np
import pytest

import lm_step_cases as LC


@pytest.mark.gpu
def test_device_step_equals_the_reference(L, gpu_ctx):
    cases = LC.cases()
    records, results, status = L.selftest_lm_step([c.script for c in cases], gpu_ctx)
    fails = LC.compare(cases, records, results, status)
    print(f"{len(cases)} scripts, {sum(len(c.sums) for c in cases)} evaluations, {len(fails)} differ")
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
def test_device_step_equals_the_host_loop(L, gpu_ctx):
    """the two loops that must take the same decisions from the same sums, held to each other directly; and a script that
    runs out before the solve stops reports so on both"""
    cases = LC.cases()
    valley = next(c for c in cases if c.name == "2d_valley")
    scripts = [c.script for c in cases] + [(valley.two_d, valley.max_iter, valley.min_matches, valley.x0, valley.sums[:7])]
    dev, host = L.selftest_lm_step(scripts, gpu_ctx), L.selftest_lm_step(scripts)
    assert np.array_equal(dev[2], host[2]) and dev[2][-1].tolist() == [1, 7]
    assert np.array_equal(LC.canonical(dev[1]), LC.canonical(host[1]))
    assert len(dev[0]) == len(host[0]) == len(scripts)
    for a, b in zip(dev[0], host[0]):
        assert np.array_equal(LC.canonical(a), LC.canonical(b))
