"""The reference and the bound that tests/test_gpu_reduction.py holds k_accumulate and k_lm_solve to, checked on the CPU
(tests/reduction_cases.py has the derivation): the oracle's sequential sum meets the bound, the EXACT family sums to
the same bits in every order, rejected rows never reach a sum, and the bound catches a dropped, doubled, misplaced or
stale term in every RANDOM and CANCEL case."""
import math
from fractions import Fraction

import numpy as np
import pytest

import reduction_cases as RC
from conftest import bits


def oracle_sums(O, rs, w):
    """O.accumulate, one call per type (each a sequential loop from 0), added up in type order"""
    S, count = np.zeros(RC.NSUMS), 0
    for t in range(3):
        if rs.counts[t] == 0:
            continue
        c, g, H, n = O.accumulate(rs.records[t], rs.status[t], rs.sat[t], w)
        S = S + RC.sums_of(c, g, H)
        count += n
    return S, count


def test_exact_family_is_exact_in_every_order(O):
    # a few thousand blocks against accumulate_one's formula in exact rational arithmetic
    for i, (n, g_zero) in enumerate(((1200, False), (1201, True), (1000, False))):
        rs = RC.exact_set(77 + i, RC.split(n, i), g_zero=g_zero)
        T = RC.block_terms(O, rs, np.zeros(6))
        frac = [RC.fraction_terms(row, rs.sat[t]) for t in range(3) for row in rs.records[t]]
        assert T.shape[0] == len(frac) == n
        for j, (tr, fr) in enumerate(zip(T, frac)):
            assert all(Fraction(float(a)) == b for a, b in zip(tr, fr)), f"{rs} block {j}: per-block value is not exact"
        exact = [sum((fr[v] for fr in frac), Fraction(0)) for v in range(RC.NSUMS)]
        assert [Fraction(float(v)) for v in RC.fsum_cols(T)] == exact
    # at the sizes the GPU tests use: every value a multiple of 2^-15, every entry's sum |t_i| < 2^38 -- so every
    # partial sum is a double and every order gives the exact sum
    for i, n in enumerate((513, 4609, 32767, 163840)):
        for g_zero in (False, True):
            rs = RC.exact_set(88 + i, RC.split(n, i), g_zero=g_zero)
            T = RC.block_terms(O, rs, np.zeros(6))
            scaled = T * 2.0 ** 15
            assert np.array_equal(scaled, np.round(scaled)), f"{rs}: a value is not a multiple of 2^-15"
            assert np.abs(scaled).sum(axis=0).max() < 2.0 ** 53
            ref = RC.fsum_cols(T)
            exact = np.array([sum(int(v) for v in scaled[:, c].tolist()) for c in range(RC.NSUMS)])
            assert np.array_equal(ref * 2.0 ** 15, exact.astype(np.float64)) and np.all(np.abs(exact) < 2 ** 53)
            seq = np.zeros(RC.NSUMS)
            for row in T[: 20000]:
                seq = seq + row
            seq = seq + T[20000:].sum(axis=0)
            rev = np.zeros(RC.NSUMS)
            for row in T[::-1][: 20000]:
                rev = rev + row
            rev = rev + T[::-1][20000:].sum(axis=0)
            S, count = oracle_sums(O, rs, np.zeros(6))
            for name, got in (("sequential", seq), ("reversed", rev), ("pairwise", T.sum(axis=0)), ("oracle", S)):
                assert np.array_equal(bits(got + 0.0), bits(ref)), f"{rs}: {name} sum differs from the exact sum"
            assert count == n
            if g_zero:
                assert not np.any(ref[1:7]) and np.any(ref[7:])


@pytest.mark.parametrize("rs", RC.cpu_cases(), ids=repr)
def test_oracle_sum_meets_the_bound(O, rs):
    for w in rs.points:
        ref = RC.Reference(O, rs, w)
        S, count = oracle_sums(O, rs, w)
        assert count == ref.count == rs.nvalid
        # each type's loop adds at most counts[t] terms from 0, then the three results are added
        bad = ref.violations(S, max(rs.counts) + 2)
        assert bad.size == 0, f"{rs} at {w}: entries {bad} outside the bound"


@pytest.mark.parametrize("pattern", RC.REJECT_PATTERNS)
def test_rejected_rows_never_reach_the_oracle_sum(O, pattern):
    for i, make in enumerate((lambda c: RC.exact_set(5, c), lambda c: RC.random_set(6, c, 1), lambda c: RC.cancel_set(7, c, 0))):
        rs = make(RC.split(4609, i))
        mask = RC.reject_rows(rs.total, rs.counts, 9 * RC.THREADS_LM, pattern)
        bad, zero = RC.rejected(rs, mask), RC.rejected(rs, mask, zero_payload=True)
        assert any(np.isnan(r).any() for r in bad.records)
        for w in rs.points:
            a, ca = oracle_sums(O, bad, w)
            b, cb = oracle_sums(O, zero, w)
            assert np.array_equal(bits(a), bits(b)) and ca == cb == rs.total - int(mask.sum())


@pytest.mark.parametrize("rs", RC.cpu_cases(), ids=repr)
def test_the_bound_catches_every_mutant(O, rs):
    """at the widest depth any forced shape uses, the bound flags each mutant of the sums in the 28 float entries
    alone (the count would catch a doubled block by itself)"""
    for w in rs.points:
        ref = RC.Reference(O, rs, w)
        assert ref.count > 0
        for name, S, count in RC.mutant_sums(O, rs, w, ref):
            assert ref.violations(S, RC.D_WIDE).size > 0, f"{rs} at {w}: mutant '{name}' passes the bound"


def test_depths_read_from_the_code():
    # k_lm_solve at nb = 64, 5 blocks per thread: 5 + 6 + 7 + 8 + 7; k_accumulate at 256 blocks, one block per thread
    assert RC.depth_lm(64, 5) == 33 and RC.depth_lm(1, 1) == 22 and RC.depth_lm(9, 2) == 24
    assert RC.depth_accum(256, 1) == 266 <= RC.D_WIDE and RC.depth_accum(1, 6) == 16
    assert math.isclose(RC.gamma(1), RC.U / (1 - RC.U))
