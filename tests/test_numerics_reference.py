"""The oracle's restatements of the fixed-size solvers and the product's host twins (SolveSPD, the Jacobi eigen-solver
of host/lsa_lm.cpp) against 50-digit mpmath references, at the degenerate inputs synthetic scans never reach.  CPU only.
Cases, references and bounds: tests/numerics_cases.py; findings: DESIGN.md 4.4."""
import numpy as np
import pytest

import numerics_cases as NC


def _report(fails):
    assert not fails, f"{len(fails)} violation(s):\n" + "\n".join(fails[:25])


@pytest.mark.parametrize("dtype,fn", [(np.float32, NC.FN["PCA_F"]), (np.float64, NC.FN["PCA_D"])], ids=["float", "double"])
def test_oracle_pca_against_mpmath(O, dtype, fn):
    fam = NC.pca_family()
    _report(NC.check_pca(fam, O.numerics(fn, fam.records), dtype))


@pytest.mark.parametrize("dtype,fn", [(np.float32, NC.FN["EIG33_F"]), (np.float64, NC.FN["EIG33_D"])], ids=["float", "double"])
def test_oracle_eigen33_against_mpmath(O, dtype, fn):
    fam = NC.eig33_family(dtype)
    _report(NC.check_eig33(fam, O.numerics(fn, fam.records), dtype))


@pytest.mark.parametrize("N", [3, 6])
def test_oracle_cholesky_against_mpmath(O, N):
    fam = NC.spd_family(N)
    _report(NC.check_spd(fam, O.numerics(NC.FN[f"SPD{N}"], fam.records), N))


@pytest.mark.parametrize("N", [3, 6])
def test_host_solve_spd_against_mpmath_and_oracle(L, O, N):
    fam = NC.spd_family(N)
    host = L.selftest_numerics(NC.FN[f"SPD{N}_HOST"], fam.records)  # no context: runs on the CPU
    _report(NC.check_spd(fam, host, N))
    assert np.array_equal(host.view(np.uint64), O.numerics(NC.FN[f"SPD{N}"], fam.records).view(np.uint64))


@pytest.mark.parametrize("N", [3, 6])
def test_oracle_jacobi_against_mpmath(O, N):
    fam = NC.jacobi_family(N)
    _report(NC.check_jacobi(fam, O.numerics(NC.FN[f"JACOBI{N}_HOST"], fam.records), N))


@pytest.mark.parametrize("N", [3, 6])
def test_host_jacobi_against_mpmath_and_oracle(L, O, N):
    fam = NC.jacobi_family(N)
    host = L.selftest_numerics(NC.FN[f"JACOBI{N}_HOST"], fam.records)
    _report(NC.check_jacobi(fam, host, N))
    assert np.array_equal(host.view(np.uint64), O.numerics(NC.FN[f"JACOBI{N}_HOST"], fam.records).view(np.uint64))


def test_oracle_residual_block_against_mpmath(O):
    fam = NC.accum_family()
    _report(NC.check_accum(fam, O.numerics(NC.FN["ACCUM"], fam.records)))


def test_oracle_pose_algebra_against_mpmath(O):
    fam = NC.pose_family()
    _report(NC.check_pose(fam, O.numerics(NC.FN["POSE"], fam.records)))


def test_families_reach_their_branches(O):
    """The case sets really reach the branches they were built for (as the oracle takes them)."""
    fam = NC.eig33_family(np.float32)
    out = O.numerics(NC.FN["EIG33_F"], fam.records)
    seen = {NC._eig_branch(o[0:3] / max(np.max(np.abs(r["M"])), 1e-300), np.float32) for o, r in zip(out, fam.refs)}
    assert seen == {"triple", "double-low", "double-high", "general"}, seen
    assert any(r.get("fallback") is not None for r in fam.refs)
    pose = NC.pose_family()
    assert any(r["gimbal"] for r in pose.refs) and any(r["slerp_linear"] for r in pose.refs) and any(not r["slerp_linear"] for r in pose.refs)
    spd = NC.spd_family(6)
    assert any(r["solvable"] for r in spd.refs) and any(not r["solvable"] for r in spd.refs)
