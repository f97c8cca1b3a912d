"""The host's trust-region loop (lidarslam_amd/csrc/host/lsa_lm_loop.cpp, driven by lsa_selftest_lm_host on scripted sums)
is held to the independent float64 statement of tests/lm_step_cases.py, bit for bit, on scripts that walk every branch:
the invalid-step retry and its reset, all eight ways of ending, the radius limits, the diagonal clamp, the acceptance
threshold, non-finite sums, 2D and 3D.  No device: tests/test_gpu_lm_step.py holds the device's step to the same records.

What the cases found: the gradient tolerance was tested on a maximum taken by comparisons, which drops a NaN -- a gradient
(1e-12, NaN, 1e-12, ...) ended the solve as converged ("gradient tolerance"), on the host and on the device.  Both now
test the entries one by one (nan_gradient_rest_under_tolerance).
"""
import os
import platform
import shutil
import subprocess

import numpy as np
import pytest

import lm_step_cases as LC
import numerics_cases as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(L):
    """(records, results, status) of the host loop on every case's script"""
    return L.selftest_lm_step([c.script for c in LC.cases()])


def test_every_case_reaches_its_branch_on_the_reference():
    """asserted on the reference's own trace -- codes, which evaluations were rejected or met invalid steps, the count of
    consecutive invalid steps, the radius at its limits: a re-tuned case cannot silently lose its branch"""
    cases = LC.cases()
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        c.check(c.ref)
        assert 1 <= len(c.sums) <= 40, c.name
        assert len(c.ref.records) == len(c.sums) and c.ref.code != LC.NONE, c.name
    for two_d in (False, True):
        codes = {c.ref.code for c in cases if c.two_d == two_d}
        assert codes == set(range(1, 9)), codes  # every way of ending but kCodeNone
    # the branches the solves on residual blocks never reached
    assert any(t["invalid"] for c in cases for t in c.ref.trace[1:]) and any(c.ref.invalid == 5 for c in cases)
    assert any(t.get("clamped_low") for c in cases for t in c.ref.trace) and not any(t.get("clamped_high") for c in cases for t in c.ref.trace)
    # (a negative model cost change needs no case of its own: with a positive diagonal D, step^T (Hs / 2 + D / radius) step
    # is positive whenever the damped matrix is positive definite; the overflow case walks its NaN instead)
    assert {"3d_threshold_above", "3d_threshold_below", "2d_threshold_above", "2d_threshold_below"} <= {c.name for c in cases}


def test_host_loop_equals_the_reference(host):
    cases = LC.cases()
    fails = LC.compare(cases, *host)
    print(f"{len(cases)} scripts, {sum(len(c.sums) for c in cases)} evaluations, {len(fails)} differ")
    assert not fails, "\n".join(fails)


def test_2d_mode_never_reads_the_inactive_sums_and_carries_z_rx_ry(host):
    """the rows and columns z, rx, ry of g and H are NaN in every 2D script: nothing of them reaches a record, and z, rx, ry
    of the start point pass through every candidate and every current point unchanged"""
    records = host[0]
    bad_inputs = ("negative_diagonal", "inf_", "nan_", "model_cost_change_overflows")
    seen = 0
    for c, rec in zip(LC.cases(), records):
        if not c.two_d:
            continue
        assert np.all(np.isnan(c.sums[:, [3, 4, 5]])) and np.all(np.isnan(c.sums[:, LC.hidx(2, 2)])), c.name
        keep = c.x0[2:5].view(np.uint64)
        assert np.all(keep != 0), c.name
        for source in (rec, np.array(c.ref.records)):
            going = source[source[:, 7] == 0]
            assert np.all(going[:, 2:5].view(np.uint64) == keep) and np.all(source[:, 25:28].view(np.uint64) == keep), c.name
            if not any(b in c.name for b in bad_inputs):
                assert np.all(np.isfinite(source)), c.name
                seen += 1
        assert np.all(c.ref.result()[2:5].view(np.uint64) == keep)
    assert seen >= 40


def test_a_script_that_runs_out_says_so(L):
    c = next(c for c in LC.cases() if c.name == "3d_valley")
    short = (c.two_d, c.max_iter, c.min_matches, c.x0, c.sums[:5])
    records, results, status = L.selftest_lm_step([short, c.script])
    assert status.tolist() == [[1, 5], [0, len(c.sums)]]
    assert np.array_equal(LC.canonical(records[0]), LC.canonical(np.array(c.ref.records[:5]))) and not results[0].any()
    assert not LC.compare([c], records[1:], results[1:], status[1:])
    with pytest.raises(L.LsaError):  # a negative max_iter is refused
        L.selftest_lm_step([(c.two_d, -1, 0, c.x0, c.sums)])


def test_the_references_damped_solve_against_mpmath():
    """every damped system the reference met, held to a 50-digit solve by the bound check_spd applies to solve_spd<N>:
    |x - x*| <= C_SPD kappa u |x*|; a system that is not positive definite (or not finite) must have been refused"""
    fails, total = [], 0
    for N in (3, 6):
        seen, recs, labels, refs, out = set(), [], [], [], []
        for c in LC.cases():
            if c.ref.n != N:
                continue
            for k, (M, b, ok, y) in enumerate(c.ref.systems):
                A = np.array([[M[max(i, j)][min(i, j)] for j in range(N)] for i in range(N)], np.float64)  # the triangle the factor reads
                b = np.array(b, np.float64)
                key = A.tobytes() + b.tobytes()
                if key in seen:
                    continue
                seen.add(key)
                ref = dict(solvable=False)
                if np.all(np.isfinite(A)) and np.all(np.isfinite(b)):
                    ev = NC._eigsy(A)[0]
                    if ev[0] > 0:
                        x = NC.mp.lu_solve(NC._mpmat(A), NC.mp.matrix([NC.mpf(float(v)) for v in b]))
                        xs = np.array([float(x[i]) for i in range(N)])
                        if not (0 < np.linalg.norm(xs) < np.inf):
                            continue  # (the overflow case: a solution whose norm is beyond the doubles has no relative error)
                        ref = dict(solvable=True, x=xs, kappa=float(ev[-1] / ev[0]))
                recs.append(np.concatenate([A.ravel(), b]))
                labels.append(f"{c.name} system {k}")
                refs.append(ref)
                out.append(np.concatenate([[1.0 if ok else 0.0], np.array(y, np.float64) if ok else np.zeros(N)]))
        fam = NC.Family(f"LM-REFERENCE-SPD{N}", np.array(recs), labels, refs)
        fails += NC.check_spd(fam, np.array(out), N)
        total += len(recs)
        assert sum(r["solvable"] for r in refs) >= 40 and sum(not r["solvable"] for r in refs) >= 10
    print(f"{total} systems")
    assert not fails, "\n".join(fails[:20])


def test_the_host_loop_is_clean_under_sanitizers(tmp_path):
    """the loop and its script driver in a stand-alone program with its own main, built for the CPU with Address + UB
    sanitizer, on every case's script; what it writes is the reference's, bit for bit.  Nothing loaded into Python runs
    under a sanitizer."""
    exe = str(tmp_path / "drv")
    host_dir = os.path.join(ROOT, "lidarslam_amd", "csrc", "host")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off"] + flags + [os.path.join(ROOT, "tests", "lm_loop_sanitize.cpp"),
                                                                             os.path.join(host_dir, "lsa_lm_loop.cpp"), "-o", exe]
    # whether this compiler has the sanitizers' runtime at all is decided on a program of one line; the build proper is then
    # asserted: an error in the driver or in the code under test is a failure, never a skip
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-std=c++17"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this compiler has no runtime for -fsanitize=address,undefined")
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    cases = LC.cases()
    header = np.array([(c.two_d, c.max_iter, c.min_matches, len(c.sums)) for c in cases], np.int32)
    scripts, answer = tmp_path / "scripts.bin", tmp_path / "out.bin"
    with open(scripts, "wb") as f:
        f.write(np.int32(len(cases)).tobytes() + header.tobytes() + np.array([c.x0 for c in cases], np.float64).tobytes()
                + np.concatenate([c.sums for c in cases]).tobytes())
    # the sanitizers' fixed shadow layout does not hold an executable placed by high-entropy ASLR: the driver runs with its
    # own address space unrandomized
    norand = ["setarch", platform.machine(), "-R"]
    if shutil.which("setarch") is None or subprocess.run(norand + ["true"], capture_output=True).returncode != 0:
        norand = []
    run = subprocess.run(norand + [exe, str(scripts), str(answer)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.startswith("ok"), (run.stdout[-1500:], run.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr
    total = int(header[:, 3].sum())
    raw = np.fromfile(answer, np.uint8)
    records = raw[:total * 42 * 8].view(np.float64).reshape(total, 42)
    results = raw[total * 42 * 8:(total * 42 + len(cases) * 45) * 8].view(np.float64).reshape(len(cases), 45)
    status = raw[(total * 42 + len(cases) * 45) * 8:].view(np.int32).reshape(len(cases), 2)
    ends = np.cumsum(header[:, 3])
    fails = LC.compare(cases, [records[e - k:e] for e, k in zip(ends, header[:, 3])], results, status)
    assert not fails, "\n".join(fails)
