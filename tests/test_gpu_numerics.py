"""The device's fixed-size solvers, evaluated by the very templates the kernels inline (lsa_selftest_numerics), are bit
for bit the oracle's restatements AND within the mpmath bounds of tests/numerics_cases.py at the degenerate inputs
synthetic scans never reach."""
import numpy as np
import pytest

import numerics_cases as NC
from conftest import bits

pytestmark = pytest.mark.gpu


def _canonical_nan(a):
    # IEEE 754 leaves a NaN's sign and payload to the hardware: x86 produces the negative default NaN where the GPU
    # produces the positive canonical one (seen in the x a failed solve_spd leaves behind).  NaN must match NaN; every
    # other value must match bit for bit.
    a = np.array(a, np.float64)
    a[np.isnan(a)] = np.nan
    return a


def _parity(name, fam, dev, ref):
    same = np.all(bits(_canonical_nan(dev)) == bits(_canonical_nan(ref)), axis=1)
    bad = np.nonzero(~same)[0]
    assert bad.size == 0, f"{name}: device differs from the oracle in {bad.size} case(s): " + "; ".join(
        f"case {i} [{fam.labels[i]}]: {dev[i].tolist()} vs {ref[i].tolist()}" for i in bad[:5])


def _report(fails):
    assert not fails, f"{len(fails)} violation(s):\n" + "\n".join(fails[:25])


CASES = [
    ("PCA_F", lambda: NC.pca_family(), lambda f, o: NC.check_pca(f, o, np.float32)),
    ("PCA_D", lambda: NC.pca_family(), lambda f, o: NC.check_pca(f, o, np.float64)),
    ("EIG33_F", lambda: NC.eig33_family(np.float32), lambda f, o: NC.check_eig33(f, o, np.float32)),
    ("EIG33_D", lambda: NC.eig33_family(np.float64), lambda f, o: NC.check_eig33(f, o, np.float64)),
    ("SPD3", lambda: NC.spd_family(3), lambda f, o: NC.check_spd(f, o, 3)),
    ("SPD6", lambda: NC.spd_family(6), lambda f, o: NC.check_spd(f, o, 6)),
    ("ACCUM", lambda: NC.accum_family(), lambda f, o: NC.check_accum(f, o)),
    ("POSE", lambda: NC.pose_family(), lambda f, o: NC.check_pose(f, o)),
]


@pytest.mark.parametrize("name,family,check", CASES, ids=[c[0] for c in CASES])
def test_device_numerics_match_oracle_and_mpmath(gpu_ctx, O, name, family, check):
    fam = family()
    dev = gpu_ctx.selftest_numerics(NC.FN[name], fam.records)
    _parity(name, fam, dev, O.numerics(NC.FN[name], fam.records))
    _report(check(fam, dev))
