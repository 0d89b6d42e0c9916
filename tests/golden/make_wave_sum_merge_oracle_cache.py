"""Writes the tests/golden/oracle/wsm_*.npz records: the float64 step reference (tests/step_reference.py: reference_loss)
for the seeded cases of tests/test_gpu_wave_sum_merge.py.  Run in the build container (no GPU needed):

    python tests/golden/make_wave_sum_merge_oracle_cache.py [-j 4] [-k substring]

It calls the SAME functions the test calls (conftest.cached_oracle with QC_WRITE_ORACLE_CACHE=1); the test checks the
inputs' digest before it trusts a record.  It also prints each case's margin of the test's pairwise-distinctness
condition, which is how the cases' seeds were chosen.  The records are data (arrays) from this repository's own oracle/
package."""
import argparse
import os
import sys
from concurrent.futures import ProcessPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.dirname(TESTS))
os.environ["QC_WRITE_ORACLE_CACHE"] = "1"


def run(case):
    import torch
    torch.set_num_threads(2)
    import test_gpu_wave_sum_merge as T
    ref = T.case_reference(case)
    return f"{case}: distinctness margin {T.distinct_margin(case, ref['grad']):.2f}"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=3)
    ap.add_argument("-k", default="")
    a = ap.parse_args()
    import test_gpu_wave_sum_merge as T
    todo = [c for c in T.CASES if a.k in c]
    with ProcessPoolExecutor(max_workers=a.j) as ex:
        for msg in ex.map(run, todo):
            print("done:", msg, flush=True)
