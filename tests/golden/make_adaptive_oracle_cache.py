"""Writes the tests/golden/oracle/adapt_ujets_*.npz records: the float64 CPU oracle's six channels of u on the seeded
datasets of tests/test_gpu_adaptive_scores.py (tests/adaptive_scores_reference.py).  The companion of
make_coef_oracle_cache.py; run in the build container (no GPU needed):

    python tests/golden/make_adaptive_oracle_cache.py [-k substring]

It calls the SAME function the tests call (conftest.cached_oracle with QC_WRITE_ORACLE_CACHE=1); the tests check the
inputs' digest before they trust a record.  The records are data (arrays) from this repository's own oracle/ package."""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.dirname(TESTS))
os.environ["QC_WRITE_ORACLE_CACHE"] = "1"

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("-k", default="")
    a = ap.parse_args()
    import adaptive_scores_reference as SR
    for case in SR.CASES:
        if a.k in case:
            print("done:", case, SR.case_ujets(case).shape, flush=True)
